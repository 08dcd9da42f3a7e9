"""csrc/host.hpp on the host alone: tests/c/host_shim.cpp, built with the host compiler the way test_ext2_host.py
builds its program, checks is_pow2 and log2u at their edges, the "<what>: <the runtime's text>" message of a
failed runtime call, and that the workspace and the event set free what they made, in order, and call nothing
when they made nothing.  Needs no GPU: only hipGetErrorString comes from the HIP runtime."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "host_shim.cpp")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_host_shim(tmp_path):
    binary = str(tmp_path / "host_shim")
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__",
                    "-isystem", os.path.join(ROCM, "include"), "-o", binary, SRC,
                    "-L" + os.path.join(ROCM, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(ROCM, "lib")],
                   check=True)
    r = subprocess.run([binary], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "host shim ok"
