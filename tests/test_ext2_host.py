"""csrc/ext2.hpp on the host (deep.hip's launchers take their Ext2 product from it): tests/c/ext2_host.cpp
built with the host compiler alone, against field.ext2_mul on Python integers."""
import itertools
import os
import random
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "ext2_host.cpp")


def test_ext2_host_matches_python_integers(tmp_path):
    from boojum_amd.field import EXT2_NON_RESIDUE, P, ext2_mul
    # every word of the C ABI is legal, canonical or not; the outputs are compared canonical
    edges = (0, 1, P - 1, P, 2**32 - 1, 2**32, 2**64 - 1)
    rng = random.Random(0x45787432)
    rows = list(itertools.product(edges, repeat=4))
    rows += [tuple(rng.randrange(2**64) for _ in range(4)) for _ in range(400)]
    binary = str(tmp_path / "ext2_host")
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-o", binary, SRC], check=True)
    text = "".join("%d %d %d %d\n" % r for r in rows)
    out = subprocess.run([binary], input=text, capture_output=True, text=True, check=True, timeout=60).stdout
    got = [tuple(int(w) for w in line.split()) for line in out.splitlines()]
    assert len(got) == len(rows)
    for (a0, a1, b0, b1), g in zip(rows, got):
        m = ext2_mul((a0, a1), (b0, b1))
        want = (m[0], m[1], (a0 * a0 - EXT2_NON_RESIDUE * a1 * a1) % P, EXT2_NON_RESIDUE * a0 % P)
        assert g == want, (a0, a1, b0, b1)
