#!/usr/bin/env python3
"""Record tests/golden/host_errors.json: the return code and bj_last_error() text of every rejected call in
tests/host_error_cases.py, from a library built at the commit BEFORE a change of the host code, so that
tests/test_host_errors.py holds the changed code to the earlier behaviour.

    git worktree add /tmp/parent HEAD~ && make -C /tmp/parent/era-boojum_amd
    python3 tools/record_host_errors.py --lib /tmp/parent/era-boojum_amd/boojum_amd/libboojum_mi355x.so

The host cases need no GPU.  The device cases (a local group's events) are recorded only with --device,
on a machine with one; without it their earlier entries in the file are kept.

--cases names another module of cases in the same format, with --out its golden: the gate-set validator's are
tests/gate_check_cases.py and tests/golden/gate_check_errors.json.
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "era-boojum_amd"), os.path.join(ROOT, "tests")]
GOLDEN = os.path.join(ROOT, "tests", "golden", "host_errors.json")


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--lib", required=True, help="libboojum_mi355x.so built at the earlier commit")
    ap.add_argument("--device", action="store_true", help="record the cases that need a GPU as well")
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--cases", default="host_error_cases", help="the module under tests/ that holds the cases")
    args = ap.parse_args()
    from boojum_amd import _lib
    import importlib
    cases = importlib.import_module(args.cases)
    L = ctypes.CDLL(os.path.abspath(args.lib))
    for name, (argtypes, restype) in _lib.SIGNATURES.items():
        fn = getattr(L, name)
        fn.argtypes, fn.restype = argtypes, restype
    try:
        golden = json.load(open(args.out))
    except OSError:
        golden = {}
    golden.update(cases.run(L, cases.HOST))
    if args.device:
        golden.update(cases.run(L, cases.DEVICE))
    known = {n for n, _ in cases.HOST + cases.DEVICE}
    golden = {k: v for k, v in golden.items() if k in known}
    with open(args.out, "w") as f:
        json.dump(golden, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d cases in %s" % (len(golden), args.out))


if __name__ == "__main__":
    main()
