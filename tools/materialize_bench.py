#!/usr/bin/env python3
"""Times the witness gather (bj_materialize_columns_d) and the sigma kernel (bj_permutation_polys_d)
beside a device-to-device copy of the same output bytes, at the reference proof's shape 2^20 x 130.

usage: python tools/materialize_bench.py [log_n] [n_vars] [uses] [--cols C] [--reps R] [--log PATH]

Two SYNTHETIC placements -- nobody has measured a real circuit's -- in both of which every variable
is used `uses` times (default 4; n_vars defaults to cells / uses):
  row_by_row      variables are allocated along the rows, so neighbouring cells of a row hold
                  neighbouring indices (cell (r, c) names variable (r * C + c) // uses);
  uniform_random  the same multiset of indices, shuffled uniformly over the cells.
Each gather is timed with device events, alternating with the copy in the same run; the figures
are medians and the ratio is gather / copy.  Prints one JSON line and appends it to the log."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "era-boojum_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from boojum_amd import field, witness  # noqa: E402


def placements(n_cols, n, n_vars, uses, seed=1):
    cells = n_cols * n
    k = np.arange(cells, dtype=np.uint64).reshape(n, n_cols)           # row-major cell number
    row_by_row = np.ascontiguousarray(((k // np.uint64(uses)) % np.uint64(n_vars)).T)
    flat = row_by_row.reshape(-1).copy()
    np.random.default_rng(seed).shuffle(flat)
    return {"row_by_row": row_by_row, "uniform_random": flat.reshape(n_cols, n)}


def alternate(run_a, run_b, reps, warmup=3):
    """Medians (ms) of run_a and run_b, alternated: a b a b ..."""
    times = ([], [])
    for i in range(warmup + reps):
        for which, run in enumerate((run_a, run_b)):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            run()
            stop.record()
            stop.synchronize()
            if i >= warmup:
                times[which].append(start.elapsed_time(stop))
    return float(np.median(times[0])), float(np.median(times[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("log_n", nargs="?", type=int, default=20)
    ap.add_argument("n_vars", nargs="?", type=int, default=0)
    ap.add_argument("uses", nargs="?", type=int, default=4)
    ap.add_argument("--cols", type=int, default=130)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-sigma", action="store_true", help="time the gathers only")
    ap.add_argument("--label", default="", help="a note for the JSON line (a build variant)")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "materialize_bench.log"))
    a = ap.parse_args()
    n, c = 1 << a.log_n, a.cols
    n_vars = a.n_vars or max(1, c * n // a.uses)
    values = field.to_device(np.random.default_rng(2).integers(0, field.P, size=n_vars, dtype=np.uint64))
    out = torch.empty((c, n), dtype=torch.int64, device="cuda")
    src = torch.empty_like(out)
    result = {"tool": "materialize_bench", "synthetic_placements": True, "log_n": a.log_n, "cols": c, "n_vars": n_vars,
              "uses": a.uses, "reps": a.reps, "output_bytes": 8 * c * n, "all_values_bytes": 8 * n_vars,
              "packed_hint_bytes": 4 * c * n, "device": torch.cuda.get_device_name(0)}
    sigma_maps = None
    for name, maps in placements(c, n, n_vars, a.uses).items():
        hint = witness.CopyHint(maps)
        hint.upload()
        gather_ms, copy_ms = alternate(lambda: witness.materialize_columns(hint, values, out), lambda: out.copy_(src),
                                       a.reps)
        hint.release()
        result[name] = {"gather_ms": round(gather_ms, 4), "copy_ms": round(copy_ms, 4),
                        "gather_over_copy": round(gather_ms / copy_ms, 3),
                        "output_GBps": round(8 * c * n / gather_ms / 1e6, 1)}
        if sigma_maps is None:
            sigma_maps = maps
    if a.label:
        result["label"] = a.label
    if not a.skip_sigma:
        sigma(result, sigma_maps, c, n, out, src, a.reps)
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(a.log), exist_ok=True)
    with open(a.log, "a") as f:
        f.write(line + "\n")


def sigma(result, sigma_maps, c, n, out, src, reps):
    # the sigma kernel on the row_by_row placement: the whole call (its table included) beside the copy
    from boojum_amd._lib import call
    from boojum_amd.stage2 import non_residues_for_copy_permutation
    import ctypes
    prev = torch.from_numpy(witness.prev_map(sigma_maps).view(np.int32)).to("cuda")
    k = (ctypes.c_uint64 * c)(*non_residues_for_copy_permutation(n, c))
    sigma_ms, copy_ms = alternate(
        lambda: call("bj_permutation_polys_d", prev.data_ptr(), c, n, k, out.data_ptr(), n, field.stream_of(out)),
        lambda: out.copy_(src), reps)
    result["sigma"] = {"sigma_ms": round(sigma_ms, 4), "copy_ms": round(copy_ms, 4),
                       "sigma_over_copy": round(sigma_ms / copy_ms, 3), "placement": "row_by_row"}


if __name__ == "__main__":
    main()
