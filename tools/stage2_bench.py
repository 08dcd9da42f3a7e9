#!/usr/bin/env python3
"""Measurement of stage 2 at the reference proof's shape (130 copy-permutation columns, n = 2^20,
chunk 8): the copy-permutation call (bj_copy_permutation_d, copy_permutation.rs:649-774) and one
lookup encoding (bj_lookup_encoding_d, lookup_argument_in_ext.rs:320-700; four sources and a
multiplicity column), timed with HIP events on the stream they run on.  Nothing existing computes
these on the device, so the yardstick is a device-to-device copy of the same number of bytes in
the same run on the same GPU.

* copy_permutation: algorithmic bytes per call = 2*C*n*8 (witness and sigma columns read) +
  2*m*n*8 (z and the intermediates written); the in-place passes over the outputs come on top and
  are not counted.
* lookup_encoding: (n_src + 1)*n*8 read + 2*n*8 written.
* copy: torch's device-to-device copy of alg_bytes / 2 bytes, whose rate counts the bytes read plus
  the bytes written, so that it moves as many bytes as the call.
* "vs_copy" is the call's algorithmic rate over the copy's.  "slot_floor" prices the rational
  pass by a static census of its code object (issue slots of one trip of the column loop, the
  inversion chain and the rest, tools/valu_census.py's weights) against the 78.6 T lane issue
  slots/s of the GPU; "frac_of_slot_floor" is that time over the whole call's.

usage: python tools/stage2_bench.py [log_n=20] [n_cols=130] [chunk=8]   (prints one JSON line)
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "era-boojum_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_PEAK_GBS = 8000.0
VALU_PEAK_SLOTS = 256 * 4 * 32 * 2.4e9   # lane issue slots/s (bench.py VALU_PEAK_TOPS)
CP_MP = 16                               # csrc/stage2.hip: chunks that share one inversion, at most
LOOKUP_SOURCES = 4


def timed(torch, fn, reps):
    st = torch.cuda.current_stream()
    fn()
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(reps):
        fn()
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3


def rational_census():
    """Issue slots per lane of cp_rational_kernel from its disassembly: one trip of the column
    loop (the innermost loop that loads the two columns), one 64-bit inversion chain (its squaring
    loops run 64 trips in all; priced as 74 products of the loop's cost per product), and
    everything else once.  None when the toolchain is not at hand."""
    try:
        import valu_census as V
        ins = V.parse(V.kernel_lines(V.disassemble("stage2"), "cp_rational_kernel"))
    except (Exception, SystemExit):
        return None
    base = ins[0][0]
    loops = []
    for i, (a, _, t) in enumerate(ins):
        if t is not None and base + t < a:
            start = next(k for k, (aa, _, _) in enumerate(ins) if aa == base + t)
            body = ins[start:i + 1]
            if sum(1 for _, mn, _ in body if mn.startswith("global_load")) == 2:
                loops.append((i - start, V.straight_line(body)[1]))
    if not loops:
        return None
    column = min(loops)[1]
    total = V.straight_line(ins)[1]
    return {"slots_per_column": column, "slots_straight_line": total, "slots_per_product": column / 12.0}


def main():
    import numpy as np
    import torch
    from boojum_amd import stage2
    from boojum_amd._lib import call
    from boojum_amd.field import P, stream_of
    log_n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    n_cols = int(sys.argv[2]) if len(sys.argv) > 2 else 130
    chunk = int(sys.argv[3]) if len(sys.argv) > 3 else 8
    if not torch.cuda.is_available():
        raise SystemExit("stage2_bench needs a GPU")
    n = 1 << log_n
    m = (n_cols + chunk - 1) // chunk
    cols = torch.empty((2 * n_cols, n), dtype=torch.int64, device="cuda")   # witness, then sigma
    call("bj_fill_synthetic_d", cols.data_ptr(), 2 * n_cols, n, log_n, 7, 0, stream_of(cols))
    rng = np.random.default_rng(1)
    beta, gamma = (tuple(int(v) for v in rng.integers(0, P, size=2, dtype=np.uint64)) for _ in range(2))
    k = (ctypes.c_uint64 * n_cols)(*stage2.non_residues_for_copy_permutation(n, n_cols))
    out = torch.empty((2 * m, n), dtype=torch.int64, device="cuda")
    status = torch.zeros((4,), dtype=torch.int64, device="cuda")
    st = stream_of(cols)

    def copy_permutation():
        call("bj_copy_permutation_d", cols.data_ptr(), n, cols[n_cols].data_ptr(), n, n_cols, log_n, k, beta[0], beta[1],
             gamma[0], gamma[1], chunk, out.data_ptr(), n, status.data_ptr(), st)

    srcs = (ctypes.c_void_p * LOOKUP_SOURCES)(*[cols[t].data_ptr() for t in range(LOOKUP_SOURCES)])
    g = (ctypes.c_uint64 * (2 * LOOKUP_SOURCES))(*[int(v) for v in rng.integers(0, P, size=2 * LOOKUP_SOURCES,
                                                                               dtype=np.uint64)])

    def lookup():
        call("bj_lookup_encoding_d", srcs, LOOKUP_SOURCES, g, beta[0], beta[1], cols[LOOKUP_SOURCES].data_ptr(), log_n,
             out[0].data_ptr(), out[1].data_ptr(), status.data_ptr(), st)

    t_cp = timed(torch, copy_permutation, 20)
    t_lk = timed(torch, lookup, 200)
    cp_bytes = 2 * n_cols * n * 8 + 2 * m * n * 8
    lk_bytes = (LOOKUP_SOURCES + 1) * n * 8 + 2 * n * 8
    # the yardstick: device-to-device copies that move as many bytes (read + written) as each call
    src1 = cols.reshape(-1)
    dst1 = torch.empty((cp_bytes // 16,), dtype=torch.int64, device="cuda")

    def copy_of(nbytes, reps):
        words = nbytes // 16
        t = timed(torch, lambda: dst1[:words].copy_(src1[:words]), reps)
        return t, 2 * words * 8 / t / 1e9, words * 8

    def row(t, nbytes, reps):
        t_copy, copy_gbs, copied = copy_of(nbytes, reps)
        gbs = nbytes / t / 1e9
        return {"ms": t * 1e3, "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac_of_hbm_peak": gbs / HBM_PEAK_GBS,
                "alg_bytes_per_call": nbytes,
                "copy": {"bytes_copied": copied, "ms": t_copy * 1e3, "read_plus_write_gbs": copy_gbs},
                "vs_copy": gbs / copy_gbs}

    cp = row(t_cp, cp_bytes, 50)
    census = rational_census()
    if census:
        groups = (m + CP_MP - 1) // CP_MP
        per_row = n_cols * census["slots_per_column"] + groups * 74 * census["slots_per_product"]
        floor = n * per_row / VALU_PEAK_SLOTS
        cp["slot_floor"] = {"census": census, "inversions_per_row": groups, "slots_per_row": per_row,
                            "ms": floor * 1e3, "frac_of_slot_floor": floor / t_cp}
    line = {
        "shape": "%d columns x 2^%d rows, chunk %d (%d output columns)" % (n_cols, log_n, chunk, 2 * m),
        "device": torch.cuda.get_device_name(0),
        "copy_permutation": cp,
        "lookup_encoding": dict(row(t_lk, lk_bytes, 200), n_src=LOOKUP_SOURCES, with_f=True),
    }
    print(json.dumps(line))


if __name__ == "__main__":
    main()
