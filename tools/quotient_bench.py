#!/usr/bin/env python3
"""Measurement of the quotient block at the reference proof's shape (130 copy-permutation columns,
n = 2^20, quotient degree 8, so 2^23 points): the copy-permutation call
(bj_quotient_copy_permutation_d, prover.rs:1148-1227 and copy_permutation.rs:1000-1249), one lookup
term (bj_quotient_lookup_term_d, lookup_argument_in_ext.rs:949-1310; four sources and a multiplicity
column), the division (bj_quotient_divide_vanishing_d, utils.rs:770-817) and the monomial step
(bit reversal + inverse transform of the two halves at q n, prover.rs:1399-1445), timed with HIP
events on the stream they run on.  Nothing existing computes these on the device, so the yardstick
of the first three is a device-to-device copy of the same number of bytes in the same run on the
same GPU.  The columns are synthetic: the kernels' work does not depend on the values.

* copy_permutation: algorithmic bytes per call = 2*C*q*n*8 (variable and sigma LDE columns) +
  2*m*q*n*8 (z and the intermediates) + 4*q*n*8 (the accumulator read and written); the shifted
  read of z comes on top and is not counted.
* lookup_term: (n_src + 3)*q*n*8 read + 4*q*n*8 for the accumulator.
* divide: 4*q*n*8.
* copy: torch's device-to-device copy of alg_bytes / 2 bytes, whose rate counts the bytes read plus
  the bytes written, so that it moves as many bytes as the call.
* "vs_copy" is the call's algorithmic rate over the copy's.  "slot_floor" prices the
  copy-permutation kernel by a static census of its code object (issue slots of one trip of the
  column loop, which serves the thread's two points; the shared inversion chain, 74 products over
  the two points, and one Ext2 product by alpha per relation, both at the loop's cost per product;
  tools/valu_census.py's weights) against the 78.6 T lane issue slots/s of the GPU;
  "frac_of_slot_floor" is that time over the call's.

usage: python tools/quotient_bench.py [log_n=20] [n_cols=130] [q=8]   (prints one JSON line)
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
QP_ROWS = 2                              # csrc/quotient.hip: points of a thread
PRODUCTS_PER_TRIP = QP_ROWS * 12         # base-field products of one trip of the column loop
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


def cp_census():
    """Issue slots per lane of quotient_cp_kernel from its disassembly: one trip of the column loop
    (the innermost loop that loads two columns for each of the thread's points), and everything
    else once.  None when the toolchain is not at hand."""
    try:
        import valu_census as V
        ins = V.parse(V.kernel_lines(V.disassemble("quotient"), "quotient_cp_kernel"))
    except (Exception, SystemExit):
        return None
    base = ins[0][0]
    loops = []
    for i, (a, _, t) in enumerate(ins):
        if t is not None and base + t < a:
            start = next(k for k, (aa, _, _) in enumerate(ins) if aa == base + t)
            body = ins[start:i + 1]
            if sum(1 for _, mn, _ in body if mn.startswith("global_load")) == 2 * QP_ROWS:
                loops.append((i - start, V.straight_line(body)[1]))
    if not loops:
        return None
    column = min(loops)[1]
    return {"slots_per_column_trip": column, "points_per_trip": QP_ROWS,
            "slots_straight_line": V.straight_line(ins)[1], "slots_per_product": column / float(PRODUCTS_PER_TRIP)}


def main():
    import numpy as np
    import torch
    from boojum_amd import stage2
    from boojum_amd._lib import call
    from boojum_amd.field import GENERATOR, P, stream_of
    log_n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    n_cols = int(sys.argv[2]) if len(sys.argv) > 2 else 130
    q = int(sys.argv[3]) if len(sys.argv) > 3 else 8
    if not torch.cuda.is_available():
        raise SystemExit("quotient_bench needs a GPU")
    log_q = q.bit_length() - 1
    n = 1 << log_n
    total = n * q
    m = (n_cols + q - 1) // q
    # variables, then sigmas, then the 2 m stage-2 columns: LDE columns of q n words each
    cols = torch.empty((2 * n_cols + 2 * m, total), dtype=torch.int64, device="cuda")
    call("bj_fill_synthetic_d", cols.data_ptr(), cols.shape[0], total, log_n + log_q, 7, 0, stream_of(cols))
    rng = np.random.default_rng(1)
    beta, gamma = (tuple(int(v) for v in rng.integers(0, P, size=2, dtype=np.uint64)) for _ in range(2))
    k = (ctypes.c_uint64 * n_cols)(*stage2.non_residues_for_copy_permutation(n, n_cols))
    alphas = (ctypes.c_uint64 * (2 * (m + 1)))(*[int(v) for v in rng.integers(0, P, size=2 * (m + 1), dtype=np.uint64)])
    dst = torch.zeros((2, total), dtype=torch.int64, device="cuda")
    st = stream_of(cols)

    def copy_permutation():
        call("bj_quotient_copy_permutation_d", cols.data_ptr(), total, cols[n_cols].data_ptr(), total,
             cols[2 * n_cols].data_ptr(), total, n_cols, log_n, log_q, k, beta[0], beta[1], gamma[0], gamma[1], alphas,
             dst[0].data_ptr(), dst[1].data_ptr(), st)

    srcs = (ctypes.c_void_p * LOOKUP_SOURCES)(*[cols[t].data_ptr() for t in range(LOOKUP_SOURCES)])
    g = (ctypes.c_uint64 * (2 * LOOKUP_SOURCES))(*[int(v) for v in rng.integers(0, P, size=2 * LOOKUP_SOURCES,
                                                                               dtype=np.uint64)])

    def lookup():
        call("bj_quotient_lookup_term_d", srcs, LOOKUP_SOURCES, g, beta[0], beta[1], cols[2 * n_cols].data_ptr(),
             cols[2 * n_cols + 1].data_ptr(), cols[LOOKUP_SOURCES].data_ptr(), gamma[0], gamma[1], log_n, log_q,
             dst[0].data_ptr(), dst[1].data_ptr(), st)

    def divide():
        call("bj_quotient_divide_vanishing_d", dst[0].data_ptr(), dst[1].data_ptr(), log_n, log_q, st)

    def monomials():
        call("bj_bitreverse_enumeration_d", dst.data_ptr(), 2, total, log_n + log_q, st)
        call("bj_ifft_natural_to_natural_d", dst.data_ptr(), 2, total, log_n + log_q, GENERATOR, None, st)

    t_cp = timed(torch, copy_permutation, 30)
    t_lk = timed(torch, lookup, 1000)
    t_dv = timed(torch, divide, 2000)
    t_mono = timed(torch, monomials, 200)
    cp_bytes = (2 * n_cols + 2 * m + 4) * total * 8
    lk_bytes = (LOOKUP_SOURCES + 3 + 4) * total * 8
    dv_bytes = 4 * total * 8
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

    cp = row(t_cp, cp_bytes, 30)
    census = cp_census()
    if census:
        # per point: the column trips' share, the shared inversion's share, and per relation one
        # Ext2 product by alpha (4 products); the rest of the straight-line code runs once per thread
        per_point = (n_cols * census["slots_per_column_trip"] / QP_ROWS
                     + 74 * census["slots_per_product"] / QP_ROWS + m * 4 * census["slots_per_product"])
        floor = total * per_point / VALU_PEAK_SLOTS
        cp["slot_floor"] = {"census": census, "slots_per_point": per_point, "ms": floor * 1e3,
                            "frac_of_slot_floor": floor / t_cp}
    line = {
        "shape": "%d columns x 2^%d rows, quotient degree %d (%d relations, 2^%d points)" % (n_cols, log_n, q, m,
                                                                                            log_n + log_q),
        "device": torch.cuda.get_device_name(0),
        "copy_permutation": cp,
        "lookup_term": dict(row(t_lk, lk_bytes, 1000), n_src=LOOKUP_SOURCES, with_f=True),
        "divide_vanishing": row(t_dv, dv_bytes, 2000),
        "monomials": {"ms": t_mono * 1e3, "columns": 2, "log_size": log_n + log_q},
    }
    print(json.dumps(line))


if __name__ == "__main__":
    main()
