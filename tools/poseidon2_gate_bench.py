#!/usr/bin/env python3
"""Measurement of the native Poseidon2 flattened gate (a kind-1 segment of a gate set,
csrc/gates_poseidon2.hpp) through bj_quotient_gate_terms_d at the reference proof's shape: 2^20 rows,
130 variable columns, quotient degree 8, so 2^23 points, one instance per point, no witness columns,
no selector.  The columns are synthetic: the kernel's work does not depend on the values.  Timed
with HIP events on the stream the call runs on, everything in one run.

* alg_bytes: 132 words per point -- the 130 cells read once and the accumulator's two words.
* copy: torch's device-to-device copy of alg_bytes / 2 bytes (its rate counts bytes read plus
  bytes written).
* slot_floor: the field operations of one point priced as tools/gates_bench.py prices them, a
  product at 14 instructions and an addition or subtraction at 8, two issue slots each, over the
  78.6 T lane issue slots/s of the GPU.  Counted from the kernel's structure (operation_counts);
  a multiplication by 2^k of the inner matrix is priced as an addition.  Addressing is scalar work
  and not in it.
* eight_gate_set: the same call on the interpreted set of tools/gates_bench.py, for scale.

usage: python tools/poseidon2_gate_bench.py [log_n=20] [q=8]   (prints one JSON line)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "era-boojum_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gates_bench import ADD_SLOTS, HBM_PEAK_GBS, MUL_SLOTS, VALU_PEAK_SLOTS, bench_set, timed   # noqa: E402

CELLS, TERMS = 130, 118


def operation_counts():
    """Products, additions / subtractions and shifts by 2^k of one instance, as the kernel forms it."""
    full, partial, sw = 8, 22, 12
    external = 3 * (8 + 6) + 4 * 5            # three M4 (8 additions, 6 doublings), then the column sums
    mul = full * sw * 4 + partial * 4 + 2 * TERMS
    add = ((full + 1) * external              # the first matrix and one per full round
           + full * sw + partial              # round constants
           + partial * (11 + sw)              # inner matrix: the sum, then sum + shifted element
           + TERMS                            # expected - cell
           + 2 * TERMS + 2)                   # the challenge sums and the accumulator
    shifts = partial * (sw - 1)               # one diagonal element is 2^0
    return mul, add, shifts


def main():
    import numpy as np
    import torch
    from boojum_amd import gates as G
    from boojum_amd._lib import call
    from boojum_amd.field import P, stream_of
    log_n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    q = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    if not torch.cuda.is_available():
        raise SystemExit("poseidon2_gate_bench needs a GPU")
    log_q = q.bit_length() - 1
    total = q << log_n
    native = G.GateSet([G.GatePlacement(G.program_of(G.Poseidon2FlattenedGate(CELLS, 0)), 1)])
    eight = G.GateSet(bench_set(G, CELLS))
    n_consts = eight.need["constants"]
    cols = torch.empty((CELLS + n_consts, q, 1 << log_n), dtype=torch.int64, device="cuda")
    call("bj_fill_synthetic_d", cols.data_ptr(), cols.shape[0], total, log_n + log_q, 7, 0, stream_of(cols))
    rng = np.random.default_rng(1)
    k = max(native.need["alphas"], eight.need["alphas"])
    alphas = G.challenges_tensor([tuple(int(v) for v in pair) for pair in
                                  rng.integers(0, P, size=(k, 2), dtype=np.uint64)], "cuda")
    dst = torch.zeros((2, total), dtype=torch.int64, device="cuda")
    variables, constants = cols[:CELLS], cols[CELLS:]

    t = timed(torch, lambda: G.evaluate_gate_terms(native, variables, None, None, alphas, q, dst[0], dst[1]), 10)
    t_eight = timed(torch, lambda: G.evaluate_gate_terms(eight, variables, None, constants, alphas, q, dst[0], dst[1]),
                    10)
    nbytes = (CELLS + 2) * total * 8
    words = nbytes // 16
    dst1 = torch.empty((words,), dtype=torch.int64, device="cuda")
    src1 = cols.reshape(-1)
    t_copy = timed(torch, lambda: dst1.copy_(src1[:words]), 10)
    copy_gbs = 2 * words * 8 / t_copy / 1e9
    mul, add, shifts = operation_counts()
    slots = mul * MUL_SLOTS + (add + shifts) * ADD_SLOTS
    floor = total * slots / VALU_PEAK_SLOTS
    gbs = nbytes / t / 1e9
    line = {
        "shape": "%d variable columns x 2^%d rows, quotient degree %d (2^%d points), one instance per point"
                 % (CELLS, log_n, q, log_n + log_q),
        "device": torch.cuda.get_device_name(0),
        "segment": {"kind": G.KIND_POSEIDON2, "terms": TERMS, "num_witness_columns_used": 0, "launches": 1},
        "gate_terms": {
            "ms": t * 1e3, "alg_bytes_per_call": nbytes, "achieved": gbs, "unit": "GB/s", "peak": HBM_PEAK_GBS,
            "frac_of_hbm_peak": gbs / HBM_PEAK_GBS,
            "copy": {"bytes_copied": words * 8, "ms": t_copy * 1e3, "read_plus_write_gbs": copy_gbs},
            "vs_copy": gbs / copy_gbs,
            "per_point": {"products": mul, "additions": add, "shifts": shifts},
            "slot_floor": {"slots_per_product": MUL_SLOTS, "slots_per_addition": ADD_SLOTS, "slots_per_point": slots,
                           "ms": floor * 1e3, "frac_of_slot_floor": floor / t},
            "bound_by": "slot_floor" if floor > t_copy else "copy",
        },
        "eight_gate_set": {"ms": t_eight * 1e3, "launches": eight.num_segments, "challenges": eight.need["alphas"]},
    }
    print(json.dumps(line))


if __name__ == "__main__":
    main()
