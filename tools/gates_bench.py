#!/usr/bin/env python3
"""Measurement of the quotient's gate terms (bj_quotient_gate_terms_d, csrc/gates.hip) at the
reference proof's shape: 2^20 rows, 130 variable columns, quotient degree 8, so 2^23 points.

The gate set is fixed and synthetic: the eight evaluators of boojum_amd.gates (ZeroCheck with the
inversion in a variable column) at their repetition counts for 130 variable, 4 witness and 8
constant columns, each under its own leaf of a depth-3 selector tree, so 3 selector columns and the
gates' own constants from column 3 on (11 constant columns).  The columns are synthetic: the
kernel's work does not depend on the values.  Timed with HIP events on the stream the call runs on.

* alg_bytes: every column the set names read once, (variables + constants) * q n * 8, plus the
  accumulator read and written, 4 * q n * 8.  The gates re-read the variable columns (each of the
  eight walks all 130); those re-reads are served by the caches or not, and are not counted.
* copy: torch's device-to-device copy of alg_bytes / 2 bytes in the same run (its rate counts bytes
  read plus bytes written).
* slot_floor: the field operations of one point priced in VALU issue slots, a product (four
  v_mad_u64_u32 and the reduction) at 14 instructions and an addition or subtraction at 8, two
  slots each as tools/valu_census.py weighs carry, 64-bit and multiply instructions, over the
  78.6 T lane issue slots/s of the GPU.  Counted from the programs: the relations of every
  repetition, two products and two additions per term for the challenge, the selector path and
  the two products by the selector per gate.  Decode, addressing and LDS traffic are not in it.
* library: the same placements, columns and challenges through GateSet(placements,
  native_library=True), whose gates run the generated straight-line walks (csrc/gates_library.hpp).
  Three rounds alternate the interpreted and the library set (10 calls each per round); both medians,
  every round's time, the launches and the ratio to the interpreted median are reported.  The first
  round of the interpreted set is "gate_terms", as before.

usage: python tools/gates_bench.py [log_n=20] [n_vars=130] [q=8]   (prints one JSON line)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "era-boojum_amd"))

HBM_PEAK_GBS = 8000.0
VALU_PEAK_SLOTS = 256 * 4 * 32 * 2.4e9   # lane issue slots/s (bench.py VALU_PEAK_TOPS)
MUL_SLOTS, ADD_SLOTS = 14 * 2, 8 * 2


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


def bench_set(G, n_vars):
    geometry = G.CSGeometry(n_vars, 4, 8, 8)
    evaluators = [e for e in G.library() if e.name != "zero_check_witness"]
    paths = [[bool(i >> b & 1) for b in range(3)] for i in range(len(evaluators))]
    return G.layout_general_purpose(list(zip(evaluators, paths)), geometry)


def operation_counts(placements):
    """(products, additions) of one point, and the temporaries stored."""
    mul = add = stores = 0
    for pl in placements:
        m = sum(1 for _, r in pl.program.relations if r.kind in ("Mul", "Square"))
        a = len(pl.program.relations) - m
        terms = pl.program.num_quotient_terms
        mul += pl.num_repetitions * (m + 2 * terms)
        add += pl.num_repetitions * (a + 2 * terms) + 2
        stores += pl.num_repetitions * len(pl.program.relations)
        depth = len(pl.selector_path)
        if depth:
            mul += depth - 1 + 2
            add += sum(1 for b in pl.selector_path if not b)
    return mul, add, stores


def main():
    import numpy as np
    import torch
    from boojum_amd import gates as G
    from boojum_amd._lib import call
    from boojum_amd.field import P, stream_of
    log_n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    n_vars = int(sys.argv[2]) if len(sys.argv) > 2 else 130
    q = int(sys.argv[3]) if len(sys.argv) > 3 else 8
    if not torch.cuda.is_available():
        raise SystemExit("gates_bench needs a GPU")
    log_q = q.bit_length() - 1
    total = q << log_n
    placements = bench_set(G, n_vars)
    gate_set = G.GateSet(placements)
    need = gate_set.need
    n_consts = need["constants"]
    cols = torch.empty((n_vars + n_consts, q, 1 << log_n), dtype=torch.int64, device="cuda")
    call("bj_fill_synthetic_d", cols.data_ptr(), cols.shape[0], total, log_n + log_q, 7, 0, stream_of(cols))
    rng = np.random.default_rng(1)
    alphas = G.challenges_tensor([tuple(int(v) for v in pair) for pair in
                                  rng.integers(0, P, size=(need["alphas"], 2), dtype=np.uint64)], "cuda")
    dst = torch.zeros((2, total), dtype=torch.int64, device="cuda")
    variables, constants = cols[:n_vars], cols[n_vars:]

    def gate_terms():
        G.evaluate_gate_terms(gate_set, variables, None, constants, alphas, q, dst[0], dst[1])

    library_set = G.GateSet(placements, native_library=True)
    kinds = [library_set.image[library_set.image[2 + s] + 7] for s in range(library_set.num_segments)]

    def library_terms():
        G.evaluate_gate_terms(library_set, variables, None, constants, alphas, q, dst[0], dst[1])

    rounds = [(timed(torch, gate_terms, 10), timed(torch, library_terms, 10)) for _ in range(3)]
    t = rounds[0][0]
    t_int, t_lib = (sorted(r[i] for r in rounds)[1] for i in range(2))
    nbytes = (n_vars + n_consts + 4) * total * 8
    words = nbytes // 16
    src1 = cols.reshape(-1)
    dst1 = torch.empty((words,), dtype=torch.int64, device="cuda")
    t_copy = timed(torch, lambda: dst1.copy_(src1[:words]), 10)
    copy_gbs = 2 * words * 8 / t_copy / 1e9
    mul, add, stores = operation_counts(placements)
    slots = mul * MUL_SLOTS + add * ADD_SLOTS
    floor = total * slots / VALU_PEAK_SLOTS
    gbs = nbytes / t / 1e9
    instructions = sum(pl.num_repetitions * len(pl.program.relations) for pl in placements)
    line = {
        "shape": "%d variable + %d constant columns x 2^%d rows, quotient degree %d (2^%d points)"
                 % (n_vars, n_consts, log_n, q, log_n + log_q),
        "device": torch.cuda.get_device_name(0),
        "gates": [{"name": pl.program.evaluator.name, "repetitions": pl.num_repetitions,
                   "relations": len(pl.program.relations), "terms": pl.program.num_quotient_terms}
                  for pl in placements],
        "launches": gate_set.num_segments, "challenges": need["alphas"],
        "gate_terms": {
            "ms": t * 1e3, "alg_bytes_per_call": nbytes, "achieved": gbs, "unit": "GB/s", "peak": HBM_PEAK_GBS,
            "frac_of_hbm_peak": gbs / HBM_PEAK_GBS,
            "copy": {"bytes_copied": words * 8, "ms": t_copy * 1e3, "read_plus_write_gbs": copy_gbs},
            "vs_copy": gbs / copy_gbs,
            "per_point": {"products": mul, "additions": add, "interpreted_instructions": instructions,
                          "lds_bytes_written": 8 * stores, "column_words_loaded_incl_rereads":
                          sum(pl.num_repetitions * sum(1 for _, r in pl.program.relations for o in r.operands
                                                       if o.kind.endswith("Poly")) for pl in placements)},
            "slot_floor": {"slots_per_product": MUL_SLOTS, "slots_per_addition": ADD_SLOTS, "slots_per_point": slots,
                           "ms": floor * 1e3, "frac_of_slot_floor": floor / t},
        },
        "library": {
            "ms": t_lib * 1e3, "interpreted_ms": t_int * 1e3, "vs_interpreted": t_lib / t_int,
            "rounds_ms": {"interpreted": [r[0] * 1e3 for r in rounds], "library": [r[1] * 1e3 for r in rounds]},
            "launches": library_set.num_segments, "segment_kinds": kinds,
            "achieved": nbytes / t_lib / 1e9, "unit": "GB/s", "vs_copy": nbytes / t_lib / 1e9 / copy_gbs,
            "frac_of_slot_floor": floor / t_lib,
        },
    }
    print(json.dumps(line))


if __name__ == "__main__":
    main()
