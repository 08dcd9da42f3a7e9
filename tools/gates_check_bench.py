#!/usr/bin/env python3
"""Measurement of the gate satisfiability check (bj_gate_set_satisfied_d, csrc/gates.hip) on the set
and shape of tools/gates_bench.py: 2^20 rows, 130 variable columns, the eight evaluators of
boojum_amd.gates at their full repetition counts under a depth-3 selector tree.  The columns are
synthetic words, so every term of every row fails (the record counts rows * terms): every wave
issues its add and its min, the worst case for the atomics.  A mostly satisfied trace is not timed.

Three times from one run, each from HIP events on the stream the calls run on:
* check: the call for the whole trace (the initialisation, the check and the value launch);
* copy: torch's device-to-device copy of the same column bytes, (variables + constants) * n * 8;
* gate_terms_q1: bj_quotient_gate_terms_d over the same columns taken as an LDE of degree 1, the
  same program walk with the challenge products and the accumulator in place of the comparison.

usage: python tools/gates_check_bench.py [log_n=20] [n_vars=130]   (prints one JSON line)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "era-boojum_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    import numpy as np
    import torch
    from boojum_amd import gates as G
    from boojum_amd._lib import call
    from boojum_amd.field import P, stream_of, to_host
    from gates_bench import bench_set, timed
    log_n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    n_vars = int(sys.argv[2]) if len(sys.argv) > 2 else 130
    if not torch.cuda.is_available():
        raise SystemExit("gates_check_bench needs a GPU")
    n = 1 << log_n
    placements = bench_set(G, n_vars)
    gate_set = G.GateSet(placements)
    need = gate_set.need
    n_consts = need["constants"]
    cols = torch.empty((n_vars + n_consts, n), dtype=torch.int64, device="cuda")
    call("bj_fill_synthetic_d", cols.data_ptr(), cols.shape[0], n, log_n, 7, 0, stream_of(cols))
    variables, constants = cols[:n_vars], cols[n_vars:]
    status = torch.zeros((4,), dtype=torch.int64, device="cuda")

    def check():
        for segment in range(gate_set.num_segments):
            call("bj_gate_set_satisfied_d", gate_set._handle, segment | (G.CHECK_BEGIN if segment == 0 else 0),
                 variables.data_ptr(), n, n_vars, None, 0, 0, constants.data_ptr(), n, n_consts, 0, n,
                 status.data_ptr(), stream_of(cols))

    t_check = timed(torch, check, 10)
    record = [int(x) for x in to_host(status)]
    report = G.report_from_status(gate_set, record)

    nbytes = (n_vars + n_consts) * n * 8
    dst = torch.empty_like(cols)
    t_copy = timed(torch, lambda: dst.copy_(cols), 10)
    del dst

    rng = np.random.default_rng(1)
    alphas = G.challenges_tensor([tuple(int(v) for v in pair) for pair in
                                  rng.integers(0, P, size=(need["alphas"], 2), dtype=np.uint64)], "cuda")
    acc = torch.zeros((2, n), dtype=torch.int64, device="cuda")
    v3, c3 = variables.unsqueeze(1), constants.unsqueeze(1)
    t_terms = timed(torch, lambda: G.evaluate_gate_terms(gate_set, v3, None, c3, alphas, 1, acc[0], acc[1]), 10)

    line = {
        "shape": "%d variable + %d constant columns x 2^%d rows" % (n_vars, n_consts, log_n),
        "device": torch.cuda.get_device_name(0),
        "gates": [{"name": pl.program.evaluator.name, "repetitions": pl.num_repetitions,
                   "terms": pl.program.num_quotient_terms} for pl in placements],
        "launches": gate_set.num_segments, "terms_per_row": need["alphas"],
        "check": {"ms": t_check * 1e3, "column_bytes": nbytes, "column_gbs": nbytes / t_check / 1e9,
                  "status": record, "num_unsatisfied": report.num_unsatisfied, "first": report.message()},
        "copy": {"bytes_copied": nbytes, "ms": t_copy * 1e3, "read_plus_write_gbs": 2 * nbytes / t_copy / 1e9},
        "gate_terms_q1": {"ms": t_terms * 1e3},
        "check_over_copy": t_check / t_copy, "check_over_gate_terms_q1": t_check / t_terms,
    }
    print(json.dumps(line))


if __name__ == "__main__":
    main()
