#!/usr/bin/env python3
"""A whole `prover.prove` at the reference proof's shape: n = 2^20 (or 2^log_n), 130 columns under
the copy permutation, quotient degree 8, FRI LDE factor 2, cap 32, the geometry of
tools/openings_bench.py (leaf widths 156 / 58 / 16 / 167).

The circuit is synthetic and satisfiable, built with array arithmetic so that 2^20 rows take
seconds on the host: FmaGateInBaseFieldWithoutConstant x 24 on every row over 96 general-purpose
columns (small operands, so c0 a b + c1 c needs no reduction), the a of every repetition a copy of
the first one's (23 copy constraints per row), one unused column, a width-3 lookup over specialized
columns with 11 repetitions and the table id as a constant, 25 witness columns of placeholders.
The Poseidon2 flattened gate, the natural load, needs a witness generator that this tool does not
have; FMA is a library gate, so the native_library comparison applies.

One JSON line: the wall time of `prove` after a warm-up (median and spread over --rounds), the
split by stage, the time inside the transcript's round functions (counted by wrapping
`_round_function`) and their number, and the same proof with native_library=True, alternated
with the default round by round.

usage: python tools/prove_bench.py [log_n] [--rounds R]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "era-boojum_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from boojum_amd import gates as G, openings, prover, stage2, transcript, witness as W  # noqa: E402

LAYOUT = openings.OpeningLayout(V=130, W=25, C=33, M=1, L=11, I=16, lookup_setups=4, quotient_degree=8)
GENERAL = dict(num_columns_under_copy_permutation=97, num_witness_columns=25, num_constant_columns=2,
               max_allowed_constraint_degree=8)
LOOKUP = stage2.LookupParameters("constant", 3, 11)
FMA_REPS, TABLE_ID = 24, 5
LDE_FACTOR, CAP, SECURITY = 2, 32, 100
PUBLIC_INPUTS = [(0, 0), (1, 0), (2, 1), (3, 5)]


class TimedTranscript(transcript.Poseidon2Transcript):
    def __init__(self):
        super().__init__()
        self.seconds, self.rounds = 0.0, 0

    def _round_function(self):
        t0 = time.perf_counter()
        super()._round_function()
        self.seconds += time.perf_counter() - t0
        self.rounds += 1


def circuit(log_n, seed=5):
    n = 1 << log_n
    rng = np.random.default_rng(seed)
    g = LAYOUT
    constants = rng.integers(0, G.P, size=(g.C, n), dtype=np.uint64)
    constants[0] = rng.integers(1, 3, size=n)
    constants[1] = rng.integers(1, 4, size=n)
    constants[2] = TABLE_ID
    tables = rng.integers(0, G.P, size=(4, n), dtype=np.uint64)
    tables[3] = TABLE_ID
    var = np.zeros((g.V, n), dtype=np.uint64)
    maps = (np.arange(g.V, dtype=np.uint64)[:, None] << np.uint64(log_n)) + np.arange(n, dtype=np.uint64)[None, :]
    for k in range(FMA_REPS):
        a = var[0] if k else rng.integers(0, 1 << 30, size=n, dtype=np.uint64)
        b = rng.integers(0, 1 << 30, size=n, dtype=np.uint64)
        c = rng.integers(0, 1 << 61, size=n, dtype=np.uint64)
        var[4 * k:4 * k + 4] = [a, b, c, constants[0] * a * b + constants[1] * c]
        maps[4 * k] = maps[0]
    maps[4 * FMA_REPS] = W.placeholder()
    picks = rng.integers(0, n, size=(g.L, n))
    for s in range(g.L):
        var[97 + 3 * s:100 + 3 * s] = tables[:3, picks[s]]
    mult = np.bincount(picks.reshape(-1), minlength=n).astype(np.uint32)
    wit_maps = np.full((g.W, n), W.placeholder(), dtype=np.uint64)
    vec = W.WitnessVec(PUBLIC_INPUTS, var.reshape(-1), mult)
    placements = [G.GatePlacement(G.capture(G.FmaGateInBaseFieldWithoutConstant()), FMA_REPS)]
    return placements, constants, tables, maps, wit_maps, vec


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 2), "min_ms": round(min(ms), 2), "max_ms": round(max(ms), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("log_n", nargs="?", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    t0 = time.perf_counter()
    placements, constants, tables, maps, wit_maps, vec = circuit(args.log_n)
    t_circuit = time.perf_counter() - t0
    config = prover.ProofConfig(LDE_FACTOR, CAP, SECURITY)
    t0 = time.perf_counter()
    setup = prover.prepare_setup(constants, maps, wit_maps, placements, tables, LOOKUP, PUBLIC_INPUTS, LAYOUT, config,
                                 G.CSGeometry(**GENERAL))
    torch.cuda.synchronize()
    t_setup = time.perf_counter() - t0
    del maps, wit_maps, constants, tables
    library = prover.ProverSetup(**dict(setup.__dict__, gate_set=G.GateSet(placements, native_library=True)))
    kinds = [library.gate_set.image[library.gate_set.image[2 + s] + 7] for s in range(library.gate_set.num_segments)]
    # the values on the device, read in place, as a resident prover would hold them
    vec.all_values = torch.from_numpy(vec.all_values.view(np.int64)).cuda()
    setups = {"default": setup, "native_library": library}
    jsons = {}
    for name, s in setups.items():                                              # warm-up: tables, pools, kernels
        jsons[name] = prover.prove(s, vec).to_json()
    walls = {k: [] for k in setups}
    stages = {k: [] for k in setups}
    tr_s, tr_rounds = [], 0
    for _ in range(args.rounds):
        for name, s in setups.items():
            tr = TimedTranscript()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            proof = prover.prove(s, vec, transcript=tr)
            torch.cuda.synchronize()
            walls[name].append((time.perf_counter() - t0) * 1e3)
            stages[name].append(proof.timings)
            if name == "default":
                tr_s.append(tr.seconds * 1e3)
                tr_rounds = tr.rounds
    res = {"bench": "prove", "log_n": args.log_n, "layout": LAYOUT._asdict(), "fri_lde_factor": LDE_FACTOR, "cap": CAP,
           "security_level": SECURITY,
           "circuit": "fma_gate_in_base_without_constant x %d + lookup 3 x %d" % (FMA_REPS, LAYOUT.L),
           "uses_library_gates": G.KIND_LIBRARY in kinds, "rounds": args.rounds,
           "host_circuit_s": round(t_circuit, 2), "prepare_setup_s": round(t_setup, 2),
           "queries": proof.openings.num_queries, "schedule": proof.openings.schedule,
           "same_proof_both_routes": jsons["default"] == jsons["native_library"],
           "transcript": dict(summary(tr_s), round_functions=tr_rounds)}
    for name in setups:
        res[name] = dict(summary(walls[name]),
                         stages_median_ms={k: round(statistics.median(t[k] for t in stages[name]) * 1e3, 2)
                                           for k in stages[name][0]})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
