#!/usr/bin/env python3
"""The opening phase at the reference proof's shape: n = 2^20 (or 2^log_n), FRI LDE factor 2, leaf
widths 156 / 58 / 16 / 167 (witness / stage 2 / quotient / setup), six opening points (z, z * omega,
0 and three public-input rows), synthetic columns.

Three ways over the same codeword, alternated round by round in one run and timed with HIP events
(medians, with the spread): the fused call (bj_deep_codeword_d, one launch), the chain of one
bj_deep_quotient_d per (oracle, point) over the column range its sources touch (nine launches),
and a device-to-device copy of the bytes the fused call reads and writes.  Descriptors and
coefficients are built and uploaded before the clock starts, for both routes.  Then, once, the wall
time of openings.prove_openings with its split by step, on either route.

usage: python tools/openings_bench.py [log_n] [--rounds R]
Prints one JSON line.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "era-boojum_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from boojum_amd import commit, deep, field, openings, pow as pow_, transcript  # noqa: E402
from boojum_amd._lib import call  # noqa: E402

# a geometry with the reference proof's leaf widths: V + W + M = 156, 2 (1 + I + L + M) = 58,
# 2 * 8 = 16, V + C + 4 = 167, I = ceil(V / 8) - 1
LAYOUT = openings.OpeningLayout(V=130, W=25, C=33, M=1, L=11, I=16, lookup_setups=4, quotient_degree=8)
LDE_FACTOR, CAP, SECURITY = 2, 16, 100
PUBLIC_INPUTS = [(0, 0), (1, 0), (2, 1), (3, 5)]


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("log_n", nargs="?", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=15)
    args = ap.parse_args()
    log_n, n = args.log_n, 1 << args.log_n
    assert openings.leaf_widths(LAYOUT) == (156, 58, 16, 167)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    widths = openings.leaf_widths(LAYOUT)
    oracles = []
    for i, w in enumerate(widths):
        tr = commit.synthetic_trace(w, log_n, seed=42 + i, device=dev)
        if i == openings.QUOTIENT:
            oracles.append(commit.quotient_commit(tr, LDE_FACTOR, CAP))
        else:
            oracles.append(commit.commit_trace_columns(tr, LDE_FACTOR, LDE_FACTOR, CAP))
        del tr
    torch.cuda.synchronize()
    rows, log_domain = LDE_FACTOR * n, log_n + 1
    groups = [o.lde.reshape(o.lde.shape[0], -1)[:, :rows] for o in oracles]

    # ---- the three kernels' arguments, off the clock
    rng = np.random.default_rng(1)
    ext = lambda: (int(rng.integers(0, field.P, dtype=np.uint64)), int(rng.integers(0, field.P, dtype=np.uint64)))  # noqa: E731
    z, omega = ext(), openings.domain_generator(log_n)
    n_z, n_0 = len(openings.sources_at_z(LAYOUT)), len(openings.sources_at_0(LAYOUT))
    pis = [(c, r, 7 + c) for c, r in PUBLIC_INPUTS]
    pi_tuples = openings.public_input_opening_tuples(pis, log_n)
    total = n_z + 1 + n_0 + len(pis)
    points = openings.opening_points(LAYOUT, z, omega, [ext() for _ in range(n_z)], [ext()], [ext() for _ in range(n_0)],
                                     pi_tuples, deep.materialize_ext_challenge_powers(ext(), total))
    assert len(points) == 6
    terms, gammas, ks = deep.codeword_terms(list(widths), points)
    g_d = field.to_device(np.array(gammas, dtype=np.uint64).reshape(-1), dev)
    out = torch.empty((2, rows), dtype=torch.int64, device=dev)
    st = field.stream_of(out)
    desc = deep.codeword_descriptor([(t.data_ptr(), t.shape[0], t.stride(0)) for t in groups], points, terms, ks,
                                    g_d.data_ptr(), len(gammas), log_domain, 0, rows, out[0].data_ptr(),
                                    out[1].data_ptr(), False)
    chain_out = torch.empty_like(out)
    chain_calls = []
    for k, (g, first, count, p, off) in enumerate(terms):
        # one call per term; the point's constant goes with its first term
        first_of_point = k == 0 or terms[k - 1][3] != p
        kk = ks[p] if first_of_point else (0, 0)
        at = points[p][0]
        chain_calls.append((groups[g][first].data_ptr(), count, groups[g].stride(0), g_d.data_ptr() + 16 * off, kk[0], kk[1],
                            at[0] % field.P, at[1] % field.P, log_domain, 0, rows, chain_out[0].data_ptr(),
                            chain_out[1].data_ptr(), 1 if k else 0, st))
    read_cols = sum(t[2] for t in terms)
    copy_words = (read_cols + 2) * rows // 2          # a copy reads and writes each word: half the words
    src = torch.empty((copy_words,), dtype=torch.int64, device=dev)
    dst = torch.empty_like(src)

    def fused():
        call("bj_deep_codeword_d", ctypes.byref(desc), st)

    def chain():
        for a in chain_calls:
            call("bj_deep_quotient_d", *a)

    def copy():
        dst.copy_(src)

    runs = {"fused": fused, "chain": chain, "copy": copy}
    for f in runs.values():
        f()
    torch.cuda.synchronize()
    same = bool(torch.equal(out, chain_out))
    ms = {k: [] for k in runs}
    for _ in range(args.rounds):
        for name, f in runs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b))
    moved = (read_cols + 2) * rows * 8
    res = {"bench": "openings", "log_n": log_n, "fri_lde_factor": LDE_FACTOR, "leaf_widths": list(widths),
           "points": len(points), "terms": len(terms), "chain_launches": len(chain_calls), "rounds": args.rounds,
           "fused_equals_chain": same, "fused_bytes": moved, "copy_bytes_moved": copy_words * 16}
    for name in runs:
        res[name] = summary(ms[name])
    res["fused"]["tb_s"] = round(moved / res["fused"]["median_ms"] / 1e9, 3)
    res["copy"]["tb_s"] = round(copy_words * 16 / res["copy"]["median_ms"] / 1e9, 3)
    res["chain_over_fused"] = round(res["chain"]["median_ms"] / res["fused"]["median_ms"], 3)
    del src, dst, chain_out, out

    # ---- prove_openings once per route
    def seeded():
        tr = transcript.Poseidon2Transcript()
        for o in (oracles[openings.SETUP], oracles[openings.WITNESS], oracles[openings.STAGE_2], oracles[openings.QUOTIENT]):
            tr.witness_merkle_tree_cap(o.get_cap())
        return tr

    # the public-input values are synthetic: the prover does not check them (the verifier would)
    cfg = openings.OpeningConfig(SECURITY, 0, pow_.NoPow, CAP, LDE_FACTOR)
    openings.prove_openings(oracles, LAYOUT, seeded(), cfg, pis)      # warm-up: tables, pools
    for route in ("fused", "chain"):
        t0 = time.perf_counter()
        proof = openings.prove_openings(oracles, LAYOUT, seeded(), cfg, pis, route=route)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        res["prove_openings_" + route] = {"wall_ms": round(wall * 1e3, 2), "queries": proof.num_queries,
                                          "schedule": proof.schedule,
                                          "split_ms": {k: round(v * 1e3, 2) for k, v in proof.timings.items()}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
