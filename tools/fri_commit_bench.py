#!/usr/bin/env python3
"""The FRI commit phase (do_fri, cs/implementations/fri/mod.rs:49-357) as one call against the
route a caller had to wire by hand before fri.do_fri existed, and the fused fold against the chain
of by-2 folds.  Device-event times, the routes alternated within one run; one JSON line.

(a) `do_fri`: fri.do_fri with a fixed-challenge stub transcript (caps still come to the host).
(b) `by2_route`: the same order and the same stub, but every reduction step as a chain of by-2
    folds (fri.interpolate), i.e. one launch and one round trip through memory per fold, with
    construct_by_chunking* per step and the same final interpolation.
(c) `fold8`: at 2^24 Ext2 elements, one fri.fold_by(..., 3) against three fri.fold calls and
    against a device-to-device copy that moves the fused fold's bytes (2 N values and 7 N / 8 roots
    in, N / 4 values out, N = 2^24; a copy of B bytes moves 2 B).

The defaults are the reference proof's shape (tests/golden/proof_fri.json): n = 2^20, LDE 2, cap 32,
schedule 3,3,3,3,3,1 (final degree 16).  The results of (a) and (b) are compared before timing.

usage: python tools/fri_commit_bench.py [log_n=20] [log_lde=1] [schedule=3,3,3,3,3,1]
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "era-boojum_amd"))

CAP = 32
P = 0xFFFFFFFF00000001


class StubTranscript:
    """Fixed challenges; what is witnessed is dropped."""

    def __init__(self):
        self.drawn = 0

    def witness_merkle_tree_cap(self, cap):
        pass

    def witness_field_elements(self, els):
        pass

    def get_challenge(self):
        self.drawn += 1
        return (0x9E3779B97F4A7C15 * self.drawn) % P


def by2_route(torch, fri, merkle, field, rows, schedule, lde_degree, hasher="poseidon2"):
    """do_fri's order with every reduction step as by-2 folds (what the package offered before)."""
    tr = StubTranscript()
    MT = merkle.MerkleTreeWithCap
    roots = fri.precompute_roots(rows.shape[1], device=rows.device)
    ci = pow(7, P - 2, P)
    cur, sources = rows, []
    for k, s in enumerate(schedule):
        build = MT.construct_by_chunking_from_flat_sources if k else MT.construct_by_chunking
        tree = build(cur, 1 << s, CAP, hasher=hasher)
        tr.witness_merkle_tree_cap(tree.get_cap())
        ch = (tr.get_challenge(), tr.get_challenge())
        c0, c1, ci = fri.interpolate(cur[0], cur[1], fri.challenge_powers(ch, s), roots, ci)
        cur = torch.stack([c0, c1])          # the flat sources of the next tree
        sources.append((c0, c1))
    m0, m1, low = fri.final_monomials(cur[0], cur[1], ci, lde_degree)
    return sources, field.to_host(m0), field.to_host(m1), low


def event_ms(torch, fn):
    st = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    fn()
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(torch, fns, rounds):
    """{name: [ms per round]}: every round runs each function once, in order."""
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(event_ms(torch, fn))
    return out


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "rounds": len(ms)}


def main():
    import numpy as np
    import torch
    from boojum_amd import field, fri, merkle
    from boojum_amd._lib import call
    from boojum_amd.field import stream_of
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    log_n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    log_lde = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    schedule = [int(s) for s in (sys.argv[3] if len(sys.argv) > 3 else "3,3,3,3,3,1").split(",")]
    full = 1 << (log_n + log_lde)
    rows = torch.empty((2, full), dtype=torch.int64, device="cuda")
    call("bj_fill_synthetic_d", rows.data_ptr(), 2, full, log_n + log_lde, 7, 0, stream_of(rows))

    def run_do_fri():
        return fri.do_fri(rows[0], rows[1], StubTranscript(), schedule, 1 << log_lde, CAP)

    def run_by2():
        return by2_route(torch, fri, merkle, field, rows, schedule, 1 << log_lde)

    # same results (also the warm-up of every kernel and shape)
    a, (b_src, b_m0, b_m1, b_low) = run_do_fri(), run_by2()
    same = all(torch.equal(x0, y0) and torch.equal(x1, y1)
               for (x0, x1), (y0, y1) in zip(a.leaf_sources_for_intermediate_oracles, b_src))
    same = same and np.array_equal(a.monomial_forms[0], b_m0) and np.array_equal(a.monomial_forms[1], b_m1)
    same = bool(same and a.low_degree == b_low)
    phase = alternate(torch, {"do_fri": run_do_fri, "by2_route": run_by2}, 15)

    # (c) the fold alone at 2^24 Ext2 elements
    log_f = 24
    nf = 1 << log_f
    src = torch.empty((2, nf), dtype=torch.int64, device="cuda")
    call("bj_fill_synthetic_d", src.data_ptr(), 2, nf, log_f, 11, 0, stream_of(src))
    roots = fri.precompute_roots(nf)
    ci, ch = pow(7, P - 2, P), (123456789, 987654321)
    out = torch.empty((2, nf >> 3), dtype=torch.int64, device="cuda")
    fused_bytes = 8 * (2 * nf + (7 * nf) // 8 + 2 * (nf >> 3))
    chain_bytes = 8 * sum(2 * (nf >> s) + (nf >> (s + 1)) + 2 * (nf >> (s + 1)) for s in range(3))
    cp_src = torch.empty((fused_bytes // 16,), dtype=torch.int64, device="cuda")
    cp_dst = torch.empty_like(cp_src)
    reps = 10

    def fused():
        for _ in range(reps):
            fri.fold_by(src[0], src[1], roots, ci, ch, 3, out=(out[0], out[1]))

    def chain():
        for _ in range(reps):
            fri.interpolate(src[0], src[1], fri.challenge_powers(ch, 3), roots, ci)

    def copy():
        for _ in range(reps):
            cp_dst.copy_(cp_src)

    c0, c1, _ = fri.interpolate(src[0], src[1], fri.challenge_powers(ch, 3), roots, ci)
    fused()
    copy()
    same_fold = bool(torch.equal(out[0], c0) and torch.equal(out[1], c1))
    fold = {k: [x / reps for x in v]
            for k, v in alternate(torch, {"fused": fused, "chain": chain, "copy": copy}, 10).items()}

    med = {k: statistics.median(v) for k, v in {**phase, **fold}.items()}
    line = {
        "shape": {"log_n": log_n, "log_lde": log_lde, "schedule": schedule, "cap": CAP, "hasher": "poseidon2"},
        "phase": {"do_fri": summary(phase["do_fri"]), "by2_route": summary(phase["by2_route"]),
                  "results_equal": same,
                  "by2_over_do_fri": med["by2_route"] / med["do_fri"],
                  "by2_route_spread": (max(phase["by2_route"]) - min(phase["by2_route"])) / med["by2_route"]},
        "fold8": {"ext2_elements": nf, "fused": summary(fold["fused"]), "chain": summary(fold["chain"]),
                  "copy": summary(fold["copy"]), "results_equal": same_fold,
                  "fused_alg_bytes": fused_bytes, "chain_alg_bytes": chain_bytes,
                  "fused_gbs": fused_bytes / med["fused"] / 1e6,
                  "chain_over_fused": med["chain"] / med["fused"],
                  "fused_over_copy": med["fused"] / med["copy"]},
    }
    print(json.dumps(line))


if __name__ == "__main__":
    main()
