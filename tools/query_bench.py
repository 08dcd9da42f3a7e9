#!/usr/bin/env python3
"""Measurement of the query phase (prover.rs:2161-2266) at the reference proof's shape: n = 2^20,
LDE 2, cap 32, the four base oracles of 156 / 58 / 16 / 167 columns and the six FRI oracles of the
schedule [3, 3, 3, 3, 3, 1]: 10 oracles and 99 path digests per query.  Inputs are synthetic
(bj_fill_synthetic_d; the FRI oracles over a synthetic codeword folded with fri.interpolate).

Two routes over the same trees in the same run, alternated, the median of the repeats reported,
for Q = 100 queries and for Q = 1, each from the call to the data on the host:
* batched: queries.construct_queries, one bj_oracle_queries_d launch and one device-to-host copy;
* per_query: what the project offered before, for every query and oracle
  MerkleTreeWithCap.get_proof (depth + 1 copies of 32 bytes) and a strided gather of the leaf's
  row copied to the host.
"device_ms" is the batched launch alone, from HIP events on its stream.

usage: python tools/query_bench.py [repeats=7]   (prints one JSON line)
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "era-boojum_amd"))

LOG_N, LOG_LDE, CAP = 20, 1, 32
BASE_COLUMNS = (156, 58, 16, 167)   # witness, stage 2, quotient, setup
SCHEDULE = (3, 3, 3, 3, 3, 1)
QUERY_COUNTS = (100, 1)


def build_oracles(torch):
    from boojum_amd import fri, queries
    from boojum_amd._lib import call
    from boojum_amd.field import stream_of
    from boojum_amd.merkle import MerkleTreeWithCap as Tree
    n, log_full = 1 << LOG_N, LOG_N + LOG_LDE
    full = 1 << log_full

    def synthetic(cols, seed):
        t = torch.empty((cols, full), dtype=torch.int64, device="cuda")
        call("bj_fill_synthetic_d", t.data_ptr(), cols, full, log_full, seed, 0, stream_of(t))
        return t

    oracles = []
    for i, c in enumerate(BASE_COLUMNS):
        src = synthetic(c, 11 + i)
        oracles.append(queries.QueryOracle(Tree.construct(src, CAP), src))
    code = synthetic(2, 99)
    roots = fri.precompute_roots(full)
    ci = None
    for k, (s, (e, shift, n_leaves)) in enumerate(zip(SCHEDULE, queries.fri_plan(LOG_N, LOG_LDE, SCHEDULE))):
        if k == 0:
            tree = Tree.construct_by_chunking(code.reshape(2, 1 << LOG_LDE, n), e, CAP)
        else:
            tree = Tree.construct_by_chunking_from_flat_sources(code, e, CAP)
        assert tree.n_leaves == n_leaves
        oracles.append(queries.QueryOracle(tree, code, e, shift))
        c0, c1, ci = fri.interpolate(code[0], code[1], fri.challenge_powers((1234 + k, 5678), s), roots, ci)
        code = torch.stack([c0, c1])
    torch.cuda.synchronize()
    return oracles


def per_query_route(oracles, indices):
    """One query at a time: get_proof and a row gather per oracle."""
    from boojum_amd.field import to_host
    out = []
    for index in indices:
        for o in oracles:
            t, e = index >> o.index_shift, o.elements_per_leaf
            leaf, path = o.tree.get_proof(t)
            out.append((to_host(o.sources[:, t * e: (t + 1) * e]).reshape(-1), leaf, path))
    return out


def main():
    import numpy as np
    import torch
    from boojum_amd import queries
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    if repeats < 5:
        raise SystemExit("at least 5 repeats")
    if not torch.cuda.is_available():
        raise SystemExit("query_bench needs a GPU")
    oracles = build_oracles(torch)
    full = 1 << (LOG_N + LOG_LDE)
    words = sum(o.words for o in oracles)
    line = {"shape": "n 2^%d, LDE %d, cap %d, columns %s, FRI schedule %s" % (
                LOG_N, 1 << LOG_LDE, CAP, "/".join(map(str, BASE_COLUMNS)), list(SCHEDULE)),
            "device": torch.cuda.get_device_name(0), "oracles": len(oracles),
            "path_digests_per_query": sum(o.depth for o in oracles), "words_per_query": words, "repeats": repeats}
    for nq in QUERY_COUNTS:
        indices = [int(v) for v in np.random.default_rng(nq).integers(0, full, size=nq)]
        # both routes once untimed: kernels loaded, and the two must agree before either is timed
        got, want = queries.construct_queries(oracles, indices), per_query_route(oracles, indices)
        for q in range(nq):
            for k, r in enumerate(got):
                el, leaf, path = want[q * len(oracles) + k]
                assert np.array_equal(r.leaf_elements[q], el) and np.array_equal(r.leaf_hash[q], leaf)
                assert np.array_equal(r.proof[q], path)
        batched, single = [], []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            queries.construct_queries(oracles, indices)
            t1 = time.perf_counter()
            per_query_route(oracles, indices)
            t2 = time.perf_counter()
            batched.append(t1 - t0)
            single.append(t2 - t1)
        # the launch alone, on preallocated buffers
        idx = torch.tensor(indices, dtype=torch.int64, device="cuda")
        out = torch.empty((nq * words,), dtype=torch.int64, device="cuda")
        status = torch.empty((4,), dtype=torch.int64, device="cuda")
        st = torch.cuda.current_stream()
        device = []
        for _ in range(repeats + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            queries.launch_queries(oracles, idx, out, status)
            e1.record(st)
            torch.cuda.synchronize()
            device.append(e0.elapsed_time(e1))
        b, s = statistics.median(batched), statistics.median(single)
        line["q%d" % nq] = {"queries": nq, "payload_bytes": nq * words * 8,
                            "batched_ms": b * 1e3, "batched_min_ms": min(batched) * 1e3,
                            "per_query_ms": s * 1e3, "per_query_min_ms": min(single) * 1e3,
                            "device_ms": statistics.median(device[2:]), "per_query_over_batched": s / b}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
