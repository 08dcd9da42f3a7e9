#!/usr/bin/env python3
"""Measurement of the query phase on sharded trees at the reference proof's shape: k n = 2^21
leaves, cap 32, the four base oracles of 156 / 58 / 16 / 167 columns, G = 8 ranks.

The ranks are threads on ONE card over the in-process group (sharded.LocalGroup), whose exchanges
are device-to-device copies ordered through a host barrier: a rehearsal transport, not for
performance.  The figures therefore show the calls, copies and synchronisations the batched call
saves, not link time; nothing here measures xGMI.  The column counts are no multiples of 8, so the
shards are not made by bj_sharded_commit_d: one full tree per oracle is built over synthetic
columns (bj_fill_synthetic_d) and every rank's rows, leaves and subtree levels are cut out of it
(local level l is the P-th slice of global level l, as the commit leaves them).

Two routes over the same shards in the same run, alternated, each from the call to the data on the
host of every rank (the slowest rank counts), the median of the repeats reported, for Q = 100 and
Q = 1:
* batched: sharded.native_sharded_queries, one bj_sharded_queries_d call and one copy per rank;
* per_index: sharded.native_sharded_query (bj_sharded_query_h) for every index and oracle.

usage: python tools/sharded_query_bench.py [repeats=5]   (prints one JSON line)
"""
import json
import os
import statistics
import sys
import threading
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "era-boojum_amd"))

LOG_NL, CAP, WORLD = 21, 32, 8
BASE_COLUMNS = (156, 58, 16, 167)   # witness, stage 2, quotient, setup
QUERY_COUNTS = (100, 1)


def build_shards(torch):
    """Per rank, per oracle: (res with lde (1, C, m), leaves (m, 4), nodes (m - cap_local, 4)), C)."""
    from boojum_amd._lib import call
    from boojum_amd.field import stream_of
    from boojum_amd.merkle import MerkleTreeWithCap as Tree
    nl, m, cap_local = 1 << LOG_NL, (1 << LOG_NL) // WORLD, max(1, CAP // WORLD)
    shards = [[] for _ in range(WORLD)]
    for i, c in enumerate(BASE_COLUMNS):
        src = torch.empty((c, nl), dtype=torch.int64, device="cuda")
        call("bj_fill_synthetic_d", src.data_ptr(), c, nl, LOG_NL, 11 + i, 0, stream_of(src))
        tree = Tree.construct(src, CAP)
        for r in range(WORLD):
            levels, lvl = [], 1
            while (m >> lvl) >= cap_local:
                start, cnt = nl - (nl >> (lvl - 1)), m >> lvl
                levels.append(tree.nodes[start + r * cnt: start + (r + 1) * cnt])
                lvl += 1
            res = types.SimpleNamespace(lde=src[:, r * m: (r + 1) * m].contiguous().unsqueeze(0),
                                        leaves=tree.leaf_hashes[r * m: (r + 1) * m].contiguous(),
                                        nodes=torch.cat(levels))
            shards[r].append((res, c))
        del src, tree
    torch.cuda.synchronize()
    return shards


def main():
    import numpy as np
    import torch
    from boojum_amd import sharded
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    if repeats < 5:
        raise SystemExit("at least 5 repeats")
    if not torch.cuda.is_available():
        raise SystemExit("sharded_query_bench needs a GPU")
    shards = build_shards(torch)
    nl = 1 << LOG_NL
    index_sets = {nq: [int(v) for v in np.random.default_rng(nq).integers(0, nl, size=nq)] for nq in QUERY_COUNTS}
    group = sharded.LocalGroup(WORLD)
    gate = threading.Barrier(WORLD)
    times = {nq: [[None] * WORLD for _ in range(repeats)] for nq in QUERY_COUNTS}
    errors = []

    def per_index(comm, mine, indices):
        return [[sharded.native_sharded_query(comm, res, c, LOG_NL, 0, CAP, i) for res, c in mine] for i in indices]

    def rank_main(r):
        try:
            torch.cuda.set_device(0)
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                comm = group.comm(r)
                mine = shards[r]
                oracles = [sharded.ShardedQueryOracle(res, c, LOG_NL, 0, CAP) for res, c in mine]
                for nq in QUERY_COUNTS:
                    indices = index_sets[nq]
                    # both routes once untimed: kernels loaded, and they must agree before either is timed
                    got, want = sharded.native_sharded_queries(comm, oracles, indices), per_index(comm, mine, indices)
                    for q in range(nq):
                        for o, g in enumerate(got):
                            el, leaf, path = want[q][o]
                            assert np.array_equal(g.leaf_elements[q], el) and np.array_equal(g.leaf_hash[q], leaf)
                            assert np.array_equal(g.proof[q], path)
                    for k in range(repeats):
                        s.synchronize()
                        gate.wait(timeout=120)
                        t0 = time.perf_counter()
                        sharded.native_sharded_queries(comm, oracles, indices)
                        t1 = time.perf_counter()
                        gate.wait(timeout=120)
                        t2 = time.perf_counter()
                        per_index(comm, mine, indices)
                        t3 = time.perf_counter()
                        times[nq][k][r] = (t1 - t0, t3 - t2)
                comm.close()
        except Exception as e:  # noqa: BLE001 - reported below
            errors.append((r, repr(e)))
            gate.abort()

    threads = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(WORLD)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=500)
    if any(t.is_alive() for t in threads) or errors:
        raise SystemExit("a rank failed or did not finish: %s" % errors)
    group.close()
    words = sum(c + 4 + 4 * (LOG_NL - 5) for c in BASE_COLUMNS)
    line = {"shape": "k n = 2^%d leaves, cap %d, columns %s, G = %d ranks as threads on one card" % (
                LOG_NL, CAP, "/".join(map(str, BASE_COLUMNS)), WORLD),
            "transport": "in-process local group (device-to-device copies behind a host barrier; not for performance)",
            "device": torch.cuda.get_device_name(0), "oracles": len(BASE_COLUMNS), "words_per_query": words,
            "repeats": repeats}
    for nq in QUERY_COUNTS:
        batched = [max(t[0] for t in rep) for rep in times[nq]]
        single = [max(t[1] for t in rep) for rep in times[nq]]
        b, s = statistics.median(batched), statistics.median(single)
        line["q%d" % nq] = {"queries": nq, "payload_bytes": nq * words * 8,
                            "gathered_bytes_per_rank": WORLD * nq * words * 8,
                            "per_index_calls": nq * len(BASE_COLUMNS),
                            "batched_ms": b * 1e3, "batched_min_ms": min(batched) * 1e3,
                            "per_index_ms": s * 1e3, "per_index_min_ms": min(single) * 1e3,
                            "per_index_over_batched": s / b}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
