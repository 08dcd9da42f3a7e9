"""bj_sharded_queries_d / sharded.native_sharded_queries on the GPU: every oracle and every index of
a batch on sharded trees in one collective call.

Ranks are threads on one card over the in-process group, as in test_gpu_native_sharded.py.  Every
expected value comes from code that is not under test: queries.construct_queries over a
MerkleTreeWithCap of the whole domain (pinned to get_proof and the oracle in test_gpu_queries.py).
The shards are cut out of that same full tree with the CPU model's shard_tree -- local level l is
the P-th slice of global level l, which is what bj_sharded_commit_d produces -- so the smallest
shapes do not depend on the commit's own size limits; one case goes through the commit itself."""
import threading
import types

import numpy as np
import pytest

import sharded_queries_model as M

P = 0xFFFFFFFF00000001
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bj():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import boojum_amd
    from boojum_amd import _lib, commit, field, merkle, queries, serialization, sharded
    lib = boojum_amd.load()
    return types.SimpleNamespace(torch=torch, field=field, Q=queries, S=sharded, lib=lib, _lib=_lib, commit=commit,
                                 ser=serialization, Tree=merkle.MerkleTreeWithCap, Error=boojum_amd.BoojumError)


def rand(shape, seed):
    return np.random.default_rng(seed).integers(0, P, size=shape, dtype=np.uint64)


class Full:
    """One oracle over the whole domain of nl leaves: the (C, nl) sources and their tree on the
    device, the unsharded QueryOracle, and rank r's ShardedQueryOracle of a G-way split."""

    def __init__(self, bj, n_cols, nl, cap, hasher="poseidon2", seed=0, path_only=False, contiguous=False):
        self.bj, self.nl, self.cap, self.hasher, self.contiguous = bj, nl, cap, hasher, contiguous
        self.flat = bj.field.to_device(rand((max(n_cols, 1), nl), 1000 * seed + n_cols))
        self.tree = bj.Tree.construct(self.flat, cap, hasher=hasher)
        self.n_cols = 0 if path_only else n_cols
        self.plain = bj.Q.QueryOracle(self.tree) if path_only else bj.Q.QueryOracle(self.tree, self.flat)

    def shard(self, G, r):
        m = self.nl // G
        leaves, nodes = M.shard_tree(self.tree.leaf_hashes, self.tree.nodes, self.cap, G, r)
        src = self.flat[:, r * m: (r + 1) * m]          # a view: the column stride is nl, > m when G > 1
        if self.contiguous:
            src = src.contiguous()
        res = types.SimpleNamespace(lde=src.unsqueeze(0), leaves=leaves.contiguous(), nodes=nodes.contiguous())
        o = self.bj.S.ShardedQueryOracle(res, self.n_cols, self.nl.bit_length() - 1, 0, self.cap, self.hasher,
                                         sources=self.n_cols > 0)
        assert o.col_stride == (0 if not self.n_cols else m if self.contiguous or G == 1 else self.nl)
        return o


def run_ranks(bj, G, rank_fn, timeout=60):
    """rank_fn(comm, r) on G threads over one in-process group; the per-rank results."""
    torch = bj.torch
    torch.cuda.synchronize()
    group = bj.S.LocalGroup(G)
    outs, errors = [None] * G, []

    def rank_main(r):
        try:
            torch.cuda.set_device(0)
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                comm = group.comm(r)
                try:
                    outs[r] = rank_fn(comm, r)
                    s.synchronize()
                finally:
                    comm.close()
        except Exception as e:  # noqa: BLE001 - reported below
            errors.append((r, repr(e)))

    threads = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(G)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=timeout)
    assert not any(t.is_alive() for t in threads), "a rank did not finish"
    group.close()
    assert not errors, errors
    return outs


def edge_indices(nl, G):
    m = nl // G
    return sorted({0, 1, m - 1, m % nl, nl // 2 - 1, nl // 2, nl - 1}) + [1, nl - 1]   # and two duplicates


def check_batch(bj, G, fulls, indices):
    """One call at world G; every rank's records equal the unsharded ones, part by part."""
    want = bj.Q.construct_queries([f.plain for f in fulls], indices)
    shards = [[f.shard(G, r) for f in fulls] for r in range(G)]
    for f, o in zip(fulls, shards[0]):
        assert bj.S.sharded_query_words(o) == o.words == f.plain.words
    got = run_ranks(bj, G, lambda comm, r: bj.S.native_sharded_queries(comm, shards[r], indices))
    for r in range(G):
        assert len(got[r]) == len(fulls)
        for o, (w, g) in enumerate(zip(want, got[r])):
            for name, part_w, part_g in zip(w._fields, w, g):
                assert part_w.shape == part_g.shape, (r, o, name)
                assert np.array_equal(part_w, part_g), "rank %d oracle %d %s" % (r, o, name)
    return want


@pytest.mark.parametrize("G,nl,n_cols,cap,hasher", [
    (1, 64, 9, 4, "poseidon2"),       # no exchange content, no top levels
    (2, 64, 9, 2, "blake2s"),         # cap = G
    (4, 64, 16, 16, "keccak256"),     # cap > G: cap_local 4
    (8, 64, 1, 4, "poseidon2"),       # cap < G: one top level, from the gathered roots alone
    (8, 64, 9, 1, "poseidon2"),       # cap < G: three top levels
    (8, 64, 9, 1, "blake2s"),
    (8, 64, 9, 2, "keccak256"),       # two top levels
    (8, 64, 33, 32, "poseidon2"),     # m = 8 = 2 cap_local: local depth 1
    (2, 64, 1, 32, "blake2s"),        # m = 32 = 2 cap_local
    (4, 1024, 33, 8, "poseidon2"),    # the largest domain: depth 7 of the subtree
    (2, 128, 600, 2, "poseidon2"),    # 624 words: four per lane in one pass
])
def test_one_oracle(bj, G, nl, n_cols, cap, hasher):
    f = Full(bj, n_cols, nl, cap, hasher, seed=G)
    check_batch(bj, G, [f], edge_indices(nl, G))


def test_contiguous_shard_and_path_only(bj):
    """col_stride = m (what bj_sharded_commit_d's block 0 has) and an oracle without sources."""
    G, nl = 4, 128
    fulls = [Full(bj, 9, nl, 8, seed=1, contiguous=True), Full(bj, 3, nl, 2, "blake2s", seed=2, path_only=True)]
    want = check_batch(bj, G, fulls, edge_indices(nl, G))
    assert want[1].leaf_elements.shape[1] == 0


def test_two_oracles_one_below_the_world(bj):
    """cap 2 < G = 4 <= cap 8: the roots all-gather carries one oracle of the two.  A digest word
    >= p planted in the byte-digest tree comes back as it is, as a leaf hash and as a sibling."""
    G, nl = 4, 128
    fulls = [Full(bj, 16, nl, 2, "keccak256", seed=3), Full(bj, 33, nl, 8, "blake2s", seed=4)]
    for f in fulls:
        f.tree.leaf_hashes[5, 2] = -1
        f.tree.nodes[3, 1] = -1      # level 1, entry 3: the sibling of leaves 4 and 5 one level up
    idx = edge_indices(nl, G) + [5, 4]
    want = check_batch(bj, G, fulls, idx)
    for w in want:
        assert w.leaf_hash[-2][2] == np.uint64(2 ** 64 - 1) and w.proof[-1][0][2] == np.uint64(2 ** 64 - 1)
        assert w.proof[-1][1][1] == np.uint64(2 ** 64 - 1)


def test_four_oracles_two_below_the_world(bj):
    """G = 8, widths 1, 9, 0 (path only), 33, caps 4, 1, 16, 32, all three hashers: the roots of the
    two oracles with cap < G travel in one exchange and are dealt out per oracle."""
    G, nl = 8, 256
    fulls = [Full(bj, 1, nl, 4, "poseidon2", seed=5), Full(bj, 9, nl, 1, "blake2s", seed=6),
             Full(bj, 2, nl, 16, "keccak256", seed=7, path_only=True), Full(bj, 33, nl, 32, "poseidon2", seed=8)]
    check_batch(bj, G, fulls, edge_indices(nl, G))


def test_one_query_and_three_hundred(bj):
    G, nl = 4, 256
    fulls = [Full(bj, 9, nl, 2, seed=9), Full(bj, 16, nl, 16, "blake2s", seed=10)]
    check_batch(bj, G, fulls, [77])
    check_batch(bj, G, fulls, [int(i) for i in np.random.default_rng(5).integers(0, nl, size=300)])


def test_all_indices_owned_by_one_rank(bj):
    """Three of the four gathered buffers hold nothing that was written; none of it is selected."""
    G, nl = 4, 64
    check_batch(bj, G, [Full(bj, 9, nl, 1, seed=11)], [32, 47, 33, 32, 40])


def test_bad_index(bj):
    """One index >= n_leaves in a batch: the status record and an all-zero record on every rank, the
    other records intact; the wrapper raises on every rank."""
    G, nl = 4, 64
    fulls = [Full(bj, 9, nl, 2, seed=12), Full(bj, 1, nl, 8, "blake2s", seed=13)]
    good, bad = [3, 5, 7, 63], [3, 5, 64, 7, 63]
    want = bj.Q.construct_queries([f.plain for f in fulls], good)
    shards = [[f.shard(G, r) for f in fulls] for r in range(G)]
    total = len(bad) * sum(o.words for o in shards[0])

    def raw(comm, r):
        out = bj.torch.full((total,), -1, dtype=bj.torch.int64, device="cuda")
        status = bj.torch.full((4,), -1, dtype=bj.torch.int64, device="cuda")
        idx = bj.field.to_device(np.array(bad, dtype=np.uint64))
        bj.S.launch_sharded_queries(comm, shards[r], idx, out, status)
        return bj.field.to_host(out), bj.field.to_host(status)

    outs = run_ranks(bj, G, raw)
    for out, status in outs:
        assert status.tolist() == [1, 2, 0, 0]
        assert np.array_equal(out, outs[0][0])
        got = bj.Q.parse_queries(out, [(o.n_elements, o.depth) for o in shards[0]], len(bad))
        for w, g in zip(want, got):
            for part_w, part_g in zip(w, g):
                assert not part_g[2].any()
                assert np.array_equal(np.delete(part_g, 2, axis=0), part_w)

    def wrapped(comm, r):
        with pytest.raises(bj.Error, match="position 2"):
            bj.S.native_sharded_queries(comm, shards[r], bad)
        return True

    assert run_ranks(bj, G, wrapped) == [True] * G


def test_commit_then_queries_end_to_end(bj):
    """native_sharded_commit at world 4 for two traces of different widths, one
    native_sharded_queries call over both, against construct_queries on the one-GPU commits; the
    per-index route (native_sharded_query) agrees, and so does the serde form."""
    torch = bj.torch
    world, log_n, log_lde, cap, hasher = 4, 13, 1, 16, "poseidon2"
    widths = (16, 8)
    nl = 1 << (log_n + log_lde)
    traces = [bj.commit.synthetic_trace(c, log_n, seed=42 + c) for c in widths]
    plain = []
    for tr in traces:
        ws = bj.commit.witness_commit(tr, 1 << log_lde, cap)
        plain.append(bj.Q.QueryOracle(ws.tree(), ws.lde))
    indices = [0, 1, nl // 2 - 1, nl // 2, nl - 1, (nl * 3) // 7]
    want = bj.Q.construct_queries(plain, indices)
    want4 = bj.Q.single_round_queries(plain[0], plain[1], plain[0], plain[1], [], indices[:2])

    def rank_main(comm, r):
        oracles, results = [], []
        for c, tr in zip(widths, traces):
            cols = torch.tensor(bj.S.native_columns(c, world, r, hasher), device="cuda")
            res = bj.S.native_sharded_commit(comm, tr.index_select(0, cols).contiguous(), c, log_n, log_lde, cap, hasher)
            results.append(res)
            oracles.append(bj.S.ShardedQueryOracle(res, c, log_n, log_lde, cap, hasher))
        batched = bj.S.native_sharded_queries(comm, oracles, indices)
        single = [[bj.S.native_sharded_query(comm, res, c, log_n, log_lde, cap, i, hasher) for i in indices]
                  for c, res in zip(widths, results)]
        serde = bj.S.native_sharded_single_round_queries(comm, oracles[0], oracles[1], oracles[0], oracles[1],
                                                         indices[:2])
        return batched, single, serde

    for batched, single, serde in run_ranks(bj, world, rank_main, timeout=120):
        for w, g, one in zip(want, batched, single):
            for part_w, part_g in zip(w, g):
                assert np.array_equal(part_w, part_g)
            for q, (elems, leaf, proof) in enumerate(one):
                assert np.array_equal(elems, g.leaf_elements[q]) and np.array_equal(leaf, g.leaf_hash[q])
                assert np.array_equal(proof, g.proof[q])
        assert serde == want4 and serde[0]["fri_queries"] == []


def test_argument_errors_at_world_one(bj):
    """Every BJ_EINVAL of the contract, at world 1 so that no rank can be left waiting."""
    EINVAL, D = -22, bj._lib.ShardedQueryOracleDesc
    nl = 64
    a, b = Full(bj, 9, nl, 4, seed=14).shard(1, 0), Full(bj, 2, nl, 8, "blake2s", seed=15).shard(1, 0)
    words = a.words + b.words
    idx = bj.field.to_device(np.array([1, 2], dtype=np.uint64))
    out = bj.torch.empty((2 * words,), dtype=bj.torch.int64, device="cuda")
    status = bj.torch.empty((4,), dtype=bj.torch.int64, device="cuda")
    group = bj.S.LocalGroup(1)
    comm = group.comm(0)

    def run(descs, n_oracles=None, comm_p=comm.handle, indices=idx.data_ptr(), n_queries=2, out_p=out.data_ptr(),
            out_words=2 * words, status_p=status.data_ptr()):
        arr = (D * max(len(descs), 1))(*descs)
        return bj.lib.bj_sharded_queries_d(comm_p, arr if descs else None,
                                           len(descs) if n_oracles is None else n_oracles, indices, n_queries, out_p,
                                           out_words, status_p, None)

    def changed(o, **kw):
        d = o.descriptor()
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    try:
        good = [a.descriptor(), b.descriptor()]
        assert run(good) == 0
        assert run(good, comm_p=None) == EINVAL
        assert run([]) == EINVAL and run(good, n_oracles=0) == EINVAL             # n_oracles outside 1..16
        assert run([a.descriptor()] * 17) == EINVAL
        assert run(good, n_queries=0) == EINVAL
        assert run(good, indices=None) == EINVAL and run(good, out_p=None) == EINVAL
        assert run(good, status_p=None) == EINVAL
        assert run([a.descriptor(), changed(b, leaves=None)]) == EINVAL
        assert run([changed(a, nodes=None), b.descriptor()]) == EINVAL
        assert run([changed(a, src=None), b.descriptor()]) == EINVAL               # n_cols > 0 needs src
        assert run([changed(a, src=None, n_cols=0), b.descriptor()], out_words=2 * (words - a.n_cols)) == 0
        assert run([changed(a, n_leaves=48), changed(b, n_leaves=48)]) == EINVAL   # no power of two
        assert run([changed(a, n_leaves=0), changed(b, n_leaves=0)]) == EINVAL
        assert run([changed(a, cap_size=3), b.descriptor()]) == EINVAL
        assert run([a.descriptor(), changed(b, cap_size=0)]) == EINVAL
        assert run([a.descriptor(), changed(b, n_leaves=32)]) == EINVAL            # n_leaves differ
        assert b"differs" in bj.lib.bj_last_error()
        assert run([a.descriptor(), changed(b, cap_size=64)]) == EINVAL            # m <= cap_local
        assert run([a.descriptor(), changed(b, cap_size=128)]) == EINVAL
        assert run([changed(a, col_stride=nl - 1), b.descriptor()]) == EINVAL
        assert b"col_stride" in bj.lib.bj_last_error()
        assert run([a.descriptor(), changed(b, hasher=3)]) == EINVAL
        assert run([changed(a, hasher=-1), b.descriptor()]) == EINVAL
        assert run(good, out_words=2 * words - 1) == EINVAL
        assert b"out_words" in bj.lib.bj_last_error()
        assert run(good) == 0                                                       # the group is still usable
        bj.torch.cuda.synchronize()
        assert bj.field.to_host(status).tolist() == [0, 2 ** 64 - 1, 0, 0]
    finally:
        comm.close()
        group.close()

