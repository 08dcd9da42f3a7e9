"""The schedule of bj_sharded_queries_d on the CPU (tests/sharded_queries_model.py): the owner's
records from its subtree and the top levels, one gather and the select give, on every rank, the
plain get_proof-order records of the full tree.  No GPU; the library is loaded only for the host
arithmetic of bj_sharded_query_words."""
import ctypes

import numpy as np
import pytest

import sharded_queries_model as M
from boojum_amd import queries as Q

P = 0xFFFFFFFF00000001


def rand(shape, seed, hi=P):
    return np.random.default_rng(seed).integers(0, hi, size=shape, dtype=np.uint64)


def oracle_of(n_cols, nl, cap, G, seed, node=M.mix_node):
    """A full tree over random leaves (the model moves digests, so the leaves need not hash the
    sources) and its G shards."""
    src = rand((n_cols, nl), seed) if n_cols else None
    leaves, nodes = M.build_tree(rand((nl, 4), seed + 1, 2 ** 64 - 1), cap, node)
    shards = []
    for r in range(G):
        lv, nd = M.shard_tree(leaves, nodes, cap, G, r)
        m = nl // G
        shards.append((None if src is None else src[:, r * m: (r + 1) * m], lv, nd))
    return dict(src=src, leaves=leaves, nodes=nodes, n_leaves=nl, cap=cap, shards=shards, node=node)


def want(oracles, indices):
    return np.concatenate([M.plain_records(o["src"], o["leaves"], o["nodes"], o["cap"], indices).reshape(-1)
                           for o in oracles])


def edge_indices(nl, G):
    m = nl // G
    return sorted({0, 1, m - 1, m % nl, nl // 2 - 1, nl // 2, nl - 1}) + [1, 1]


@pytest.mark.parametrize("G", [1, 2, 4, 8])
@pytest.mark.parametrize("cap", [1, 2, 4, 8, 16])
def test_model_equals_plain_records(G, cap):
    """cap < G, = G and > G for every world; m = 2 cap_local (local depth 1) among them."""
    nl = 64
    o = oracle_of(5, nl, cap, G, 10 * G + cap)
    idx = edge_indices(nl, G) + list(range(0, nl, 3))
    for out, status in M.sharded_queries([o], G, idx):
        assert np.array_equal(out, want([o], idx))
        assert status.tolist() == [0, 2 ** 64 - 1, 0, 0]


@pytest.mark.parametrize("G,nl,cap", [(2, 4, 1), (4, 8, 4), (8, 16, 8), (8, 32, 16), (8, 16, 1)])
def test_local_depth_one(G, nl, cap):
    """m = 2 cap_local: the subtree is the leaves and one level."""
    o = oracle_of(3, nl, cap, G, nl + cap)
    assert o["shards"][0][2].shape[0] == max(1, cap // G)
    idx = list(range(nl))
    for out, _ in M.sharded_queries([o], G, idx):
        assert np.array_equal(out, want([o], idx))


def test_shard_is_a_slice_of_every_level():
    nl, cap, G = 64, 2, 4
    leaves, nodes = M.build_tree(rand((nl, 4), 3), cap)
    for r in range(G):
        lv, nd = M.shard_tree(leaves, nodes, cap, G, r)
        assert lv.shape == (16, 4) and nd.shape == (15, 4)          # cap_local = 1: down to the subtree root
        assert np.array_equal(nd[-1], M.level(leaves, nodes, 4)[r])
        # a shard is itself a tree under the same node function
        assert np.array_equal(nd, M.tree_nodes(lv, 1))
    with pytest.raises(ValueError):
        M.shard_tree(leaves, nodes, 64, 4, 0)


def test_several_oracles_with_a_subset_below_the_world():
    """Four oracles of different widths and caps in one call, G = 8: two have cap < G (their roots
    travel together), one cap = G, one cap > G, one is path-only; each with its own node function."""
    G, nl = 8, 128
    other = lambda a, b: M.mix_node(b, a)  # noqa: E731
    oracles = [oracle_of(1, nl, 4, G, 1), oracle_of(9, nl, 8, G, 2, other), oracle_of(0, nl, 1, G, 3, other),
               oracle_of(33, nl, 32, G, 4)]
    idx = edge_indices(nl, G) + [17] * 3
    w = want(oracles, idx)
    assert w.size == len(idx) * sum(M.words(c, nl, cap) for c, cap in ((1, 4), (9, 8), (0, 1), (33, 32)))
    outs = M.sharded_queries(oracles, G, idx)
    for out, _ in outs:
        assert np.array_equal(out, w)
    parsed = Q.parse_queries(outs[3][0], [(1, 5), (9, 4), (0, 7), (33, 2)], len(idx))
    assert np.array_equal(parsed[1].leaf_elements[2], oracles[1]["src"][:, idx[2]])
    assert np.array_equal(parsed[2].leaf_hash[4], oracles[2]["leaves"][idx[4]])


def test_all_indices_owned_by_one_rank_and_bad_indices():
    G, nl = 4, 64
    o = oracle_of(2, nl, 2, G, 7)
    idx = [32, 47, 33, 32]                       # rank 2 owns everything: the other buffers stay unwritten
    for out, _ in M.sharded_queries([o], G, idx):
        assert np.array_equal(out, want([o], idx))
    bad = [5, 64, 2 ** 64 - 1, 6]
    for out, status in M.sharded_queries([o], G, bad):
        assert np.array_equal(out, want([o], bad))   # zero records at positions 1 and 2
        assert status.tolist() == [2, 1, 0, 0]
    assert not want([o], bad).reshape(4, -1)[1:3].any()


@pytest.mark.parametrize("n_cols,n_leaves,cap", [(156, 1 << 21, 32), (0, 64, 1), (33, 1 << 10, 1 << 9), (1, 2, 1)])
def test_library_words_equal_the_unsharded_formula(n_cols, n_leaves, cap):
    from boojum_amd import _lib
    d = _lib.ShardedQueryOracleDesc(None, 0, n_cols, 0, None, None, n_leaves, cap, 0)
    got = _lib.load().bj_sharded_query_words(ctypes.byref(d))
    assert got == Q.query_words(n_cols, 1, n_leaves, cap) == M.words(n_cols, n_leaves, cap)


def test_library_words_reject_bad_sizes():
    from boojum_amd import _lib
    lib = _lib.load()
    assert lib.bj_sharded_query_words(None) == 0
    for n_leaves, cap in ((48, 4), (64, 3), (0, 1), (64, 0), (4, 8)):
        d = _lib.ShardedQueryOracleDesc(None, 0, 1, 0, None, None, n_leaves, cap, 0)
        assert lib.bj_sharded_query_words(ctypes.byref(d)) == 0
