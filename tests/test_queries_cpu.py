"""The host arithmetic of boojum_amd.queries, without a GPU and without the HIP library.

* The plan against the reference's own proof: `fri_plan`'s shifts and leaf widths, applied to the
  flat query indices of tests/golden/proof_queries.json, verify every FRI query of
  tests/golden/proof_fri.json to its cap (prover.rs:2226-2254, proof.rs:89-91), the last oracle's
  empty path included.
* The layout of bj_oracle_queries_d's output: record words, block offsets and parsing against the
  formula of include/boojum_mi355x.h.
"""
import json
import os

import numpy as np
import pytest

import oracle as O
from boojum_amd import queries as Q

HERE = os.path.dirname(os.path.abspath(__file__))
FRI = json.load(open(os.path.join(HERE, "golden", "proof_fri.json")))
QRY = json.load(open(os.path.join(HERE, "golden", "proof_queries.json")))
LOG_N, LOG_LDE, CAP, SCHEDULE = 20, 1, 32, [3, 3, 3, 3, 3, 1]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    O.lib()


def test_module_is_exported():
    import boojum_amd
    assert "queries" in boojum_amd.__all__


def test_fri_plan_of_the_reference_proof():
    assert FRI["vk"]["domain_size"] == 1 << LOG_N and FRI["proof_config"]["fri_lde_factor"] == 1 << LOG_LDE
    assert Q.fri_plan(LOG_N, LOG_LDE, SCHEDULE) == [
        (8, 3, 1 << 18), (8, 6, 1 << 15), (8, 9, 1 << 12), (8, 12, 1 << 9), (8, 15, 1 << 6), (2, 16, 1 << 5)]
    # every oracle covers the same domain, which is what bj_oracle_queries_d requires
    assert {n << s for _, s, n in Q.fri_plan(LOG_N, LOG_LDE, SCHEDULE)} == {1 << 21}
    assert Q.fri_plan(4, 2, []) == []
    with pytest.raises(ValueError):
        Q.fri_plan(4, 1, [3, 2])   # folds 2^5 > 2^4 rows
    with pytest.raises(ValueError):
        Q.fri_plan(4, 1, [0])


@pytest.mark.parametrize("qi", range(6))
def test_plan_verifies_the_reference_fri_queries(qi):
    index = QRY["queries"][qi]["index"]
    q = FRI["queries"][qi]
    # the two fixtures hold the same query
    assert q["witness_query"]["leaf_elements"] == QRY["queries"][qi]["witness"]["leaf_elements"]
    caps = [FRI["fri_base_oracle_cap"]] + FRI["fri_intermediate_oracles_caps"]
    plan = Q.fri_plan(LOG_N, LOG_LDE, SCHEDULE)
    assert len(q["fri_queries"]) == len(plan) == len(caps) == 6
    for (e, shift, n_leaves), fq, cap in zip(plan, q["fri_queries"], caps):
        assert len(fq["leaf_elements"]) == 2 * e
        assert len(fq["proof"]) == (n_leaves // CAP).bit_length() - 1
        assert len(cap) == CAP
        leaf = O.hash_into_leaf(fq["leaf_elements"])
        assert O.verify_proof_over_cap(fq["proof"], cap, leaf, index >> shift)
        # the index matters: the neighbour leaf does not verify
        assert not O.verify_proof_over_cap(fq["proof"], cap, leaf, (index >> shift) ^ 1)
    # the depth-0 oracle: n_leaves == cap_size, the leaf hash is the cap entry itself
    assert plan[-1][2] == CAP and q["fri_queries"][-1]["proof"] == []
    assert Q.query_words(2, plan[-1][0], plan[-1][2], CAP) == 4 + 4


def test_shift_is_the_reference_index_arithmetic():
    """proof.rs:89-91 / prover.rs:2226-2254 step by step against the flat shift, over both cosets."""
    n = 1 << LOG_N
    plan = Q.fri_plan(LOG_N, LOG_LDE, SCHEDULE)
    for q in QRY["queries"]:
        coset, inner = divmod(q["index"], n)
        domain_size = n
        for s, (e, shift, _) in zip(SCHEDULE, plan):
            assert e == 1 << s
            tree_idx = (coset << (domain_size.bit_length() - 1 - s)) + inner // e
            assert tree_idx == q["index"] >> shift
            inner >>= s
            domain_size >>= s
        assert q["fri_base"]["index"] == q["index"] >> plan[0][1]


@pytest.mark.parametrize("n_cols,e,n_leaves,cap,want", [
    (156, 1, 1 << 21, 32, 156 + 4 + 64), (167, 1, 1 << 21, 32, 167 + 4 + 64), (2, 8, 1 << 18, 32, 16 + 4 + 52),
    (2, 2, 32, 32, 4 + 4), (0, 1, 64, 1, 4 + 24), (600, 1, 128, 4, 600 + 4 + 20)])
def test_query_words(n_cols, e, n_leaves, cap, want):
    # (n_cols << e') + 4 + 4 * log2(n_leaves / cap_size)
    assert Q.query_words(n_cols, e, n_leaves, cap) == want


def test_query_words_rejects_bad_sizes():
    for args in ((1, 3, 64, 4), (1, 1, 48, 4), (1, 1, 64, 3), (1, 1, 4, 8)):
        with pytest.raises(ValueError):
            Q.query_words(*args)


def test_reference_proof_query_counts():
    """One query of the reference's proof touches 10 oracles and its paths hold 99 digests."""
    plan = Q.fri_plan(LOG_N, LOG_LDE, SCHEDULE)
    depths = [16] * 4 + [(n // CAP).bit_length() - 1 for _, _, n in plan]
    assert len(depths) == 10 and sum(depths) == 99


def test_block_offsets():
    assert Q.block_offsets([10, 3, 8], 5) == [0, 50, 65, 105]
    assert Q.block_offsets([], 7) == [0]


def test_parse_hand_made_buffer():
    """Two oracles, three queries: oracle 0 has 3 leaf elements and depth 2 (15 words), oracle 1 no
    elements and depth 0 (4 words).  Word values encode (oracle, query, word)."""
    shapes, nq = [(3, 2), (0, 0)], 3
    words = [15, 4]
    buf = np.zeros(nq * sum(words) + 5, dtype=np.uint64)   # spare words behind are ignored
    at = 0
    for o, w in enumerate(words):
        for q in range(nq):
            for i in range(w):
                buf[at] = 10000 * o + 100 * q + i
                at += 1
    r0, r1 = Q.parse_queries(buf, shapes, nq)
    assert r0.leaf_elements.shape == (3, 3) and r0.leaf_hash.shape == (3, 4) and r0.proof.shape == (3, 2, 4)
    assert r0.leaf_elements[1].tolist() == [100, 101, 102]
    assert r0.leaf_hash[2].tolist() == [203, 204, 205, 206]
    assert r0.proof[0].tolist() == [[7, 8, 9, 10], [11, 12, 13, 14]]
    assert r1.leaf_elements.shape == (3, 0) and r1.proof.shape == (3, 0, 4)   # n_leaves == cap_size: empty proof
    assert r1.leaf_hash[1].tolist() == [10100, 10101, 10102, 10103]
    with pytest.raises(ValueError):
        Q.parse_queries(buf[:56], shapes, nq)


def test_oracle_query_json_shape():
    q = Q.OracleQuery(np.array([1, 2, 3], dtype=np.uint64), np.arange(8, dtype=np.uint64).reshape(2, 4))
    assert q.to_json() == {"leaf_elements": [1, 2, 3], "proof": [[0, 1, 2, 3], [4, 5, 6, 7]]}
