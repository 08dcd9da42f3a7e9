"""bj_oracle_queries_d / boojum_amd.queries on the GPU, bit-exact against what the project already
offers one query at a time: MerkleTreeWithCap.get_proof for the leaf hash and the path, direct
indexing of the source tensor for the leaf's elements, and the library's host hash_into_leaf /
verify_proof_over_cap for the tie between them (proof.rs:64-97, merkle_tree.rs:462-504)."""
import ctypes

import numpy as np
import pytest

P = 0xFFFFFFFF00000001
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bj():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import boojum_amd
    from boojum_amd import _lib, field, fri, merkle, queries, serialization
    lib = boojum_amd.load()
    return type("BJ", (), dict(torch=torch, field=field, fri=fri, merkle=merkle, Q=queries, lib=lib, _lib=_lib,
                               ser=serialization, Tree=merkle.MerkleTreeWithCap, Error=boojum_amd.BoojumError))


def rand(shape, seed):
    return np.random.default_rng(seed).integers(0, P, size=shape, dtype=np.uint64)


def check_oracle(bj, res, oracle, flat_src, indices, hashed=()):
    """res: the OracleQueries of `oracle` for `indices`; flat_src: host (C, L) array of what the
    leaves hashed, or None.  Every record against get_proof and the source; the positions in
    `hashed` also through the host hasher: the elements hash to the leaf, the path leads to the cap."""
    tree, e = oracle.tree, oracle.elements_per_leaf
    assert res.leaf_hash.shape == (len(indices), 4) and res.proof.shape == (len(indices), oracle.depth, 4)
    assert res.leaf_elements.shape == (len(indices), oracle.n_cols * e)
    for q, idx in enumerate(indices):
        t = idx >> oracle.index_shift
        leaf, path = tree.get_proof(t)
        assert np.array_equal(res.leaf_hash[q], leaf), (q, idx)
        assert np.array_equal(res.proof[q], path), (q, idx)
        if flat_src is not None:
            # column 0's e elements, then column 1's, ...
            assert np.array_equal(res.leaf_elements[q], flat_src[:, t * e: (t + 1) * e].reshape(-1)), (q, idx)
    H = bj.merkle.HASHERS[tree.hasher][0]
    cap = tree.get_cap()
    for q in hashed:
        t = indices[q] >> oracle.index_shift
        assert np.array_equal(H.hash_into_leaf(res.leaf_elements[q]), res.leaf_hash[q])
        assert bj.Tree.verify_proof_over_cap(res.proof[q], cap, res.leaf_hash[q], t, hasher=tree.hasher)


# ------------------------------------------------------------------ one oracle at a time

@pytest.mark.parametrize("n_cols", [1, 7, 300])
def test_witness_like_oracle_all_indices(bj, n_cols):
    """n = 2^6, D = 2, cap 4: all 128 indices in one call; 300 columns are more than a block's threads."""
    src = rand((n_cols, 2, 64), n_cols)
    dev = bj.field.to_device(src)
    o = bj.Q.QueryOracle(bj.Tree.construct(dev, 4), dev)
    assert (o.n_leaves, o.depth, o.col_stride, o.words) == (128, 5, 128, n_cols + 24)
    assert bj.Q.oracle_query_words(o) == o.words
    idx = list(range(128))
    res, = bj.Q.construct_queries([o], idx)
    check_oracle(bj, res, o, src.reshape(n_cols, 128), idx, hashed=(0, 77, 127))


@pytest.mark.parametrize("e,words", [(1, 600 + 4 + 20), (2, 1200 + 4 + 16)])
def test_wide_oracle_takes_several_passes(bj, e, words):
    """600 columns: four words per lane in one pass (624 words), and with two elements per leaf a
    second pass for the words past 1024."""
    src = rand((600, 128), 600 + e)
    dev = bj.field.to_device(src)
    tree = bj.Tree.construct(dev, 4) if e == 1 else bj.Tree.construct_by_chunking(dev, e, 4)
    o = bj.Q.QueryOracle(tree, dev, e, e.bit_length() - 1)
    assert (o.n_cols, o.words) == (600, words)
    idx = [0, 1, 64, 127, 31]
    res, = bj.Q.construct_queries([o], idx)
    check_oracle(bj, res, o, src, idx, hashed=(1,))


def test_tree_over_a_subset_of_cosets(bj):
    """D = 4 with the tree over the first 2 cosets: the column stride is 4 n, the domain 2 n."""
    src = rand((3, 4, 64), 11)
    dev = bj.field.to_device(src)
    o = bj.Q.QueryOracle(bj.Tree.construct(dev, 4, num_cosets=2), dev)
    assert (o.n_leaves, o.col_stride) == (128, 256)
    idx = list(range(128))
    res, = bj.Q.construct_queries([o], idx)
    check_oracle(bj, res, o, src.reshape(3, 256), idx, hashed=(64, 127))
    with pytest.raises(bj.Error):
        bj.Q.construct_queries([o], [128])   # coset 2 is in the tensor but not in the tree


def test_depth_16(bj):
    """One column on 2^16 leaves with cap 1: the 68 digest words are more than one wave."""
    src = rand((1, 1 << 16), 16)
    dev = bj.field.to_device(src)
    o = bj.Q.QueryOracle(bj.Tree.construct(dev, 1), dev)
    assert (o.depth, o.words) == (16, 1 + 4 + 64)
    idx = [0, 1, 65535, 65534, 12345, 32768, 43690, 21845]
    res, = bj.Q.construct_queries([o], idx)
    check_oracle(bj, res, o, src, idx, hashed=(2, 4))


@pytest.mark.parametrize("e", [2, 4, 8])
def test_chunked_leaves(bj, e):
    """construct_by_chunking over two columns: c0's E elements, then c1's E."""
    src = rand((2, 2, 64), 20 + e)
    dev = bj.field.to_device(src)
    shift = e.bit_length() - 1
    o = bj.Q.QueryOracle(bj.Tree.construct_by_chunking(dev, e, 4), dev, e, shift)
    assert (o.n_leaves, o.domain, o.n_elements) == (128 // e, 128, 2 * e)
    idx = list(range(128))
    res, = bj.Q.construct_queries([o], idx)
    flat = src.reshape(2, 128)
    check_oracle(bj, res, o, flat, idx, hashed=range(0, 128, 9))
    t = 77 >> shift
    assert np.array_equal(res.leaf_elements[77][:e], flat[0, t * e: (t + 1) * e])
    assert np.array_equal(res.leaf_elements[77][e:], flat[1, t * e: (t + 1) * e])


def test_flat_sources_with_tree_equal_to_cap(bj):
    """n_leaves == cap_size (the last FRI oracle): depth 0, nodes = NULL, the leaf is the cap entry."""
    src = rand((2, 32), 31)
    dev = bj.field.to_device(src)
    tree = bj.Tree.construct_by_chunking_from_flat_sources(dev, 2, 16)
    o = bj.Q.QueryOracle(tree, dev, 2, 1)
    assert (o.n_leaves, o.depth, o.words) == (16, 0, 8) and not o.descriptor().nodes
    idx = list(range(32))
    res, = bj.Q.construct_queries([o], idx)
    check_oracle(bj, res, o, src, idx, hashed=(0, 31))
    assert res.proof.shape == (32, 0, 4)
    assert np.array_equal(res.leaf_hash[9], tree.get_cap()[4])


@pytest.mark.parametrize("hasher", ["blake2s", "keccak256"])
def test_byte_digest_hashers_come_back_unreduced(bj, hasher):
    src = rand((5, 2, 64), 40)
    dev = bj.field.to_device(src)
    o = bj.Q.QueryOracle(bj.Tree.construct(dev, 4, hasher=hasher), dev)
    idx = list(range(128))
    res, = bj.Q.construct_queries([o], idx)
    check_oracle(bj, res, o, src.reshape(5, 128), idx, hashed=(3, 100))
    # digests are bytes, so words >= p occur, if only once in 2^32: plant one in this test's own
    # tree (the copy does not care what the bits are) and see it come back as it is
    t = 5
    o.tree.leaf_hashes[t, 2] = -1
    r, = bj.Q.construct_queries([o], [t, t ^ 1])
    want = bj.field.to_host(o.tree.leaf_hashes[t])
    assert (want >= np.uint64(P)).any()
    assert np.array_equal(r.leaf_hash[0], want) and np.array_equal(r.proof[1][0], want)


def test_path_only(bj):
    dev = bj.field.to_device(rand((4, 2, 64), 50))
    o = bj.Q.QueryOracle(bj.Tree.construct(dev, 8))
    assert (o.n_cols, o.words) == (0, 4 + 16) and not o.descriptor().src
    idx = [0, 127, 5, 5]
    res, = bj.Q.construct_queries([o], idx)
    assert res.leaf_elements.shape == (4, 0)
    check_oracle(bj, res, o, None, idx)


def test_oracle_query_construct_takes_the_reference_arguments(bj):
    """OracleQuery::construct(tree, source, lde_factor, coset_idx, domain_size, inner_idx, num_elements)."""
    src = rand((2, 2, 64), 60)
    dev = bj.field.to_device(src)
    tree = bj.Tree.construct_by_chunking(dev, 4, 4)
    q = bj.Q.OracleQuery.construct(tree, dev, 2, 1, 64, 37, 4)
    t = (1 << (6 - 2)) + 37 // 4
    leaf, path = tree.get_proof(t)
    assert np.array_equal(q.proof, path)
    assert np.array_equal(q.leaf_elements, src.reshape(2, 128)[:, 4 * t: 4 * t + 4].reshape(-1))
    assert np.array_equal(bj.merkle.Poseidon2Sponge.hash_into_leaf(q.leaf_elements), leaf)
    assert q.to_json() == bj.ser.oracle_query_to_json(q.leaf_elements, path)


# ------------------------------------------------------------------ a whole round

@pytest.fixture(scope="module")
def round_(bj):
    """n = 2^8, LDE 2, cap 4, schedule [3, 2, 1]: four base oracles of different widths and the three
    FRI oracles over a random codeword folded with fri.interpolate.  Built once, never written."""
    log_n, log_lde, cap, schedule = 8, 1, 4, [3, 2, 1]
    n, full = 1 << log_n, 1 << (log_n + log_lde)
    oracles, srcs = [], []
    for i, c in enumerate((9, 5, 2, 13)):
        s = rand((c, 2, n), 70 + i)
        d = bj.field.to_device(s)
        oracles.append(bj.Q.QueryOracle(bj.Tree.construct(d, cap), d))
        srcs.append(s.reshape(c, full))
    code = bj.field.to_device(rand((2, full), 80))
    roots = bj.fri.precompute_roots(full)
    plan = bj.Q.fri_plan(log_n, log_lde, schedule)
    ci = None
    for k, (s, (e, shift, n_leaves)) in enumerate(zip(schedule, plan)):
        if k == 0:
            tree = bj.Tree.construct_by_chunking(code.reshape(2, 2, n), e, cap)
        else:
            tree = bj.Tree.construct_by_chunking_from_flat_sources(code, e, cap)
        assert tree.n_leaves == n_leaves
        oracles.append(bj.Q.QueryOracle(tree, code, e, shift))
        srcs.append(bj.field.to_host(code))
        c0, c1, ci = bj.fri.interpolate(code[0], code[1], bj.fri.challenge_powers((1234 + k, 5678), s), roots, ci)
        code = bj.torch.stack([c0, c1])
    indices = [0, full - 1, 300, 7, 300, 256, 255, 511 - 8, 64, 65, 66, 67, 129, 400, 31, 32]
    return type("Round", (), dict(log_n=log_n, schedule=schedule, oracles=oracles, srcs=srcs, indices=indices))


def test_whole_round(bj, round_):
    r = round_
    assert len(r.oracles) == 7 and len(r.indices) == 16
    assert [o.words for o in r.oracles] == [9 + 32, 5 + 32, 2 + 32, 13 + 32, 16 + 4 + 16, 8 + 4 + 8, 4 + 4 + 4]
    res = bj.Q.construct_queries(r.oracles, r.indices)
    for o, s, rr in zip(r.oracles, r.srcs, res):
        check_oracle(bj, rr, o, s, r.indices, hashed=(1, 2))
    # the FRI tree indices from (coset_idx, inner_idx) as the reference computes them
    # (prover.rs:2226-2254, proof.rs:89-91), not from the flat shift
    n = 1 << r.log_n
    for q, index in enumerate(r.indices):
        coset_idx, inner_idx = divmod(index, n)
        domain_size = n
        for k, s in enumerate(r.schedule):
            e = 1 << s
            tree_idx = (coset_idx << (domain_size.bit_length() - 1 - s)) + inner_idx // e
            o = r.oracles[4 + k]
            leaf, path = o.tree.get_proof(tree_idx)
            assert np.array_equal(res[4 + k].leaf_hash[q], leaf) and np.array_equal(res[4 + k].proof[q], path)
            assert np.array_equal(res[4 + k].leaf_elements[q],
                                  r.srcs[4 + k][:, tree_idx * e: (tree_idx + 1) * e].reshape(-1))
            inner_idx >>= s
            domain_size >>= s


def test_single_round_queries_serde_shape(bj, round_):
    r = round_
    got = bj.Q.single_round_queries(*r.oracles[:4], r.oracles[4:], r.indices[:3])
    assert len(got) == 3

    def want(o, index):
        t, e = index >> o.index_shift, o.elements_per_leaf
        s = r.srcs[r.oracles.index(o)]
        return bj.ser.oracle_query_to_json(s[:, t * e: (t + 1) * e].reshape(-1), o.tree.get_proof(t)[1])

    for g, index in zip(got, r.indices):
        assert list(g) == ["witness_query", "stage_2_query", "quotient_query", "setup_query", "fri_queries"]
        for name, o in zip(list(g)[:4], r.oracles):
            assert g[name] == want(o, index)
        assert g["fri_queries"] == [want(o, index) for o in r.oracles[4:]]
    assert bj.ser.dumps(got[0]).startswith('{"witness_query":{"leaf_elements":[')


# ------------------------------------------------------------------ status, errors, graphs

def _buffers(bj, oracles, n_queries, fill=-1):
    total = n_queries * sum(o.words for o in oracles)
    out = bj.torch.full((total,), fill, dtype=bj.torch.int64, device="cuda")
    status = bj.torch.full((4,), fill, dtype=bj.torch.int64, device="cuda")
    return out, status


def _parse(bj, out, oracles, n_queries):
    return bj.Q.parse_queries(bj.field.to_host(out), [(o.n_elements, o.depth) for o in oracles], n_queries)


def test_bad_index(bj, round_):
    oracles = [round_.oracles[0], round_.oracles[5]]
    good, bad = [3, 5, 7, 511], [3, 5, 512, 7, 511]
    want = bj.Q.construct_queries(oracles, good)
    out, status = _buffers(bj, oracles, len(bad))
    bj.Q.launch_queries(oracles, bj.field.to_device(np.array(bad, dtype=np.uint64)), out, status)
    assert bj.field.to_host(status).tolist() == [1, 2, 0, 0]
    for w, g in zip(want, _parse(bj, out, oracles, len(bad))):
        for part_w, part_g in zip(w, g):
            assert not part_g[2].any()                                   # the bad query's records are zero
            assert np.array_equal(np.delete(part_g, 2, axis=0), part_w)   # the others are intact
    with pytest.raises(bj.Error, match="position 2"):
        bj.Q.construct_queries(oracles, bad)
    # a good batch rewrites the record
    bj.Q.launch_queries(oracles, bj.field.to_device(np.array(good, dtype=np.uint64)), out, status)
    assert bj.field.to_host(status).tolist() == [0, 2 ** 64 - 1, 0, 0]
    # several bad ones, 2^64 - 1 among them: the count and the first position
    many = np.array([1 << 40, 0, 2 ** 64 - 1] + [512] * 300, dtype=np.uint64)
    out, status = _buffers(bj, oracles, many.size)
    bj.Q.launch_queries(oracles, bj.field.to_device(many), out, status)
    assert bj.field.to_host(status).tolist() == [302, 0, 0, 0]


def test_argument_errors(bj, round_):
    EINVAL, D = -22, bj._lib.QueryOracleDesc
    a, b = round_.oracles[0], round_.oracles[6]
    idx = bj.field.to_device(np.array([1, 2], dtype=np.uint64))
    out, status = _buffers(bj, [a, b], 2)
    words = a.words + b.words

    def run(descs, n_oracles=None, indices=idx.data_ptr(), n_queries=2, out_p=out.data_ptr(), out_words=2 * words,
            status_p=status.data_ptr()):
        arr = (D * max(len(descs), 1))(*descs)
        return bj.lib.bj_oracle_queries_d(arr if descs else None, len(descs) if n_oracles is None else n_oracles,
                                          indices, n_queries, out_p, out_words, status_p, None)

    def changed(o, **kw):
        d = o.descriptor()
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    good = [a.descriptor(), b.descriptor()]
    assert run(good) == 0
    assert run([]) == EINVAL and run(good, n_oracles=0) == EINVAL                 # n_oracles outside 1..16
    assert run([a.descriptor()] * 17) == EINVAL
    assert run(good, n_queries=0) == EINVAL
    assert run(good, indices=None) == EINVAL and run(good, out_p=None) == EINVAL and run(good, status_p=None) == EINVAL
    assert run([a.descriptor(), changed(b, leaves=None)]) == EINVAL
    assert run([changed(a, nodes=None), b.descriptor()]) == EINVAL                # depth 5 needs nodes
    assert run([a.descriptor(), changed(b, nodes=None)]) == EINVAL                # and so does depth 1
    assert run([a.descriptor(), changed(b, nodes=None, cap_size=b.n_leaves)]) == 0       # depth 0 does not
    assert run([changed(a, src=None), b.descriptor()]) == EINVAL                  # n_cols > 0 needs src
    assert run([changed(a, src=None, n_cols=0), b.descriptor()], out_words=2 * (words - a.n_cols)) == 0
    assert run([changed(a, n_leaves=384, index_shift=0), b.descriptor()]) == EINVAL      # no power of two
    assert run([changed(a, n_leaves=0), b.descriptor()]) == EINVAL
    assert run([changed(a, cap_size=3), b.descriptor()]) == EINVAL
    assert run([changed(a, cap_size=0), b.descriptor()]) == EINVAL
    assert run([a.descriptor(), changed(b, cap_size=2 * b.n_leaves)]) == EINVAL   # n_leaves < cap_size
    assert run([changed(a, col_stride=a.n_leaves - 1), b.descriptor()]) == EINVAL
    assert run([a.descriptor(), changed(b, col_stride=(b.n_leaves << b.log_e) - 1)]) == EINVAL
    assert run([a.descriptor(), changed(b, index_shift=b.index_shift - 1)]) == EINVAL    # domains disagree
    assert run(good, out_words=2 * words - 1) == EINVAL
    assert b"out_words" in bj.lib.bj_last_error()
    assert bj.lib.bj_oracle_query_words(None) == 0
    assert bj.lib.bj_oracle_query_words(ctypes.byref(changed(a, cap_size=3))) == 0
    bj.torch.cuda.synchronize()


def test_graph_replay_follows_the_index_buffer(bj, round_):
    """The call captures as it is (descriptors by value, nothing allocated, no synchronisation);
    a replay reads the index buffer as it is then."""
    torch = bj.torch
    oracles = round_.oracles
    first, second = [0, 511, 300, 77], [12, 256, 255, 300]
    idx = bj.field.to_device(np.array(first, dtype=np.uint64))
    out, status = _buffers(bj, oracles, 4)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # load the kernel before the capture
        bj.Q.launch_queries(oracles, idx, out, status)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        bj.Q.launch_queries(oracles, idx, out, status)
    for indices in (first, second):
        idx.copy_(bj.field.to_device(np.array(indices, dtype=np.uint64)))
        out.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert bj.field.to_host(status).tolist() == [0, 2 ** 64 - 1, 0, 0]
        want = bj.Q.construct_queries(oracles, indices)
        for w, got in zip(want, _parse(bj, out, oracles, 4)):
            for part_w, part_g in zip(w, got):
                assert np.array_equal(part_w, part_g)
