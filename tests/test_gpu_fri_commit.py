"""The FRI commit phase on the GPU: bj_fri_fold_multi_d (`fri.fold_by`), `fri.final_monomials`,
`fri.do_fri` and `transcript.Poseidon2Transcript`, bit-exact against the chain of by-2 folds, the
oracle, the model of tests/fri_model.py and the oracle's transcript."""
import numpy as np
import pytest

import oracle as O
import transcript as T

import fri_model as M

pytestmark = pytest.mark.gpu

SPECIALS = [0, O.P - 1, O.P, O.P + 1, (1 << 64) - 1]
OFFSETS = [(0, 0), (1, 3), (3, 0)]     # elements into the buffers: (16-byte aligned, 8, 8), c0 != c1


@pytest.fixture(scope="module")
def bj():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import boojum_amd
    from boojum_amd import field, fri, merkle, queries, transcript
    boojum_amd.load()
    return type("BJ", (), dict(torch=torch, field=field, fri=fri, merkle=merkle, queries=queries,
                               transcript=transcript, BoojumError=boojum_amd.BoojumError))


def rand(shape, seed, high=O.P):
    return np.random.default_rng(seed).integers(0, high, size=shape, dtype=np.uint64)


def ints(a):
    return [int(v) for v in a]


def view_at(bj, a, off):
    """`a` on the device as a view that starts `off` elements into its buffer."""
    buf = bj.torch.zeros((a.size + off,), dtype=bj.torch.int64, device="cuda")
    buf[off:].copy_(bj.field.to_device(a))
    return buf[off:]


def chain(bj, c0, c1, roots, ci, ch, r):
    d0, d1, _ = bj.fri.interpolate(c0, c1, bj.fri.challenge_powers(ch, r), roots, ci)
    return d0, d1


def sizes(r):
    return [1 << r, 1 << (r + 1), 1 << 11, (3 * 256 + 5) << r]


# ------------------------------------------------------------------ 1. fold_by

@pytest.mark.parametrize("r,n_src", [(r, n) for r in (1, 2, 3) for n in sizes(r)])
def test_fold_by_is_the_chain_and_the_oracle(bj, r, n_src):
    c0, c1 = rand(n_src, 10 + r), rand(n_src, 20 + r)
    log_full = (n_src - 1).bit_length()
    roots_h = O.precompute_twiddles(max(log_full, 1), True)
    roots = bj.field.to_device(roots_h)
    ci, ch = int(O.gl_inv(7)), (int(rand(1, 3)[0]), int(rand(1, 4)[0]))
    w0, w1, cik = c0, c1, ci
    for alpha in bj.fri.challenge_powers(ch, r):
        w0, w1 = O.fri_fold(w0, w1, roots_h, cik, alpha)
        cik = cik * cik % O.P
    assert len(w0) == n_src >> r
    for o0, o1 in OFFSETS:
        v0, v1 = view_at(bj, c0, o0), view_at(bj, c1, o1)
        d0, d1 = bj.fri.fold_by(v0, v1, roots, ci, ch, r)
        g0, g1 = chain(bj, v0, v1, roots, ci, ch, r)
        assert bj.torch.equal(d0, g0) and bj.torch.equal(d1, g1), (o0, o1)
        assert np.array_equal(bj.field.to_host(d0), w0) and np.array_equal(bj.field.to_host(d1), w1), (o0, o1)


@pytest.mark.parametrize("r", [1, 2, 3])
def test_fold_by_is_the_chain_on_any_u64(bj, r):
    """Non-canonical representatives included (the oracle takes canonical values, so chain only);
    the root table at an 8-byte-aligned address as well."""
    n_src = (3 * 256 + 5) << r
    c0, c1 = rand(n_src, 30 + r, high=1 << 64), rand(n_src, 40 + r, high=1 << 64)
    for k, v in enumerate(SPECIALS):
        c0[k], c1[len(SPECIALS) - 1 - k] = v, v          # against each other in the first pairs
        c0[n_src - 1 - k], c1[n_src // 2 + k] = v, v
    table = rand(n_src // 2 + 1, 50 + r, high=1 << 64)
    table[:5] = SPECIALS
    ch = ((1 << 64) - 1, O.P + 5)
    for ci in (O.P, (1 << 64) - 2, int(O.gl_inv(7))):
        for (o0, o1), ro in zip(OFFSETS, (0, 1, 0)):
            roots = view_at(bj, table, 0)[ro:]
            v0, v1 = view_at(bj, c0, o0), view_at(bj, c1, o1)
            d0, d1 = bj.fri.fold_by(v0, v1, roots, ci, ch, r)
            g0, g1 = chain(bj, v0, v1, roots, ci, ch, r)
            assert bj.torch.equal(d0, g0) and bj.torch.equal(d1, g1), (ci, o0, o1, ro)
            assert int(bj.field.to_host(d0).max()) < O.P and int(bj.field.to_host(d1).max()) < O.P


# ------------------------------------------------------------------ 2. the error contract

def test_fold_by_error_contract(bj):
    roots = bj.field.to_device(O.precompute_twiddles(6, True))
    c = bj.field.to_device(rand(64, 1))
    for r, n in ((2, 6), (3, 12), (3, 4), (2, 2)):
        with pytest.raises(bj.BoojumError):
            bj.fri.fold_by(c[:n], c[:n], roots, 3, (1, 2), r)
    for r in (0, 4):
        with pytest.raises(bj.BoojumError):
            bj.fri.fold_by(c, c, roots, 3, (1, 2), r)
    for r in (1, 2, 3):
        d0, d1 = bj.fri.fold_by(c[:0], c[:0], roots, 3, (1, 2), r)
        assert d0.numel() == 0 and d1.numel() == 0
    bj.torch.cuda.synchronize()


# ------------------------------------------------------------------ 3.-6. do_fri

CASES = {
    "by8_4_2": (6, 2, [3, 2, 1], 4),      # the last intermediate tree has size == cap, final degree 1
    "by2_8_8": (10, 1, [1, 3, 3], 16),
    "by8": (6, 2, [3], 4),                # no intermediate oracle
}
_CODEWORDS = {}


def codeword(log_n, log_d):
    """(monomials (2, n), LDE columns (2, D * n)) of a random Ext2 polynomial of degree < n."""
    if (log_n, log_d) not in _CODEWORDS:
        m = rand((2, 1 << log_n), 100 + log_n)
        vals = np.stack([O.bitreverse(O.fft_natural_to_bitreversed(m[k])) for k in range(2)])
        mono, lde = O.lde(vals, log_d)
        assert np.array_equal(mono, m)
        _CODEWORDS[(log_n, log_d)] = (m, lde.reshape(2, -1))     # shared: the tests copy before they change it
    return _CODEWORDS[(log_n, log_d)]


def seeded(cls):
    tr = cls()
    tr.witness_field_elements([5, 6, 7])
    return tr


def tree_sizes(log_n, log_d, schedule):
    out, size = [], 1 << (log_n + log_d)
    for s in schedule:
        out.append(size >> s)
        size >>= s
    return out


@pytest.mark.parametrize("case", sorted(CASES))
def test_do_fri_end_to_end(bj, case):
    log_n, log_d, schedule, cap = CASES[case]
    nl = tree_sizes(log_n, log_d, schedule)
    assert nl[0] > cap and all(x >= cap for x in nl[1:])
    if case == "by8_4_2":
        assert nl[-1] == cap
    m, lde = codeword(log_n, log_d)
    dev = bj.field.to_device(lde)
    tr = seeded(T.Poseidon2Transcript)
    res = bj.fri.do_fri(dev[0].reshape(1 << log_d, -1), dev[1].reshape(1 << log_d, -1), tr, schedule, 1 << log_d, cap)
    assert len(res.leaf_sources_for_intermediate_oracles) == len(schedule)
    assert len(res.intermediate_oracles) == len(schedule) - 1 and len(res.challenges) == len(schedule)
    # leaf sources: the chain of by-2 folds under the drawn challenges
    roots = bj.fri.precompute_roots(lde.shape[1])
    c0, c1, ci = dev[0], dev[1], int(O.gl_inv(7))
    rows = [dev]
    for s, ch, (g0, g1) in zip(schedule, res.challenges, res.leaf_sources_for_intermediate_oracles):
        c0, c1, ci = bj.fri.interpolate(c0, c1, bj.fri.challenge_powers(ch, s), roots, ci)
        assert bj.torch.equal(g0, c0) and bj.torch.equal(g1, c1)
        rows.append(bj.torch.stack([c0, c1]))
    # caps: the trees construct_by_chunking* build over them, and the oracle's
    trees = [res.base_oracle] + list(res.intermediate_oracles)
    caps = []
    for k, (s, t, src) in enumerate(zip(schedule, trees, rows)):
        build = bj.merkle.MerkleTreeWithCap.construct_by_chunking_from_flat_sources if k else \
            bj.merkle.MerkleTreeWithCap.construct_by_chunking
        caps.append(t.get_cap())
        assert t.n_leaves == nl[k] and caps[k].shape == (cap, 4)
        assert np.array_equal(caps[k], build(src, 1 << s, cap).get_cap())
        assert np.array_equal(caps[k], O.merkle_construct_by_chunking(bj.field.to_host(src), 1 << s, cap)[3])
    # challenges: a fresh host transcript fed the caps in order
    replay = seeded(T.Poseidon2Transcript)
    for c, ch in zip(caps, res.challenges):
        replay.witness_merkle_tree_cap(c)
        assert (replay.get_challenge(), replay.get_challenge()) == ch
    # monomials: the closed form from the input monomials
    want = (ints(m[0]), ints(m[1]))
    for s, ch in zip(schedule, res.challenges):
        want = M.fold_monomials_by(want[0], want[1], ch, s)
    assert len(want[0]) == (1 << log_n) >> sum(schedule)
    assert ints(res.monomial_forms[0]) == want[0] and ints(res.monomial_forms[1]) == want[1]
    assert res.low_degree == (True, True)
    # c0 then c1 were witnessed
    replay.witness_field_elements(want[0])
    replay.witness_field_elements(want[1])
    assert tr.get_challenge() == replay.get_challenge()
    # final_monomials on the last fold: the same coefficients, on the device
    f0, f1, low = bj.fri.final_monomials(c0, c1, ci, 1 << log_d)
    assert ints(bj.field.to_host(f0)) == want[0] and ints(bj.field.to_host(f1)) == want[1] and low == (True, True)


def test_do_fri_reports_a_corrupted_codeword(bj):
    log_n, log_d, schedule, cap = CASES["by8_4_2"]
    _, lde = codeword(log_n, log_d)
    bad = lde.copy()
    bad[1, 77] = (int(bad[1, 77]) + 1) % O.P
    # two allocations of their own: do_fri pairs them in a copy
    c0, c1 = bj.field.to_device(bad[0]), bj.field.to_device(bad[1])
    res = bj.fri.do_fri(c0, c1, seeded(T.Poseidon2Transcript), schedule, 1 << log_d, cap)
    assert False in res.low_degree
    good = bj.fri.do_fri(bj.field.to_device(lde[0]), bj.field.to_device(lde[1]), seeded(T.Poseidon2Transcript),
                         schedule, 1 << log_d, cap)
    assert good.low_degree == (True, True)
    assert not np.array_equal(good.base_oracle.get_cap(), res.base_oracle.get_cap())
    assert len(res.monomial_forms[0]) == 1


def test_do_fri_asserts_where_the_reference_does(bj):
    log_n, log_d, _, cap = CASES["by8"]
    _, lde = codeword(log_n, log_d)
    dev = bj.field.to_device(lde)
    for schedule in ([0], [4], [3, 0], [3, 3, 1]):        # the last one: final_degree == 0
        with pytest.raises(ValueError):
            bj.fri.do_fri(dev[0], dev[1], seeded(T.Poseidon2Transcript), schedule, 1 << log_d, cap)


@pytest.mark.parametrize("case", ["by8_4_2", "by2_8_8"])
def test_query_oracles_verify_and_chain(bj, case):
    log_n, log_d, schedule, cap = CASES[case]
    _, lde = codeword(log_n, log_d)
    dev = bj.field.to_device(lde)
    res = bj.fri.do_fri(dev[0], dev[1], seeded(T.Poseidon2Transcript), schedule, 1 << log_d, cap)
    n, full = 1 << log_n, lde.shape[1]
    indices = [0, n - 1, n, full - 1]
    oracles = res.query_oracles(dev[0], dev[1])
    plan = bj.queries.fri_plan(log_n, log_d, schedule)
    assert [(o.elements_per_leaf, o.index_shift, o.n_leaves) for o in oracles] == plan
    out = bj.queries.construct_queries(oracles, indices)
    caps = [res.base_oracle.get_cap()] + [t.get_cap() for t in res.intermediate_oracles]
    for q, index in enumerate(indices):
        for o, c, r in zip(oracles, caps, out):
            assert O.verify_proof_over_cap(r.proof[q], c, O.hash_into_leaf(r.leaf_elements[q]),
                                           index >> o.index_shift), (index, o.index_shift)
        M.chain_check(index, [ints(r.leaf_elements[q]) for r in out], schedule, res.challenges,
                      [ints(f) for f in res.monomial_forms], full)


class StubTranscript:
    """Records what it is given and hands out fixed challenges."""

    def __init__(self):
        self.caps, self.elements, self.drawn = [], [], 0

    def witness_merkle_tree_cap(self, cap):
        self.caps.append(np.array(cap, dtype=np.uint64))

    def witness_field_elements(self, els):
        self.elements.append(ints(els))

    def get_challenge(self):
        self.drawn += 1
        return (0x9E3779B97F4A7C15 * self.drawn) % O.P


def test_do_fri_blake2s_is_the_step_by_step_route(bj):
    log_n, log_d, schedule, cap = CASES["by2_8_8"]
    _, lde = codeword(log_n, log_d)
    dev = bj.field.to_device(lde)
    tr = StubTranscript()
    res = bj.fri.do_fri(dev[0], dev[1], tr, schedule, 1 << log_d, cap, hasher="blake2s")
    ref = StubTranscript()
    roots = bj.fri.precompute_roots(lde.shape[1])
    cur, ci = dev, int(O.gl_inv(7))
    MT = bj.merkle.MerkleTreeWithCap
    for k, s in enumerate(schedule):
        build = MT.construct_by_chunking_from_flat_sources if k else MT.construct_by_chunking
        want_cap = build(cur, 1 << s, cap, hasher="blake2s").get_cap()
        assert np.array_equal(tr.caps[k], want_cap)
        assert not np.array_equal(want_cap, build(cur, 1 << s, cap).get_cap())     # not the Poseidon2 tree
        ch = (ref.get_challenge(), ref.get_challenge())
        assert res.challenges[k] == ch
        c0, c1, ci = bj.fri.interpolate(cur[0], cur[1], bj.fri.challenge_powers(ch, s), roots, ci)
        g0, g1 = res.leaf_sources_for_intermediate_oracles[k]
        assert bj.torch.equal(g0, c0) and bj.torch.equal(g1, c1)
        cur = bj.torch.stack([c0, c1])
    assert len(tr.caps) == len(schedule) and tr.drawn == 2 * len(schedule)
    assert tr.elements == [ints(res.monomial_forms[0]), ints(res.monomial_forms[1])]
    assert res.base_oracle.hasher == "blake2s" and all(t.hasher == "blake2s" for t in res.intermediate_oracles)


# ------------------------------------------------------------------ 7. the transcript

@pytest.mark.parametrize("extra", [0, 1, 7])
def test_poseidon2_transcript_is_the_oracles(bj, extra):
    cap = rand((2, 4), 60 + extra)                       # 8 elements
    els = ints(rand(extra, 70 + extra))
    ours, theirs = bj.transcript.Poseidon2Transcript(), T.Poseidon2Transcript()
    for tr in (ours, theirs):
        tr.witness_merkle_tree_cap(cap)
        tr.witness_field_elements(els)
    # 8 challenges of the finalize, 8 of a second round function, 4 of a third
    a = [ours.get_challenge() for _ in range(20)]
    b = [theirs.get_challenge() for _ in range(20)]
    assert a == b and len(set(a)) == 20 and all(0 <= x < O.P for x in a)
    # the sponge state persists: witness again mid-way through the available challenges
    for tr in (ours, theirs):
        tr.witness_field_elements(els + [9])
    assert [ours.get_challenge() for _ in range(9)] == [theirs.get_challenge() for _ in range(9)]


# ------------------------------------------------------------------ 8. graph capture

def test_fold_by_captures_into_a_graph(bj):
    torch = bj.torch
    r, n_src = 3, 1 << 11
    roots = bj.fri.precompute_roots(n_src)
    ci, ch = int(O.gl_inv(7)), (123456789, 987654321)
    src = bj.field.to_device(rand((2, n_src), 80))
    out = torch.zeros((2, n_src >> r), dtype=torch.int64, device="cuda")

    def calls():
        bj.fri.fold_by(src[0], src[1], roots, ci, ch, r, out=(out[0], out[1]))

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):   # load the kernel before the capture
        calls()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        calls()
    for seed in (81, 82):
        src.copy_(bj.field.to_device(rand((2, n_src), seed)))
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        e0, e1 = bj.fri.fold_by(src[0], src[1], roots, ci, ch, r)
        assert torch.equal(out[0], e0) and torch.equal(out[1], e1)
