"""The FRI commit-phase model (tests/fri_model.py) against the oracle, without a GPU: the by-2 fold,
the per-output r-step fold, the monomial closed form, and the verifier-side chain check over the
model's own do_fri with the oracle's Poseidon2 transcript."""
import numpy as np
import pytest

import oracle as O
import transcript as T

import fri_model as M

LOG_N, LOG_D, SCHEDULE, CAP = 6, 2, [3, 2, 1], 4


def rand(shape, seed):
    return np.random.default_rng(seed).integers(0, O.P, size=shape, dtype=np.uint64)


def ints(a):
    return [int(v) for v in a]


@pytest.fixture(scope="module")
def codeword():
    """Monomials of a random Ext2 polynomial of degree < n and its coset LDE, flat."""
    m = rand((2, 1 << LOG_N), 11)
    # the oracle's LDE takes the values over the natural domain, so go through them
    vals = np.stack([O.fft_natural_to_bitreversed(m[k]) for k in range(2)])
    vals = np.stack([O.bitreverse(vals[k]) for k in range(2)])
    got_mono, lde = O.lde(vals, LOG_D)
    assert np.array_equal(got_mono, m)
    return ints(m[0]), ints(m[1]), ints(lde[0].reshape(-1)), ints(lde[1].reshape(-1))


def cap_of(rows, elements_per_leaf, cap_size):
    src = np.array(rows, dtype=np.uint64)
    return O.merkle_construct_by_chunking(src, elements_per_leaf, cap_size)[3]


def test_model_constants_are_the_oracles():
    for log_n in (1, 5, 8):
        assert M.domain_generator(log_n) == int(O.domain_generator(log_n))
        assert M.inverse_roots(1 << log_n) == ints(O.precompute_twiddles(log_n, True))


@pytest.mark.parametrize("log_n", [1, 4, 7])
def test_fold_by_2_is_the_oracles(log_n):
    n = 1 << log_n
    c0, c1 = rand(n, 1), rand(n, 2)
    roots = O.precompute_twiddles(log_n, True)
    ci, ch = int(O.gl_inv(7)), (int(rand(1, 3)[0]), int(rand(1, 4)[0]))
    w0, w1 = O.fri_fold(c0, c1, roots, ci, ch)
    d0, d1 = M.fold_multiple(ints(c0), ints(c1), ints(roots), ci, ch)
    assert d0 == ints(w0) and d1 == ints(w1)


@pytest.mark.parametrize("r", [1, 2, 3])
def test_r_step_fold_is_r_folds(r):
    n = 5 << r
    c0, c1 = ints(rand(n, 5)), ints(rand(n, 6))
    roots = ints(rand(n // 2, 7))      # any table: the indexing is what is checked
    ci, ch = 123456789, (int(rand(1, 8)[0]), int(rand(1, 9)[0]))
    w0, w1, cik = c0, c1, ci
    for alpha in M.challenge_powers(ch, r):
        w0, w1 = M.fold_multiple(w0, w1, roots, cik, alpha)
        cik = cik * cik % M.P
    assert M.fold_by(c0, c1, roots, ci, ch, r) == (w0, w1)


def test_closed_form_is_the_interpolation_of_the_folded_lde(codeword):
    m0, m1, c0, c1 = codeword
    roots = M.inverse_roots(len(c0))
    ci = M.inv(M.GEN)
    for k, s in enumerate(SCHEDULE):
        ch = (int(rand(1, 20 + k)[0]), int(rand(1, 30 + k)[0]))
        c0, c1 = M.fold_by(c0, c1, roots, ci, ch, s)
        m0, m1 = M.fold_monomials_by(m0, m1, ch, s)
        ci = pow(ci, 1 << s, M.P)
        for half, want in ((c0, m0), (c1, m1)):
            got = ints(O.ifft_natural_to_natural(O.bitreverse(np.array(half, dtype=np.uint64)), M.inv(ci)))
            assert got[:len(want)] == want
            assert len(got) == len(want) << LOG_D and not any(got[len(want):])
            assert M.interpolate_bitreversed(half, M.inv(ci)) == got
    assert len(m0) == 1


def run_model(c0, c1):
    tr = T.Poseidon2Transcript()
    tr.witness_field_elements([1, 2, 3])
    return M.do_fri(c0, c1, tr, SCHEDULE, 1 << LOG_D, CAP, cap_of), tr


def leaves_at(c0, c1, res, index):
    rows = [(c0, c1)] + res["leaf_sources"][:-1]
    out, shift = [], 0
    for s, r in zip(SCHEDULE, rows):
        shift += s
        out.append(M.leaf_of(r, 1 << s, index >> shift))
    return out


def test_chain_check_passes_on_the_models_do_fri(codeword):
    m0, m1, c0, c1 = codeword
    res, tr = run_model(c0, c1)
    assert res["low_degree"] == (True, True)
    assert len(res["caps"]) == 3 and all(len(c) == CAP for c in res["caps"])
    want = (m0, m1)
    for ch, s in zip(res["challenges"], SCHEDULE):
        want = M.fold_monomials_by(want[0], want[1], ch, s)
    assert res["monomial_forms"] == [want[0], want[1]]
    # the transcript saw cap, cap, cap, m0, m1 in this order
    replay = T.Poseidon2Transcript()
    replay.witness_field_elements([1, 2, 3])
    for cap, ch in zip(res["caps"], res["challenges"]):
        replay.witness_merkle_tree_cap(cap)
        assert (replay.get_challenge(), replay.get_challenge()) == ch
    replay.witness_field_elements(res["monomial_forms"][0])
    replay.witness_field_elements(res["monomial_forms"][1])
    assert replay.get_challenge() == tr.get_challenge()
    full = len(c0)
    for index in (0, 1, (1 << LOG_N) - 1, 1 << LOG_N, full - 1, 77):
        M.chain_check(index, leaves_at(c0, c1, res, index), SCHEDULE, res["challenges"], res["monomial_forms"], full)


def test_chain_check_fails_on_a_corrupted_codeword(codeword):
    _, _, c0, c1 = codeword
    bad = list(c0)
    bad[77] = (bad[77] + 1) % M.P
    res, _ = run_model(bad, c1)
    assert res["low_degree"] != (True, True)
    with pytest.raises(AssertionError):
        M.chain_check(77, leaves_at(bad, c1, res, 77), SCHEDULE, res["challenges"], res["monomial_forms"], len(c0))
    # a leaf that is not the committed one breaks the chain between two oracles
    res, _ = run_model(c0, c1)
    leaves = leaves_at(c0, c1, res, 77)
    leaves[1][0] = (leaves[1][0] + 1) % M.P
    with pytest.raises(AssertionError, match="does not hold the fold"):
        M.chain_check(77, leaves, SCHEDULE, res["challenges"], res["monomial_forms"], len(c0))
