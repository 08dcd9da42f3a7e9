"""Stage 2 without a GPU: the model (tests/stage2_model.py) against the reference's definitions
(copy_permutation.rs:14-28, 425-522, 649-774; utils.rs:636-688), the host entry point
bj_non_residues_h against the model, and the argument checks of the two device entry points that
are made before any device work."""
import ctypes

import numpy as np
import pytest

import transcript as T

import stage2_model as M

P = M.P
BETA, GAMMA = (0x1234567890ABCDEF % P, 0x0FEDCBA987654321), (0xDEADBEEFCAFEF00D % P, 0x1122334455667788)


@pytest.fixture(scope="module")
def valid():
    """(C, q) = (5, 2): three chunks, the last one short, over 2^5 rows."""
    w, sigma = M.valid_inputs(5, 5, seed=11)
    return w, sigma, M.copy_permutation(w, sigma, BETA, GAMMA, 2)


def test_z_is_the_exclusive_prefix_product(valid):
    _, _, cp = valid
    assert cp.z[0] == M.ONE
    for i in range(len(cp.z) - 1):
        assert cp.z[i + 1] == T.e_mul(cp.z[i], cp.a[i])
    assert cp.zeros == 0


def test_partial_product_relations(valid):
    """p_0 den_0 = z num_0, p_j den_j = p_{j-1} num_j, z[i+1] den_{m-1} = p_{m-2} num_{m-1}: the
    relations the quotient checks per row (copy_permutation.rs:740-745)."""
    _, _, cp = valid
    m, n = len(cp.num), len(cp.z)
    assert m == 3 and len(cp.intermediates) == m - 1
    for i in range(n):
        prev = cp.z[i]
        for j in range(m - 1):
            assert T.e_mul(cp.intermediates[j][i], cp.den[j][i]) == T.e_mul(prev, cp.num[j][i])
            prev = cp.intermediates[j][i]
        nxt = cp.z[i + 1] if i + 1 < n else cp.total
        assert T.e_mul(nxt, cp.den[m - 1][i]) == T.e_mul(prev, cp.num[m - 1][i])


def test_total_product_is_one_exactly_on_valid_inputs(valid):
    w, sigma, cp = valid
    assert cp.total == M.ONE
    bad = sigma.copy()
    bad[3, 17] = (int(bad[3, 17]) + 1) % P
    assert M.copy_permutation(w, bad, BETA, GAMMA, 2).total != M.ONE


def test_one_chunk_has_no_intermediates():
    w, sigma = M.valid_inputs(3, 3, seed=5)
    cp = M.copy_permutation(w, sigma, BETA, GAMMA, 4)
    assert cp.intermediates == [] and cp.total == M.ONE


def test_zero_denominator_counts_and_gives_zero():
    """beta, gamma in the base field make w = -(beta sigma + gamma) reachable."""
    w, sigma = M.valid_inputs(3, 3, seed=6)
    beta, gamma = (BETA[0], 0), (GAMMA[0], 0)
    w = w.copy()
    w[1, 4] = (P - (beta[0] * int(sigma[1, 4]) + gamma[0]) % P) % P
    cp = M.copy_permutation(w, sigma, beta, gamma, 2)
    assert cp.zeros == 1 and cp.a[4] == M.ZERO and cp.total == M.ZERO


@pytest.mark.parametrize("log_n", [4, 20])
def test_non_residues_are_in_distinct_cosets_outside_the_domain(log_n):
    n = 1 << log_n
    k = M.non_residues_for_copy_permutation(n, 130)
    assert k[0] == 1 and len(k) == 130
    powers = [pow(v, n, P) for v in k]
    assert powers[0] == 1 and 1 not in powers[1:]      # k_c outside the domain (k_0 = 1 is the domain itself)
    assert len(set(powers)) == len(powers)             # k_a / k_b outside the domain for every pair
    assert all(pow(v, (P - 1) // 2, P) == P - 1 for v in k[1:])


@pytest.mark.parametrize("log_n,num", [(4, 130), (20, 130), (0, 3), (10, 1)])
def test_bj_non_residues_h_equals_the_model(log_n, num):
    from boojum_amd import stage2
    assert stage2.non_residues_for_copy_permutation(1 << log_n, num) == \
        M.non_residues_for_copy_permutation(1 << log_n, num)


def test_num_intermediate_partial_product_relations():
    from boojum_amd import stage2
    for f in (stage2.num_intermediate_partial_product_relations, M.num_intermediate_partial_product_relations):
        assert f(130, 8) == 16
        assert f(8, 8) == 0
        assert f(9, 8) == 1


def test_argument_errors_before_any_device_work():
    """Every rejected call returns BJ_EINVAL from the checks at the top of the entry point, so it
    needs no device: the pointers are never followed."""
    from boojum_amd import _lib
    L = _lib.load()
    fake = 0x1000   # a non-null "device pointer"
    k = (ctypes.c_uint64 * 4)(1, 7, 11, 13)

    def cp(vars_=fake, vs=16, sig=fake, ss=16, n_cols=4, log_n=4, nr=k, chunk=2, out=fake, os_=16, status=fake):
        return L.bj_copy_permutation_d(vars_, vs, sig, ss, n_cols, log_n, nr, 1, 2, 3, 4, chunk, out, os_, status, None)

    for kwargs, word in [(dict(n_cols=0), b"n_cols"), (dict(chunk=0), b"power of two"), (dict(chunk=3), b"power of two"),
                         (dict(chunk=6), b"power of two"), (dict(vs=15), b"stride"), (dict(ss=15), b"stride"),
                         (dict(os_=15), b"stride"), (dict(vars_=None), b"null"), (dict(sig=None), b"null"),
                         (dict(nr=None), b"null"), (dict(out=None), b"null"), (dict(status=None), b"null"),
                         (dict(log_n=33), b"2-adicity")]:
        assert cp(**kwargs) == -22, kwargs
        assert word in L.bj_last_error(), (kwargs, L.bj_last_error())

    srcs = (ctypes.c_void_p * 17)(*([fake] * 17))
    g = (ctypes.c_uint64 * 34)()

    def lk(srcs_=srcs, n_src=2, g_=g, log_n=4, o0=fake, o1=fake, status=fake):
        return L.bj_lookup_encoding_d(srcs_, n_src, g_, 1, 2, None, log_n, o0, o1, status, None)

    for kwargs, word in [(dict(n_src=0), b"n_src"), (dict(n_src=17), b"n_src"), (dict(srcs_=None), b"null"),
                         (dict(g_=None), b"null"), (dict(o0=None), b"null"), (dict(o1=None), b"null"),
                         (dict(status=None), b"null"), (dict(log_n=33), b"2-adicity")]:
        assert lk(**kwargs) == -22, kwargs
        assert word in L.bj_last_error(), (kwargs, L.bj_last_error())
    holed = (ctypes.c_void_p * 2)(fake, None)
    assert lk(srcs_=holed) == -22 and b"null source" in L.bj_last_error()

    out = (ctypes.c_uint64 * 2)()
    assert L.bj_non_residues_h(0, 4, out) == -22
    assert L.bj_non_residues_h(2, 33, out) == -22
    assert L.bj_non_residues_h(2, 4, None) == -22


def test_lookup_model_is_the_definition():
    """A_s (beta + sum gamma^t col) = 1 and B (beta + sum gamma^t table) = mult, both variants."""
    rng = np.random.default_rng(3)
    n, width, reps = 8, 3, 2
    variables = rng.integers(0, P, size=(1 + (width + 1) * reps, n), dtype=np.uint64)
    constants = rng.integers(0, 5, size=(2, n), dtype=np.uint64)
    tables = rng.integers(0, P, size=(width + 1, n), dtype=np.uint64)
    mult = rng.integers(0, 9, size=(1, n), dtype=np.uint64)
    powers = M.gamma_powers(GAMMA, width + 1)
    for kind, idxes in (("variable", []), ("constant", [1])):
        wit, mu, zeros = M.lookup_poly_pairs_specialized(variables, mult, constants, tables, idxes, BETA, GAMMA, 1,
                                                         kind, width, reps)
        assert zeros == 0 and len(wit) == reps and len(mu) == 1
        per = width + 1 if kind == "variable" else width
        for s in range(reps):
            cols = [variables[1 + s * per + t] for t in range(per)] + ([constants[1]] if kind == "constant" else [])
            for i in range(n):
                d = BETA
                for t, col in enumerate(cols):
                    d = T.e_add(d, T.e_mul_base(powers[t], int(col[i])))
                assert T.e_mul(wit[s][i], d) == M.ONE
        for i in range(n):
            d = BETA
            for t in range(width + 1):
                d = T.e_add(d, T.e_mul_base(powers[t], int(tables[t][i])))
            assert T.e_mul(mu[0][i], d) == (int(mult[0][i]), 0)
