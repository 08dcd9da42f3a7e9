"""The quotient block without a GPU: the model (tests/quotient_model.py) against the verifier's
equation at a point off the domain, the degree bound of its quotient, the host entry point
bj_vanishing_inverses_h against the model, and the argument checks of the three device entry
points that are made before any device work."""
import ctypes
import functools

import pytest

import transcript as T

import quotient_model as Q
import stage2_model as S

P = Q.P
BETA, GAMMA = (0x1234567890ABCDEF % P, 0x0FEDCBA987654321), (0xDEADBEEFCAFEF00D % P, 0x1122334455667788)
LK_BETA, LK_GAMMA = (0x0BADC0FFEE0DDF00, 0x7766554433221100), (0x13579BDF02468ACE, 0x0F1E2D3C4B5A6978)
AT = (0x0123456789ABCDEF, 0x0FEDCBA987654321 % P)   # the point off the domain
SHAPES = [(5, 3, 4), (17, 4, 8)]


def challenges(count, seed):
    """Fixed Ext2 challenges."""
    out, v = [], (seed * 0x9E3779B97F4A7C15 + 1) % P
    for _ in range(count):
        a = v
        v = (v * 6364136223846793005 + 1442695040888963407) % P
        out.append((a, v))
        v = (v * 6364136223846793005 + 1442695040888963407) % P
    return out


@functools.lru_cache(maxsize=None)
def case(n_cols, log_n, q, with_lookup):
    w, sigma = S.valid_inputs(n_cols, log_n, seed=21)
    m = (n_cols + q - 1) // q
    lookup = lookup_challenges = None
    if with_lookup:
        lookup = Q.lookup_setup(log_n, 3, 1, seed=31)
        lookup["beta"], lookup["gamma"] = LK_BETA, LK_GAMMA
        lookup_challenges = challenges(2, 8)
    alphas = challenges(m + 1, 7)
    r = Q.quotient(w, sigma, BETA, GAMMA, q.bit_length() - 1, alphas, lookup, lookup_challenges)
    assert r.cp.zeros == 0 and r.cp.total == S.ONE
    return w, sigma, alphas, lookup, lookup_challenges, r


def base_at(col, at):
    return Q.horner(Q.monomials(col), at)


def ext_at(poly, at):
    return Q.horner_ext(Q.monomials([v[0] for v in poly]), Q.monomials([v[1] for v in poly]), at)


def quotient_times_vanishing_at(r, at):
    """q(at) (at^n - 1) with q(at) = sum_i at^(i n) chunk_i(at), the chunks as committed."""
    n = 1 << r.log_n
    total, step, power = Q.ZERO, Q.e_pow(at, n), Q.ONE
    for i in range(1 << r.log_q):
        c0, c1 = [int(v) for v in r.chunks[2 * i]], [int(v) for v in r.chunks[2 * i + 1]]
        total = T.e_add(total, T.e_mul(power, Q.horner_ext(c0, c1, at)))
        power = T.e_mul(power, step)
    return T.e_mul(total, T.e_sub(step, Q.ONE))


@pytest.mark.parametrize("with_lookup", [False, True])
@pytest.mark.parametrize("n_cols,log_n,q", SHAPES)
def test_identity_at_a_point_off_the_domain(n_cols, log_n, q, with_lookup):
    """Every input polynomial evaluated at AT from its monomials by Horner: the sum of the terms
    there is q(AT) (AT^n - 1).  This is the equation the verifier checks, so it pins the model's
    terms, division, interpolation and chunk order to it and not to themselves."""
    w, sigma, alphas, lookup, lookup_challenges, r = case(n_cols, log_n, q, with_lookup)
    n = 1 << log_n
    assert Q.e_pow(AT, n) != Q.ONE
    omega = T.domain_generator(log_n)
    k = S.non_residues_for_copy_permutation(n, n_cols)
    total = Q.copy_permutation_terms_at(
        AT, [base_at(c, AT) for c in w], [base_at(c, AT) for c in sigma], ext_at(r.cp.z, AT),
        ext_at(r.cp.z, T.e_mul_base(AT, omega)), [ext_at(p, AT) for p in r.cp.intermediates], BETA, GAMMA, alphas, q,
        k, n)
    if with_lookup:
        powers = S.gamma_powers(LK_GAMMA, 4)
        srcs = [base_at(lookup["variables"][1 + t], AT) for t in range(4)]
        total = T.e_add(total, Q.lookup_term_at(ext_at(r.wit[0], AT), srcs, powers, LK_BETA, Q.ONE,
                                                lookup_challenges[0]))
        tables = [base_at(c, AT) for c in lookup["tables"]]
        total = T.e_add(total, Q.lookup_term_at(ext_at(r.mult[0], AT), tables, powers, LK_BETA,
                                                base_at(lookup["mult"][0], AT), lookup_challenges[1]))
    assert total == quotient_times_vanishing_at(r, AT)


@pytest.mark.parametrize("with_lookup", [False, True])
@pytest.mark.parametrize("n_cols,log_n,q", SHAPES)
def test_top_coefficients_are_zero(n_cols, log_n, q, with_lookup):
    """The quotient's degree is at most q n - q - 1: the last q coefficients of both halves."""
    r = case(n_cols, log_n, q, with_lookup)[-1]
    c0, c1 = r.mono
    assert len(c0) == len(c1) == q << log_n
    assert c0[-q:] == [0] * q and c1[-q:] == [0] * q
    assert any(c0) and any(c1)


def test_an_altered_sigma_shows_in_the_last_coefficient():
    """One sigma cell altered (fixed seed and cell): the terms no longer vanish on the domain, and
    the last coefficient of both halves, which the reference asserts on (prover.rs:1424-1439), is
    non-zero for this seed."""
    n_cols, log_n, q = 5, 3, 4
    w, sigma, alphas = case(n_cols, log_n, q, False)[:3]
    bad = sigma.copy()
    bad[3, 5] = (int(bad[3, 5]) + 1) % P
    r = Q.quotient(w, bad, BETA, GAMMA, 2, alphas)
    assert r.cp.total != S.ONE
    assert r.mono[0][-1] != 0 and r.mono[1][-1] != 0


@pytest.mark.parametrize("log_q", [0, 1, 3])
@pytest.mark.parametrize("log_n", [0, 3, 10, 20])
def test_bj_vanishing_inverses_h_equals_the_model(log_n, log_q):
    from boojum_amd import quotient
    got = quotient.vanishing_inverses(log_n, log_q)
    assert got == Q.vanishing_inverses(log_n, log_q)
    # and the definition: the inverse of x^n - 1 at a point of each coset
    if log_n <= 3:
        n, xs = 1 << log_n, Q.lde_points(log_n, log_q)
        for i, v in enumerate(got):
            assert v * (pow(xs[i * n], n, P) - 1) % P == 1


def test_argument_errors_before_any_device_work():
    """Every rejected call returns BJ_EINVAL from the checks at the top of the entry point, so it
    needs no device: the pointers are never followed."""
    from boojum_amd import _lib
    L = _lib.load()
    fake = 0x1000   # a non-null "device pointer"
    k = (ctypes.c_uint64 * 4)(1, 7, 11, 13)
    a = (ctypes.c_uint64 * 6)()

    def cp(vars_=fake, vs=32, sig=fake, ss=32, s2=fake, zs=32, n_cols=4, log_n=4, log_q=1, nr=k, alphas=a, d0=fake,
           d1=fake):
        return L.bj_quotient_copy_permutation_d(vars_, vs, sig, ss, s2, zs, n_cols, log_n, log_q, nr, 1, 2, 3, 4,
                                                alphas, d0, d1, None)

    for kwargs, word in [(dict(n_cols=0), b"n_cols"), (dict(vs=31), b"stride"), (dict(ss=31), b"stride"),
                         (dict(zs=31), b"stride"), (dict(vars_=None), b"null"), (dict(sig=None), b"null"),
                         (dict(s2=None), b"null"), (dict(nr=None), b"null"), (dict(alphas=None), b"null"),
                         (dict(d0=None), b"null"), (dict(d1=None), b"null"), (dict(log_n=32), b"2-adicity"),
                         (dict(log_n=33, log_q=0), b"2-adicity"), (dict(log_n=4, log_q=8), b"BJ_QUOTIENT_MAX_DEGREE")]:
        assert cp(**kwargs) == -22, kwargs
        assert word in L.bj_last_error(), (kwargs, L.bj_last_error())

    srcs = (ctypes.c_void_p * 17)(*([fake] * 17))
    g = (ctypes.c_uint64 * 34)()

    def lk(srcs_=srcs, n_src=2, g_=g, e0=fake, e1=fake, log_n=4, log_q=1, d0=fake, d1=fake):
        return L.bj_quotient_lookup_term_d(srcs_, n_src, g_, 1, 2, e0, e1, None, 3, 4, log_n, log_q, d0, d1, None)

    for kwargs, word in [(dict(n_src=0), b"n_src"), (dict(n_src=17), b"n_src"), (dict(srcs_=None), b"null"),
                         (dict(g_=None), b"null"), (dict(e0=None), b"null"), (dict(e1=None), b"null"),
                         (dict(d0=None), b"null"), (dict(d1=None), b"null"), (dict(log_n=32), b"2-adicity"),
                         (dict(log_q=8), b"BJ_QUOTIENT_MAX_DEGREE")]:
        assert lk(**kwargs) == -22, kwargs
        assert word in L.bj_last_error(), (kwargs, L.bj_last_error())
    holed = (ctypes.c_void_p * 2)(fake, None)
    assert lk(srcs_=holed) == -22 and b"null source" in L.bj_last_error()

    def dv(d0=fake, d1=fake, log_n=4, log_q=1):
        return L.bj_quotient_divide_vanishing_d(d0, d1, log_n, log_q, None)

    for kwargs, word in [(dict(d0=None), b"null"), (dict(d1=None), b"null"), (dict(log_n=32), b"2-adicity"),
                         (dict(log_q=8), b"BJ_QUOTIENT_MAX_DEGREE")]:
        assert dv(**kwargs) == -22, kwargs
        assert word in L.bj_last_error(), (kwargs, L.bj_last_error())

    out = (ctypes.c_uint64 * 2)()
    assert L.bj_vanishing_inverses_h(32, 1, out) == -22
    assert L.bj_vanishing_inverses_h(4, 1, None) == -22
