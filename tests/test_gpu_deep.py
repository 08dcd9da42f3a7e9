"""GPU DEEP step (boojum_amd/deep.py, csrc/deep.hip) against Python integers and the reference's
own proof, bit-exact: barycentric weights (utils.rs:907-1021), evaluations at z (utils.rs:1085-1200,
prover.rs:1501-1780) and the quotening pass (prover.rs:1823-2050, 2523-2706).

Sizes cover every path of the kernels: evaluate_at has one path per (column tile full / partial,
one / several row ranges, one / several rows per thread) and a row range is at least 1024 rows, so
2^11 x 65 columns reaches all of them; the quotient kernel has an aligned path (window on row
pairs, 16-byte accesses) and a general one (the window 37 + 91), a column loop unrolled by 8 with
a remainder loop (33 = 4 * 8 + 1, 397 = 49 * 8 + 5), and more than one block at 2^10 rows."""
import numpy as np
import pytest

import oracle as O
import transcript as T

import deep_groups

pytestmark = pytest.mark.gpu

P = O.P


@pytest.fixture(scope="module")
def bj():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import boojum_amd
    from boojum_amd import _lib, commit, deep, field
    boojum_amd.load()
    return type("BJ", (), dict(torch=torch, field=field, deep=deep, commit=commit, lib=_lib))


def rng(seed):
    return np.random.default_rng(seed)


def rand(shape, seed):
    return rng(seed).integers(0, P, size=shape, dtype=np.uint64)


def rand_ext(seed):
    a = rand(2, seed)
    return (int(a[0]), int(a[1]))


def bitrev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


def ext_pow(a, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = T.e_mul(r, a)
        a = T.e_mul(a, a)
        e >>= 1
    return r


def points(seed, domain_log, coset=7):
    """An Ext2 point, a base point outside coset * <w_{2^domain_log}>, and 0."""
    base = 3
    assert pow(base * pow(coset, P - 2, P) % P, 1 << domain_log, P) != 1
    return [rand_ext(seed), (base, 0), (0, 0)]


# ------------------------------------------------------------------ 1. weights
@pytest.mark.parametrize("log_n", [0, 1, 2, 6, 11])
def test_weights_match_the_closed_form(bj, log_n):
    n, coset = 1 << log_n, 7
    omega = T.domain_generator(log_n)
    for at in points(100 + log_n, log_n):
        w0, w1 = bj.deep.precompute_for_barycentric_evaluation_in_extension(n, coset, at)
        got = list(zip((int(v) for v in bj.field.to_host(w0)), (int(v) for v in bj.field.to_host(w1))))
        if log_n == 0:
            assert got == [(1, 0)]
            continue
        cn = pow(coset, n, P)
        c = T.e_mul_base(T.e_sub(ext_pow(at, n), (cn, 0)), coset * pow(n * cn % P, P - 2, P) % P)
        want = [None] * n
        wi = 1
        for i in range(n):
            den = T.e_inv(T.e_sub(at, (coset * wi % P, 0)))
            want[bitrev(i, log_n)] = T.e_mul(T.e_mul_base(c, wi), den)
            wi = wi * omega % P
        assert got == want, at
        tot = (0, 0)
        for w in got:
            tot = T.e_add(tot, w)
        assert tot == (1, 0)   # the evaluation of the constant 1


# ------------------------------------------------------------------ 2. evaluate at z
def horner(mono, z):
    r = (0, 0)
    for c in reversed(mono):
        r = T.e_mul(r, z)
        r = ((r[0] + int(c)) % P, r[1])
    return r


@pytest.mark.parametrize("log_n,n_cols", [(1, 1), (6, 3), (11, 65), (14, 2)])
def test_evaluate_at_z_equals_horner_of_the_monomials(bj, log_n, n_cols):
    """Coset 0 of the oracle's LDE, passed inside the whole (C, 4, n) buffer so that a stride
    mistake reads another coset, against Horner evaluation of the oracle's monomials."""
    n = 1 << log_n
    trace = O.synthetic_trace(n_cols, log_n, seed=7 + log_n)
    _, lde = O.lde(trace, 2)
    z = rand_ext(200 + log_n)
    lde_d = bj.field.to_device(lde)
    w = bj.deep.precompute_for_barycentric_evaluation_in_extension(n, 7, z)
    got = bj.deep.barycentric_evaluate_base_at_extension_for_bitreversed(lde_d[:, 0, :], w)
    want = [horner(O.ifft_natural_to_natural(trace[c]), z) for c in range(n_cols)]
    assert got == want


def test_evaluate_extension_columns(bj):
    """An Ext2 polynomial held as (c0, c1) columns is e0 + u e1 of the two base evaluations."""
    log_n = 6
    n = 1 << log_n
    trace = O.synthetic_trace(4, log_n, seed=3)
    _, lde = O.lde(trace, 2)
    z = rand_ext(77)
    lde_d = bj.field.to_device(lde)
    w = bj.deep.precompute_for_barycentric_evaluation_in_extension(n, 7, z)
    got = bj.deep.barycentric_evaluate_extension_at_extension_for_bitreversed(lde_d[0::2, 0, :], lde_d[1::2, 0, :], w)
    mono = [O.ifft_natural_to_natural(trace[c]) for c in range(4)]
    want = []
    for c in (0, 2):
        e0, e1 = horner(mono[c], z), horner(mono[c + 1], z)
        want.append(T.e_add(e0, T.e_mul(e1, (0, 1))))
    assert got == want


# ------------------------------------------------------------------ 3. accumulator bound
@pytest.mark.parametrize("log_n", [16, 20])
def test_evaluate_accumulator_bound(bj, log_n):
    """Every value and both halves of every weight p - 1: each product is 1, the sums n."""
    n = 1 << log_n
    full = bj.torch.full
    cols = full((2, n), -(1 << 32), dtype=bj.torch.int64, device="cuda")   # the bits of p - 1
    assert int(bj.field.to_host(cols[0, :1])[0]) == P - 1
    w = (cols[0], cols[1])
    got = bj.deep.barycentric_evaluate_base_at_extension_for_bitreversed(cols, w)
    assert got == [(n % P, n % P)] * 2


def quotient_reference(storage, entries, at, log_domain, row0, dst0, dst1, accumulate):
    """sum_j ch_j (f_j(x_L) - v_j) / (x_L - at) for every row of the window, from the sources
    themselves (not through the plan), added to dst when accumulating."""
    omega = T.domain_generator(log_domain)
    n_rows = len(dst0)
    out0, out1 = [], []
    for r in range(n_rows):
        x = 7 * pow(omega, bitrev(row0 + r, log_domain), P) % P
        s = (0, 0)
        for col, is_ext, ch, v in entries:
            f = (int(storage[col][r]), int(storage[col + 1][r]) if is_ext else 0)
            s = T.e_add(s, T.e_mul(ch, T.e_sub(f, v)))
        q = T.e_mul(s, T.e_inv(T.e_sub((x, 0), at)))
        if accumulate:
            q = T.e_add(q, (int(dst0[r]), int(dst1[r])))
        out0.append(q[0])
        out1.append(q[1])
    return out0, out1


def run_quotient(bj, storage, entries, at, log_domain, row0, dst0, dst1, accumulate):
    d0, d1 = bj.field.to_device(dst0), bj.field.to_device(dst1)
    st = bj.field.to_device(storage) if storage.shape[0] else None
    bj.deep.quotening_operation_in_extension(d0, d1, st, entries, at, log_domain, row0=row0, accumulate=accumulate)
    return [int(v) for v in bj.field.to_host(d0)], [int(v) for v in bj.field.to_host(d1)]


def test_quotient_accumulator_bound(bj):
    """397 columns of p - 1 with every coefficient (p - 1, p - 1) over 256 rows."""
    log_domain, n_cols = 8, 397
    n = 1 << log_domain
    storage = np.full((n_cols, n), P - 1, dtype=np.uint64)
    entries = [(c, False, (P - 1, P - 1), rand_ext(300 + c) if c == 0 else (0, 0)) for c in range(n_cols)]
    at = rand_ext(299)
    zero = np.zeros(n, dtype=np.uint64)
    got = run_quotient(bj, storage, entries, at, log_domain, 0, zero, zero, False)
    assert got == quotient_reference(storage, entries, at, log_domain, 0, zero, zero, False)


# ------------------------------------------------------------------ 4. quotient
def make_entries(n_cols, seed):
    """Sources over some of the columns (the others keep a zero coefficient): base columns and,
    where two neighbouring columns are free, Ext2 pairs."""
    r = rng(seed)
    entries, c = [], 0
    while c < n_cols:
        kind = int(r.integers(0, 3))   # 0: no source, 1: base, 2: Ext2 pair
        if n_cols == 1:
            kind = 1
        if kind == 2 and c + 1 < n_cols:
            entries.append((c, True, rand_ext(seed * 1000 + c), rand_ext(seed * 2000 + c)))
            c += 2
        else:
            if kind:
                entries.append((c, False, rand_ext(seed * 1000 + c), rand_ext(seed * 2000 + c)))
            c += 1
    return entries


CASES = [(ld, nc, None) for ld in (1, 6, 10) for nc in (0, 1, 5, 33)] + [(10, nc, (37, 91)) for nc in (0, 1, 5, 33)]


@pytest.mark.parametrize("log_domain,n_cols,window", CASES)
def test_quotient_matches_python_integers(bj, log_domain, n_cols, window):
    """Every row of the window, for an Ext2, a base and the zero opening point, overwriting and
    accumulating onto a random dst.  The window 37 + 91 starts and ends off a pair and off a block
    boundary."""
    row0, n_rows = window or (0, 1 << log_domain)
    storage = rand((n_cols, n_rows), 400 + log_domain + n_cols)
    entries = make_entries(n_cols, 7 + n_cols)
    covered = {c + k for c, is_ext, _, _ in entries for k in range(2 if is_ext else 1)}
    assert n_cols < 5 or len(covered) < n_cols   # some coefficients are zero
    for k, at in enumerate(points(500 + log_domain, log_domain)):
        for accumulate in (False, True):
            dst0, dst1 = rand(n_rows, 600 + k), rand(n_rows, 700 + k)
            got = run_quotient(bj, storage, entries, at, log_domain, row0, dst0, dst1, accumulate)
            want = quotient_reference(storage, entries, at, log_domain, row0, dst0, dst1, accumulate)
            assert got == want, (at, accumulate)


def test_quotient_constant_only(bj):
    """n_cols = 0 with a constant: q = -K / (x - at) (the plan of sources that are all constants
    cannot arise in the prover; the C ABI allows it)."""
    log_domain = 6
    n = 1 << log_domain
    k, at = rand_ext(801), rand_ext(802)
    d0 = bj.torch.zeros((n,), dtype=bj.torch.int64, device="cuda")
    d1 = bj.torch.zeros_like(d0)
    bj.lib.call("bj_deep_quotient_d", 0, 0, 0, 0, k[0], k[1], at[0], at[1], log_domain, 0, n, d0.data_ptr(),
                d1.data_ptr(), 0, bj.field.stream_of(d0))
    omega = T.domain_generator(log_domain)
    want = [T.e_mul(T.e_sub((0, 0), k), T.e_inv(T.e_sub((7 * pow(omega, bitrev(r, log_domain), P) % P, 0), at)))
            for r in range(n)]
    got = list(zip((int(v) for v in bj.field.to_host(d0)), (int(v) for v in bj.field.to_host(d1))))
    assert got == want


# ------------------------------------------------------------------ 5. the reference's proof
def test_quotient_reproduces_the_proofs_deep_values(bj):
    """For the 6 queries of proof_fri.json: an 8-row window aligned down from the query index with
    the query's 397 leaf values in its own row (random elsewhere), four accumulating calls with the
    plans of test_deep_cpu's groups; dst at the query's row is the verifier's DEEP value."""
    fx, rep = deep_groups.proof()
    groups, n_cols = deep_groups.opening_groups(fx, rep)
    assert n_cols == 397 and len(groups) == 4 and len(rep["queries"]) == 6
    n_domain = fx["vk"]["domain_size"] * fx["proof_config"]["fri_lde_factor"]
    log_domain = n_domain.bit_length() - 1
    for i, (q, r) in enumerate(zip(fx["queries"], rep["queries"])):
        row0 = r["index"] & ~7
        storage = rand((n_cols, 8), 900 + i)
        storage[:, r["index"] - row0] = np.array(deep_groups.leaf_row(q), dtype=np.uint64)
        st = bj.field.to_device(storage)
        d0 = bj.torch.zeros((8,), dtype=bj.torch.int64, device="cuda")
        d1 = bj.torch.zeros_like(d0)
        for at, entries in groups:
            bj.deep.quotening_operation_in_extension(d0, d1, st, entries, at, log_domain, row0=row0, accumulate=True)
        got = (int(bj.field.to_host(d0)[r["index"] - row0]), int(bj.field.to_host(d1)[r["index"] - row0]))
        assert got == r["deep"], r["index"]


# ------------------------------------------------------------------ 6. the two halves together
def test_evaluations_and_quotening_give_a_low_degree_codeword(bj):
    """A committed 2^8 x 4 trace at D = 4: evaluations at z from coset 0, then quotening over the
    whole 2^10 domain.  sum_c ch_c (f_c(X) - f_c(z)) / (X - z) is a polynomial of degree <= n - 2
    exactly when the values are the evaluations, so the interpolated codeword has no coefficient at
    index >= n - 1 -- and has one as soon as one f(z) is off by one."""
    log_n, log_d, c = 8, 2, 4
    n, domain = 1 << log_n, 1 << (log_n + log_d)
    trace = bj.field.to_device(rand((c, n), 1000))
    ws = bj.commit.witness_commit(trace, 1 << log_d, 16)
    z = rand_ext(1001)
    w = bj.deep.precompute_for_barycentric_evaluation_in_extension(n, 7, z)
    evals = bj.deep.barycentric_evaluate_base_at_extension_for_bitreversed(ws.lde[:, 0, :], w)
    ch = bj.deep.materialize_ext_challenge_powers(rand_ext(1002), c)
    flat = ws.lde.reshape(c, domain)

    def high_coefficients(values):
        d0 = bj.torch.empty((domain,), dtype=bj.torch.int64, device="cuda")
        d1 = bj.torch.empty_like(d0)
        entries = [(j, False, ch[j], values[j]) for j in range(c)]
        bj.deep.quotening_operation_in_extension(d0, d1, flat, entries, z, log_n + log_d, accumulate=False)
        out = []
        for d in (d0, d1):
            mono = O.ifft_natural_to_natural(O.bitreverse(bj.field.to_host(d)), 7)
            out.append(mono[n - 1:])
        return out

    for hi in high_coefficients(evals):
        assert not hi.any()
    wrong = list(evals)
    wrong[2] = ((wrong[2][0] + 1) % P, wrong[2][1])
    assert any(hi.any() for hi in high_coefficients(wrong))


# ------------------------------------------------------------------ 7. argument errors
def test_argument_errors(bj):
    L = bj.lib.load()
    t = bj.torch.zeros((4, 64), dtype=bj.torch.int64, device="cuda")
    st = bj.field.stream_of(t)
    # row0 + n_rows past the domain
    rc = L.bj_deep_quotient_d(t.data_ptr(), 1, 64, t[1].data_ptr(), 0, 0, 1, 0, 6, 1, 64, t[2].data_ptr(),
                              t[3].data_ptr(), 0, st)
    assert rc == -22 and b"row0" in L.bj_last_error()
    # null gammas with n_cols > 0
    rc = L.bj_deep_quotient_d(t.data_ptr(), 1, 64, None, 0, 0, 1, 0, 6, 0, 64, t[2].data_ptr(), t[3].data_ptr(), 0, st)
    assert rc == -22 and b"gammas" in L.bj_last_error()
    # col_stride smaller than the run of rows; log_domain / log_n past the 2-adicity
    rc = L.bj_deep_quotient_d(t.data_ptr(), 2, 32, t[1].data_ptr(), 0, 0, 1, 0, 6, 0, 64, t[2].data_ptr(),
                              t[3].data_ptr(), 0, st)
    assert rc == -22 and L.bj_last_error()
    rc = L.bj_deep_quotient_d(t.data_ptr(), 1, 64, t[1].data_ptr(), 0, 0, 1, 0, 33, 0, 64, t[2].data_ptr(),
                              t[3].data_ptr(), 0, st)
    assert rc == -22 and L.bj_last_error()
    rc = L.bj_evaluate_at_d(t.data_ptr(), 1, 64, 33, t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), st)
    assert rc == -22 and L.bj_last_error()
    rc = L.bj_evaluate_at_d(t.data_ptr(), 2, 32, 6, t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), st)
    assert rc == -22 and L.bj_last_error()
    rc = L.bj_barycentric_weights_d(33, 7, 1, 0, t[0].data_ptr(), t[1].data_ptr(), st)
    assert rc == -22 and L.bj_last_error()
    rc = L.bj_barycentric_weights_d(6, 7, 1, 0, None, t[1].data_ptr(), st)
    assert rc == -22 and L.bj_last_error()
    # n_rows = 0 is a no-op
    assert L.bj_deep_quotient_d(None, 0, 0, None, 0, 0, 1, 0, 6, 64, 0, None, None, 0, st) == 0
    bj.torch.cuda.synchronize()
    assert not t.any()   # nothing was launched
