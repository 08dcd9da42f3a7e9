"""GPU quotient block (boojum_amd/quotient.py, csrc/quotient.hip) against the Python-integer model
(tests/quotient_model.py), every output bit-equal.

The sizes are the smallest that reach each path of the kernels:

* Rows.  The copy-permutation kernel's tile is 512 points per workgroup (256 threads, two points
  each, 256 apart), over q n points; here q = 2 and C = 3 (two relations: one with an intermediate
  as lhs, one with the shifted z).  n = 1: two points, the row after a row is the row itself.
  n = 2: the wrap from row n - 1 to row 0.  2^3: 16 points, a partly filled wave, every thread's
  second point outside.  2^7: 256 points, all first points, no second.  2^8: exactly one tile.
  2^9: two tiles.  2^11: eight tiles.
* Relations, at n = 2^6.  (C, q) = (3, 4): one relation, no intermediates, lhs the shifted z;
  (5, 4): short last chunk; (17, 8): three relations; (35, 2): 18 relations.  A launch holds at
  most 128 columns and 64 relations: (131, 2) at n = 2^4 is 66 relations, two launches, the second
  starting from p_63 with a short last chunk and without the L_1 term; (259, 4) is 65 relations in
  launches of 32, 32 and 1.
* Lookup term: one point per thread, 256 per workgroup: n = 1 (2 points), 2^5 (one partly filled
  workgroup), 2^9 (four workgroups); 1, 4 and 16 sources; with and without f.
* Division: one point per thread; it runs at every size of the end-to-end and graph tests and at
  n = 1, 2^3 and 2^9 on its own.

The LDEs the kernels read are the model's (its own coset LDE), except in the end-to-end test,
where the device computes them."""
import ctypes
import functools

import numpy as np
import pytest

import oracle as O
import quotient_model as Q
import stage2_model as S

pytestmark = pytest.mark.gpu

P = Q.P
BETA, GAMMA = (0x1234567890ABCDEF % P, 0x0FEDCBA987654321), (0xDEADBEEFCAFEF00D % P, 0x1122334455667788)
LK_BETA, LK_GAMMA = (0x0BADC0FFEE0DDF00, 0x7766554433221100), (0x13579BDF02468ACE, 0x0F1E2D3C4B5A6978)


@pytest.fixture(scope="module")
def bj():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import boojum_amd
    from boojum_amd import _lib, commit, field, lde, quotient, stage2
    boojum_amd.load()
    return type("BJ", (), dict(torch=torch, field=field, stage2=stage2, quotient=quotient, commit=commit, lde=lde,
                               lib=_lib))


def rand(shape, seed, high=P):
    return np.random.default_rng(seed).integers(0, high, size=shape, dtype=np.uint64)


def challenges(count, seed):
    return [tuple(int(v) for v in pair) for pair in rand((count, 2), 1000 + seed)]


@functools.lru_cache(maxsize=None)
def case(n_cols, log_n, q, seed=1):
    """Valid inputs and the model's whole block, computed once per shape; nobody writes to them."""
    w, sigma = S.valid_inputs(n_cols, log_n, seed)
    alphas = challenges((n_cols + q - 1) // q + 1, seed)
    r = Q.quotient(w, sigma, BETA, GAMMA, q.bit_length() - 1, alphas)
    assert r.cp.zeros == 0 and r.cp.total == S.ONE
    return w, sigma, alphas, r


def lde_tensor(bj, columns, q):
    """Leaf-order columns (lists of D n values) -> (C, D, n) device tensor."""
    a = np.array(columns, dtype=np.uint64)
    return bj.field.to_device(a.reshape(a.shape[0], q, a.shape[1] // q))


def accumulator(bj, total, start=None):
    if start is None:
        z = bj.torch.zeros((2, total), dtype=bj.torch.int64, device="cuda")
    else:
        z = bj.field.to_device(start)
    return z[0], z[1]


def start_values(total, seed):
    """A seeded random accumulator (standing in for gate terms) as a (2, total) array and as Ext2."""
    a = rand((2, total), seed)
    return a, [(int(a[0][i]), int(a[1][i])) for i in range(total)]


def run_cp(bj, r, alphas, q, start=None):
    d0, d1 = accumulator(bj, len(r.w_lde[0]), start)
    bj.quotient.compute_quotient_terms_in_extension(
        lde_tensor(bj, r.w_lde, q), lde_tensor(bj, r.sigma_lde, q), lde_tensor(bj, S.ext_columns(r.s2_lde), q), BETA,
        GAMMA, alphas, q, d0, d1)
    return np.stack([bj.field.to_host(d0), bj.field.to_host(d1)])


# ------------------------------------------------------------------ 1. rows
@pytest.mark.parametrize("log_n", [0, 1, 3, 7, 8, 9, 11])
def test_row_counts(bj, log_n):
    _, _, alphas, r = case(3, log_n, 2)
    assert np.array_equal(run_cp(bj, r, alphas, 2), Q.acc_columns(r.cp_terms))


# ------------------------------------------------------------------ 2. relations
@pytest.mark.parametrize("n_cols,q,log_n", [(3, 4, 6), (5, 4, 6), (17, 8, 6), (35, 2, 6), (131, 2, 4), (259, 4, 4)])
def test_relations(bj, n_cols, q, log_n):
    _, _, alphas, r = case(n_cols, log_n, q)
    assert len(r.s2) == (n_cols + q - 1) // q
    assert np.array_equal(run_cp(bj, r, alphas, q), Q.acc_columns(r.cp_terms))


# ------------------------------------------------------------------ 3. sources at a higher LDE degree
def test_sources_at_lde_degree_8(bj):
    """Sources LDE'd at 8, q = 2: the column stride is 8 n, the first two cosets are read, and they
    are the 2-LDE (subset_for_degree)."""
    n_cols, log_n, q = 5, 6, 2
    w, sigma, alphas, r = case(n_cols, log_n, q)
    n = 1 << log_n
    w8 = [Q.coset_lde(c, 3) for c in w]
    s8 = [Q.coset_lde(c, 3) for c in sigma]
    z8 = [Q.ext_lde(p, 3) for p in r.s2]
    assert [c[:q * n] for c in w8] == r.w_lde and [p[:q * n] for p in z8] == r.s2_lde
    d0, d1 = accumulator(bj, q * n)
    v = lde_tensor(bj, w8, 8)
    assert v.stride(0) == 8 * n
    bj.quotient.compute_quotient_terms_in_extension(v, lde_tensor(bj, s8, 8), lde_tensor(bj, S.ext_columns(z8), 8),
                                                    BETA, GAMMA, alphas, q, d0, d1)
    assert np.array_equal(np.stack([bj.field.to_host(d0), bj.field.to_host(d1)]), Q.acc_columns(r.cp_terms))


# ------------------------------------------------------------------ 4. the accumulator is added to
def test_a_nonzero_accumulator_is_added_to(bj):
    n_cols, log_n, q = 5, 6, 4
    _, _, alphas, r = case(n_cols, log_n, q)
    a, ext = start_values(q << log_n, 5)
    want = [Q.T.e_add(s, t) for s, t in zip(ext, r.cp_terms)]
    assert np.array_equal(run_cp(bj, r, alphas, q, start=a), Q.acc_columns(want))


# ------------------------------------------------------------------ 5. non-canonical inputs
def test_non_canonical_inputs_give_the_same_output(bj):
    """The kernel is pointwise, so any columns serve: every input drawn below 2^32 - 1 and p added
    to all of them (columns, accumulator, non-residues, challenge limbs that fit)."""
    n_cols, log_n, log_q = 5, 5, 1
    n, q = 1 << log_n, 1 << log_q
    total, m = n * q, 3
    small = 2**32 - 1
    w, sigma = rand((n_cols, total), 1, small), rand((n_cols, total), 2, small)
    s2 = rand((2 * m, total), 3, small)
    start = rand((2, total), 4, small)
    beta, gamma = (BETA[0], 12345), (77, GAMMA[1])
    alphas = [(3, 5), (BETA[1], 9), (11, 13), (17, GAMMA[0])]   # the two large limbs do not fit p more
    pairs = [[(int(s2[2 * t][i]), int(s2[2 * t + 1][i])) for i in range(total)] for t in range(m)]
    terms = Q.copy_permutation_terms(w, sigma, pairs, beta, gamma, alphas, log_n, log_q)
    want = Q.acc_columns([Q.T.e_add((int(start[0][i]), int(start[1][i])), t) for i, t in enumerate(terms)])
    k = S.non_residues_for_copy_permutation(n, n_cols)

    def launch(lift):
        dev = [bj.field.to_device(a + np.uint64(lift)) for a in (w, sigma, s2, start)]
        flat = [v + lift if v <= small else v for pair in alphas for v in pair]
        bj.lib.call("bj_quotient_copy_permutation_d", dev[0].data_ptr(), total, dev[1].data_ptr(), total,
                    dev[2].data_ptr(), total, n_cols, log_n, log_q, (ctypes.c_uint64 * n_cols)(*[v + lift for v in k]),
                    beta[0], beta[1] + lift, gamma[0] + lift, gamma[1], (ctypes.c_uint64 * len(flat))(*flat),
                    dev[3][0].data_ptr(), dev[3][1].data_ptr(), bj.field.stream_of(dev[3]))
        return bj.field.to_host(dev[3])

    assert np.array_equal(launch(0), want)
    assert np.array_equal(launch(P), want)


# ------------------------------------------------------------------ 6. lookup terms
@pytest.mark.parametrize("log_n", [0, 5, 9])
@pytest.mark.parametrize("n_src", [1, 4, 16])
def test_lookup_term(bj, n_src, log_n):
    """With and without f, the sources taken from two tensors (and some >= p), onto a non-zero
    accumulator; pointwise, so random columns serve as LDEs."""
    q = 2
    n, total = 1 << log_n, 2 << log_n
    a, b = rand((n_src // 2 + 1, total), 10 + n_src), rand((n_src, total), 20 + log_n, high=2**64)
    e, f = rand((2, total), 30 + n_src), rand(total, 31 + n_src, high=2**64)
    ad, bd, ed, fd = (lde_tensor(bj, v, q) for v in (a, b, e, f.reshape(1, -1)))
    pick = [(t % 2, t // 2) for t in range(n_src)]   # alternately from a and b
    sources = [(a, b)[w][r] for w, r in pick]
    sources_d = [(ad, bd)[w][r] for w, r in pick]
    g = challenges(n_src, 40)
    alpha = challenges(1, 41 + n_src)[0]
    e_ext = [(int(e[0][i]), int(e[1][i])) for i in range(total)]
    start, start_ext = start_values(total, 50 + log_n)
    for fm, fdev in ((None, None), (f, fd[0])):
        want = [Q.T.e_add(s, t) for s, t in zip(start_ext, Q.lookup_term(e_ext, sources, g, LK_BETA, fm, alpha))]
        d0, d1 = accumulator(bj, total, start)
        bj.quotient.lookup_term(sources_d, g, LK_BETA, (ed[0], ed[1]), alpha, q, d0, d1, f=fdev)
        assert np.array_equal(np.stack([bj.field.to_host(d0), bj.field.to_host(d1)]), Q.acc_columns(want))


@pytest.mark.parametrize("kind", ["variable", "constant"])
def test_lookup_terms_specialized(bj, kind):
    """Both reference variants at width 3 x 2 repetitions, the variables at offset 1, 2^5 rows, q = 2."""
    log_n, q, width, reps = 5, 2, 3, 2
    d = Q.lookup_setup(log_n, width, reps, 60, kind)
    d["beta"], d["gamma"] = LK_BETA, LK_GAMMA
    alphas = challenges(reps + 1, 61)
    r = Q.lookup_block(d, 1, alphas)
    dev = {name: lde_tensor(bj, cols, q) for name, cols in r.lk_lde.items()}
    enc = lde_tensor(bj, S.ext_columns(r.wit_lde + r.mult_lde), q)
    pairs = [(enc[2 * i], enc[2 * i + 1]) for i in range(reps + 1)]
    d0, d1 = accumulator(bj, q << log_n)
    bj.quotient.compute_quotient_terms_for_lookup_specialized(
        dev["variables"], dev["mult"], pairs[:reps], pairs[reps:], dev["constants"], dev["tables"], LK_BETA, LK_GAMMA,
        alphas, d["idxes"], r.per_arg, reps, 1, 1, q, d0, d1)
    assert np.array_equal(np.stack([bj.field.to_host(d0), bj.field.to_host(d1)]), Q.acc_columns(r.lk_terms))


# ------------------------------------------------------------------ 7. division
@pytest.mark.parametrize("log_n,log_q", [(0, 1), (3, 1), (9, 2), (4, 0)])
def test_divide_by_vanishing(bj, log_n, log_q):
    total = 1 << (log_n + log_q)
    a, ext = start_values(total, 70 + log_n)
    d0, d1 = accumulator(bj, total, a)
    bj.quotient.divide_by_vanishing_for_bitreversed_coset_enumeration(d0, d1, log_n)
    want = Q.acc_columns(Q.divide_by_vanishing(ext, log_n, log_q))
    assert np.array_equal(np.stack([bj.field.to_host(d0), bj.field.to_host(d1)]), want)


# ------------------------------------------------------------------ 8. end to end on the device
def test_end_to_end_on_the_device(bj):
    """C = 5, n = 2^8, q = 4, one lookup sub-argument of width 3: stage 2, the LDEs, the terms, the
    division and the monomials all on the device; the chunks, their zero top coefficients and the
    quotient commit's cap against the model; then one altered sigma cell reports "unsatisfied"."""
    n_cols, log_n, q, width = 5, 8, 4, 3
    n = 1 << log_n
    w, sigma = S.valid_inputs(n_cols, log_n, 3)
    d = Q.lookup_setup(log_n, width, 1, 80)
    d["beta"], d["gamma"] = LK_BETA, LK_GAMMA
    m = 2
    ch = challenges(m + 1 + 2, 81)
    r = Q.quotient(w, sigma, BETA, GAMMA, 2, ch[:m + 1], d, ch[m + 1:])
    assert r.cp.total == S.ONE
    to = bj.field.to_device
    lk = {name: to(d[name]) for name in ("variables", "constants", "tables", "mult")}

    def pipeline(sigma_host, check):
        wd, sd = to(w), to(sigma_host)
        st = bj.stage2.second_stage_trace(
            wd, sd, BETA, GAMMA, q, check=check,
            lookup=dict(variables_columns=lk["variables"], multiplicities_columns=lk["mult"],
                        constant_polys=lk["constants"], lookup_tables_columns=lk["tables"], table_id_column_idxes=[],
                        beta=LK_BETA, gamma=LK_GAMMA, variables_offset=1,
                        lookup_parameters=bj.stage2.LookupParameters("variable", width, 1)))
        lde = lambda t: bj.lde.transform_raw_storages_to_lde(t, q)   # noqa: E731
        return bj.quotient.quotient_from_arguments(
            lde(wd), lde(sd), lde(st.trace), BETA, GAMMA, ch, q,
            lookup=dict(variables_lde=lde(lk["variables"]), multiplicities_lde=lde(lk["mult"]),
                        constants_lde=lde(lk["constants"]), tables_lde=lde(lk["tables"]), beta=LK_BETA, gamma=LK_GAMMA,
                        table_id_column_idxes=[], column_elements_per_subargument=width + 1, num_subarguments=1,
                        variables_offset=1))

    chunks, top_is_zero = pipeline(sigma, True)
    got = bj.field.to_host(chunks)
    assert got.shape == (2 * q, n)
    assert np.array_equal(got, r.chunks)
    assert top_is_zero == (True, True)
    assert not got[-2:, -q:].any() and got.any()
    oc = bj.commit.quotient_commit(chunks, 2, 4)
    cosets = O.lde_cosets(log_n, 1)
    l_ref = np.stack([np.stack([O.fft_natural_to_bitreversed(r.chunks[i].copy(), int(s)) for s in cosets])
                      for i in range(2 * q)])
    cap_ref = O.merkle_construct(l_ref.reshape(2 * q, 2 * n), 4)[3]
    assert np.array_equal(np.asarray(oc.get_cap(), dtype=np.uint64), np.asarray(cap_ref, dtype=np.uint64))

    bad = sigma.copy()
    bad[3, 100] = (int(bad[3, 100]) + 1) % P
    rb = Q.quotient(w, bad, BETA, GAMMA, 2, ch[:m + 1], d, ch[m + 1:])
    assert rb.mono[0][-1] != 0 and rb.mono[1][-1] != 0
    chunks, top_is_zero = pipeline(bad, False)
    assert top_is_zero == (False, False)
    assert np.array_equal(bj.field.to_host(chunks), rb.chunks)


# ------------------------------------------------------------------ 9. graph capture
def test_the_three_calls_capture_into_one_graph(bj):
    """Copy-permutation terms, one lookup term and the division captured into one HIP graph (nothing
    allocated, no synchronisation); a replay on other contents of the same buffers gives the model's
    divided accumulator for them."""
    torch = bj.torch
    n_cols, log_n, q = 5, 6, 4
    total = q << log_n
    runs = []
    for seed in (1, 2):
        _, _, alphas, r = case(n_cols, log_n, q, seed)
        runs.append((r, alphas))
    alphas = runs[0][1]
    assert runs[1][1] != alphas
    src, e, f = rand((2, total), 90), rand((2, total), 91), rand((1, total), 92)
    g, lk_alpha = challenges(2, 93), challenges(1, 94)[0]
    e_ext = [(int(e[0][i]), int(e[1][i])) for i in range(total)]

    def want(r, a):
        # the captured challenges are the first run's: the second run's columns go through them too
        terms = Q.copy_permutation_terms(r.w_lde, r.sigma_lde, r.s2_lde, BETA, GAMMA, a, log_n, 2)
        lk = Q.lookup_term(e_ext, list(src), g, LK_BETA, f[0], lk_alpha)
        acc = [Q.T.e_add(s, t) for s, t in zip(terms, lk)]
        return Q.acc_columns(Q.divide_by_vanishing(acc, log_n, 2))

    r0 = runs[0][0]
    v, s, z = (lde_tensor(bj, c, q) for c in (r0.w_lde, r0.sigma_lde, S.ext_columns(r0.s2_lde)))
    sd, ed, fd = (lde_tensor(bj, c, q) for c in (src, e, f))
    dst = torch.zeros((2, total), dtype=torch.int64, device="cuda")

    def calls():
        bj.quotient.compute_quotient_terms_in_extension(v, s, z, BETA, GAMMA, alphas, q, dst[0], dst[1])
        bj.quotient.lookup_term([sd[0], sd[1]], g, LK_BETA, (ed[0], ed[1]), lk_alpha, q, dst[0], dst[1], f=fd[0])
        bj.quotient.divide_by_vanishing_for_bitreversed_coset_enumeration(dst[0], dst[1], log_n)

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):   # load the kernels before the capture
        calls()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        calls()
    for r, _ in runs:
        for t, cols in ((v, r.w_lde), (s, r.sigma_lde), (z, S.ext_columns(r.s2_lde))):
            t.copy_(lde_tensor(bj, cols, q))
        dst.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bj.field.to_host(dst), want(r, alphas))
