"""GPU stage 2 (boojum_amd/stage2.py, csrc/stage2.hip) against the Python-integer model
(tests/stage2_model.py), every output bit-equal.

The sizes are the smallest that reach each path of the kernels:

* Scan.  The rational pass scans a tile of 128 rows per workgroup (two waves), one workgroup turns
  the tile totals into their prefix (a thread owns a run of ceil(tiles / 256) consecutive tiles,
  256 threads = four waves), the apply pass multiplies the two.  n = 1 and 2: one partly filled
  wave, z[0] = 1 alone.  2^6: one wave of one tile.  2^7: a whole tile, both waves.  2^8: exactly
  two tiles.  2^13: 64 tiles, the totals in one wave.  2^14: 128 tiles, two waves of the totals
  workgroup.  2^16: 512 tiles, so the totals exceed the workgroup's 256 threads and a thread walks
  a run of two.
* Chunking.  (C, q) = (3, 4): one chunk, no intermediates; (5, 4): short last chunk; (17, 8): three
  chunks; (4, 1): a chunk per column; (8, 8).  (35, 2): 18 chunks, more than the 16 that share one
  inversion, so two groups of nine.  (259, 4): more than the 256 columns of one rational launch,
  the launches meeting on a chunk boundary; (600, 512): three launches that split chunk 0 and meet
  chunk 1 on its boundary; (300, 512): one chunk split over two launches.
* Lookup.  A workgroup's tile is 1024 rows, four per thread: n = 1 and 2^5 (rows 1..3 of every
  thread outside), 2^9 (rows 2, 3 outside), 2^11 (two tiles); 1, 4 and 16 sources.

No input holds a zero denominator unless one is planted: the model counts them for every case."""
import ctypes
import functools

import numpy as np
import pytest

import stage2_model as M

pytestmark = pytest.mark.gpu

P = M.P
BETA, GAMMA = (0x1234567890ABCDEF % P, 0x0FEDCBA987654321), (0xDEADBEEFCAFEF00D % P, 0x1122334455667788)


@pytest.fixture(scope="module")
def bj():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import boojum_amd
    from boojum_amd import _lib, commit, field, stage2
    boojum_amd.load()
    return type("BJ", (), dict(torch=torch, field=field, stage2=stage2, commit=commit, lib=_lib,
                               Error=boojum_amd.BoojumError))


@functools.lru_cache(maxsize=None)
def case(n_cols, log_n, q, seed=1):
    """Valid inputs and the model's result, computed once per shape; nobody writes to them."""
    w, sigma = M.valid_inputs(n_cols, log_n, seed)
    cp = M.copy_permutation(w, sigma, BETA, GAMMA, q)
    assert cp.zeros == 0 and cp.total == M.ONE
    return w, sigma, cp


def run(bj, w, sigma, q, beta=BETA, gamma=GAMMA, check=True, **kw):
    z, inter = bj.stage2.compute_partial_products_in_extension(bj.field.to_device(w), bj.field.to_device(sigma), beta,
                                                               gamma, q, check=check, **kw)
    got = np.stack([bj.field.to_host(c) for pair in [z] + inter for c in pair])
    status = [int(v) for v in bj.field.to_host(bj.stage2.compute_partial_products_in_extension.status)]
    return got, status


# ------------------------------------------------------------------ 1. scan
@pytest.mark.parametrize("log_n", [0, 1, 6, 7, 8, 13, 14, 16])
def test_scan_sizes(bj, log_n):
    w, sigma, cp = case(2, log_n, 1)
    got, status = run(bj, w, sigma, 1)
    assert status == [1, 0, 0, 0]
    assert np.array_equal(got, M.copy_permutation_columns(cp))


# ------------------------------------------------------------------ 2. chunking
@pytest.mark.parametrize("n_cols,q,log_n", [(3, 4, 9), (5, 4, 9), (17, 8, 9), (4, 1, 9), (8, 8, 9), (35, 2, 8),
                                            (259, 4, 3), (600, 512, 2), (300, 512, 3)])
def test_chunking(bj, n_cols, q, log_n):
    w, sigma, cp = case(n_cols, log_n, q)
    got, status = run(bj, w, sigma, q)
    m = (n_cols + q - 1) // q
    assert got.shape == (2 * m, 1 << log_n)
    assert len(cp.intermediates) == bj.stage2.num_intermediate_partial_product_relations(n_cols, q) == m - 1
    assert status == [1, 0, 0, 0]
    assert np.array_equal(got, M.copy_permutation_columns(cp))


# ------------------------------------------------------------------ 3. non-canonical inputs
def test_non_canonical_inputs_give_the_same_output(bj):
    """p added to every input that still fits a u64 (values below 2^32 - 1): every witness value
    (drawn small here), the sigmas that are small, the non-residues and the challenge limbs."""
    n_cols, log_n, q = 5, 9, 4
    n = 1 << log_n
    w, sigma = M.valid_inputs(n_cols, log_n, seed=2)
    small = np.random.default_rng(9).integers(0, 2**32 - 1, size=w.shape, dtype=np.uint64)
    # keep the permutation's cycles: equal witness values stay equal
    w = small.reshape(-1)[np.unique(w, return_inverse=True)[1].reshape(-1)].reshape(w.shape)
    beta, gamma = (BETA[0], 12345), (77, GAMMA[1])
    cp = M.copy_permutation(w, sigma, beta, gamma, q)
    assert cp.zeros == 0 and cp.total == M.ONE
    want = M.copy_permutation_columns(cp)
    got, status = run(bj, w, sigma, q, beta, gamma)
    assert status == [1, 0, 0, 0] and np.array_equal(got, want)

    def lift(a):
        a = np.asarray(a, dtype=np.uint64)
        return np.where(a < np.uint64(2**32 - 1), a + np.uint64(P), a)

    w2, s2 = lift(w), lift(sigma)
    assert (w2 >= np.uint64(P)).all() and (s2 != sigma).any()
    k = [int(v) for v in lift(M.non_residues_for_copy_permutation(n, n_cols))]
    assert all(v >= P for v in k)
    wd, sd = bj.field.to_device(w2), bj.field.to_device(s2)
    out = bj.torch.empty((2 * 2, n), dtype=bj.torch.int64, device="cuda")
    status_d = bj.torch.zeros((4,), dtype=bj.torch.int64, device="cuda")
    bj.lib.call("bj_copy_permutation_d", wd.data_ptr(), n, sd.data_ptr(), n, n_cols, log_n,
                (ctypes.c_uint64 * n_cols)(*k), beta[0], beta[1] + P, gamma[0] + P, gamma[1], q, out.data_ptr(), n,
                status_d.data_ptr(), bj.field.stream_of(out))
    assert [int(v) for v in bj.field.to_host(status_d)] == [1, 0, 0, 0]
    assert np.array_equal(bj.field.to_host(out), want)


# ------------------------------------------------------------------ 4. strides
def test_strides_and_out_inside_a_wider_trace(bj):
    """Columns that are slices of wider tensors (strides above n, other data between the columns
    that must stay as it was) and out as the copy-permutation rows of a second_stage_trace tensor."""
    n_cols, log_n, q = 5, 9, 4
    n = 1 << log_n
    w, sigma, cp = case(n_cols, log_n, q)
    want = M.copy_permutation_columns(cp)
    t = bj.torch
    wide_w = t.full((n_cols, n + 24), -1, dtype=t.int64, device="cuda")
    wide_s = t.full((n_cols, n + 8), -1, dtype=t.int64, device="cuda")
    wide_w[:, :n] = bj.field.to_device(w)
    wide_s[:, :n] = bj.field.to_device(sigma)
    wide_out = t.full((4, n + 40), -1, dtype=t.int64, device="cuda")
    z, inter = bj.stage2.compute_partial_products_in_extension(wide_w[:, :n], wide_s[:, :n], BETA, GAMMA, q,
                                                               out=wide_out[:, :n])
    assert np.array_equal(bj.field.to_host(wide_out[:, :n]), want)
    assert bool((wide_out[:, n:] == -1).all()) and z[0].data_ptr() == wide_out.data_ptr()
    st = bj.stage2.SecondStageTrace(n, n_cols, q, n_witness_enc=2, n_mult_enc=1)
    st.trace.fill_(-1)
    bj.stage2.compute_partial_products_in_extension(wide_w[:, :n], wide_s[:, :n], BETA, GAMMA, q,
                                                    out=st.copy_permutation)
    assert st.trace.shape == (2 * (2 + 2 + 1), n)
    assert np.array_equal(bj.field.to_host(st.trace[:4]), want)
    assert bool((st.trace[4:] == -1).all())


# ------------------------------------------------------------------ 5. status
def test_status_on_an_altered_sigma(bj):
    w, sigma, _ = case(5, 9, 4)
    bad = sigma.copy()
    bad[3, 300] = (int(bad[3, 300]) + 1) % P
    cp = M.copy_permutation(w, bad, BETA, GAMMA, 4)
    assert cp.zeros == 0 and cp.total != M.ONE
    got, status = run(bj, w, bad, 4, check=False)
    assert status == [cp.total[0], cp.total[1], 0, 0]
    assert np.array_equal(got, M.copy_permutation_columns(cp))
    with pytest.raises(bj.Error, match="grand product"):
        run(bj, w, bad, 4)


def test_status_on_a_zero_denominator(bj):
    """beta, gamma in the base field make w = -(beta sigma + gamma) reachable: one zero chunk
    denominator, counted, its factor taken as 0; the call returns normally."""
    w, sigma, _ = case(5, 9, 4)
    beta, gamma = (BETA[0], 0), (GAMMA[0], 0)
    w = w.copy()
    w[2, 130] = (P - (beta[0] * int(sigma[2, 130]) + gamma[0]) % P) % P
    cp = M.copy_permutation(w, sigma, beta, gamma, 4)
    assert cp.zeros == 1
    got, status = run(bj, w, sigma, 4, beta, gamma, check=False)
    assert status == [cp.total[0], cp.total[1], 1, 0]
    assert np.array_equal(got, M.copy_permutation_columns(cp))
    with pytest.raises(bj.Error, match="zero denominator"):
        run(bj, w, sigma, 4, beta, gamma)


# ------------------------------------------------------------------ 6. lookup
def rand(shape, seed, high=P):
    return np.random.default_rng(seed).integers(0, high, size=shape, dtype=np.uint64)


@pytest.mark.parametrize("log_n", [0, 5, 9, 11])
@pytest.mark.parametrize("n_src", [1, 4, 16])
def test_lookup_encoding(bj, n_src, log_n):
    """With and without f, the sources taken from two tensors (and some >= p)."""
    n = 1 << log_n
    a, b = rand((n_src // 2 + 1, n), 10 + n_src), rand((n_src, n), 20 + log_n, high=2**64)
    f = rand(n, 30 + n_src, high=2**64)
    ad, bd, fd = bj.field.to_device(a), bj.field.to_device(b), bj.field.to_device(f)
    pick = [(t % 2, t // 2) for t in range(n_src)]   # alternately from a and b
    sources = [(a, b)[w][r] for w, r in pick]
    sources_d = [(ad, bd)[w][r] for w, r in pick]
    g = [tuple(int(v) for v in rand(2, 40 + t)) for t in range(n_src)]
    out = bj.torch.empty((2, n), dtype=bj.torch.int64, device="cuda")
    for fm, fdev in ((None, None), (f, fd)):
        want, zeros = M.lookup_encoding(sources, g, BETA, fm)
        assert zeros == 0
        status = bj.stage2.lookup_encoding(sources_d, g, BETA, out[0], out[1], f=fdev)
        assert [int(v) for v in bj.field.to_host(status)] == [0, 0, 0, 0]
        assert np.array_equal(bj.field.to_host(out), M.ext_columns([want]))


def test_lookup_zero_denominator(bj):
    n = 1 << 9
    src = rand((1, n), 50)
    beta, g = (BETA[0], 0), [(GAMMA[0], 0)]
    src[0, 77] = (P - beta[0]) * pow(g[0][0], P - 2, P) % P
    want, zeros = M.lookup_encoding(src, g, beta)
    assert zeros == 1 and want[77] == M.ZERO
    out = bj.torch.empty((2, n), dtype=bj.torch.int64, device="cuda")
    status = bj.stage2.lookup_encoding([bj.field.to_device(src)[0]], g, beta, out[0], out[1])
    assert [int(v) for v in bj.field.to_host(status)] == [0, 0, 1, 0]
    assert np.array_equal(bj.field.to_host(out), M.ext_columns([want]))


def lookup_inputs(log_n, width, reps, seed):
    n = 1 << log_n
    return dict(variables=rand((1 + (width + 1) * reps, n), seed), constants=rand((2, n), seed + 1, high=7),
                tables=rand((width + 1, n), seed + 2), mult=rand((1, n), seed + 3, high=100))


@pytest.mark.parametrize("kind,idxes", [("variable", []), ("constant", [1])])
def test_lookup_poly_pairs_specialized(bj, kind, idxes):
    """Both reference variants at width 3 x 2 repetitions, the variables at offset 1."""
    width, reps = 3, 2
    d = lookup_inputs(9, width, reps, 60)
    wit, mult, zeros = M.lookup_poly_pairs_specialized(d["variables"], d["mult"], d["constants"], d["tables"], idxes,
                                                       BETA, GAMMA, 1, kind, width, reps)
    assert zeros == 0
    dev = {k: bj.field.to_device(v) for k, v in d.items()}
    gw, gm = bj.stage2.compute_lookup_poly_pairs_specialized(
        dev["variables"], dev["mult"], dev["constants"], dev["tables"], idxes, BETA, GAMMA, 1,
        bj.stage2.LookupParameters(kind, width, reps))
    assert len(gw) == reps and len(gm) == 1
    got = np.stack([bj.field.to_host(c) for pair in gw + gm for c in pair])
    assert np.array_equal(got, M.ext_columns(wit + mult))


# ------------------------------------------------------------------ 7. end to end
def test_second_stage_trace_commits_like_the_models_columns(bj):
    """second_stage_trace filled on the device and committed as it is (2^10 rows, LDE 4, cap 4)
    gives the cap of second_stage_commit fed the model's columns one by one; then the same fill
    replayed from a captured HIP graph on other inputs."""
    log_n, n_cols, q, width, reps = 10, 5, 4, 3, 2
    t = bj.torch

    def model_cap(w, sigma, d):
        cp = M.copy_permutation(w, sigma, BETA, GAMMA, q)
        assert cp.zeros == 0 and cp.total == M.ONE
        wit, mult, zeros = M.lookup_poly_pairs_specialized(d["variables"], d["mult"], d["constants"], d["tables"], [],
                                                           GAMMA, BETA, 1, "variable", width, reps)
        assert zeros == 0

        def pairs(polys):
            cols = bj.field.to_device(M.ext_columns(polys))
            return [(cols[2 * i], cols[2 * i + 1]) for i in range(len(polys))]

        ref = bj.commit.second_stage_commit(pairs([cp.z])[0], pairs(cp.intermediates), pairs(wit), pairs(mult), 4, 4, 4)
        return np.asarray(ref.get_cap())

    inputs = []
    for seed in (3, 4):
        w, sigma = M.valid_inputs(n_cols, log_n, seed)
        d = lookup_inputs(log_n, width, reps, 70 + 10 * seed)
        inputs.append((w, sigma, d, model_cap(w, sigma, d)))

    wd, sd = bj.field.to_device(inputs[0][0]), bj.field.to_device(inputs[0][1])
    dev = {k: bj.field.to_device(v) for k, v in inputs[0][2].items()}

    def fill(check):
        lookup = dict(variables_columns=dev["variables"], multiplicities_columns=dev["mult"],
                      constant_polys=dev["constants"], lookup_tables_columns=dev["tables"], table_id_column_idxes=[],
                      beta=GAMMA, gamma=BETA, variables_offset=1,
                      lookup_parameters=bj.stage2.LookupParameters("variable", width, reps))
        return bj.stage2.second_stage_trace(wd, sd, BETA, GAMMA, q, lookup=lookup, check=check)

    st = fill(True)
    assert st.trace.shape == (2 * (2 + reps + 1), 1 << log_n)
    cap = bj.commit.commit_trace_columns(st.trace, 4, 4, 4).get_cap()
    assert np.array_equal(np.asarray(cap), inputs[0][3])

    t.cuda.synchronize()
    graph = t.cuda.CUDAGraph()
    with t.cuda.graph(graph):
        st = fill(False)
    # other inputs in the captured buffers
    wd.copy_(bj.field.to_device(inputs[1][0]))
    sd.copy_(bj.field.to_device(inputs[1][1]))
    for k, v in inputs[1][2].items():
        dev[k].copy_(bj.field.to_device(v))
    st.trace.fill_(-1)
    graph.replay()
    t.cuda.synchronize()
    cap = bj.commit.commit_trace_columns(st.trace, 4, 4, 4).get_cap()
    assert np.array_equal(np.asarray(cap), inputs[1][3])
    assert not np.array_equal(inputs[0][3], inputs[1][3])
