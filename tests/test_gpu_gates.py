"""GPU gate terms (boojum_amd/gates.py, csrc/gates.hip) against the Python-integer model
(tests/gates_model.py), every output bit-equal.

The kernel takes one point per thread, 256 threads per workgroup, and is pointwise, so the column
tensors of most tests hold seeded random words, not LDEs of anything; the end-to-end and graph
tests run real LDEs.  The accumulator always starts from seeded random words, so every test also
checks that the call adds.  The sizes are the smallest that reach each path:

* Points (q n of them).  q = 2 with n = 1: two points; n = 2^3: 16 points, a partly filled wave;
  n = 2^7: 256 points, exactly one workgroup; n = 2^9: four workgroups.  q = 8 at n = 2^4.  Sources
  at D = 8 read at q = 2: the column stride is 8 n and only the first 2 n words of a column are
  read.  A thread never takes a second point.
* Selectors, at 16 points: no path; depth 1 at both polarities; depth 3 with mixed bits; depth 8,
  the cap; two gates under one prefix.
* Programs, at 16 points: each evaluator of the library once and at its repetition count for 128
  variable, 4 witness and 8 constant columns (FMA x 32); specialized placement with initial
  offsets, with shared and with per-repetition constants; bare-column and ConstantValue writes,
  Mul(x, x), Double / Negate / Square and the constants 0, 1, p - 1 (gates_model.PowerSumEvaluator);
  a chain of 300 temporaries in three slots; 16 such chains, 4800 instructions, which is two
  launches (the cap is 4096), against the model and against two sets that fit one launch each.
* End to end (n = 2^3, q = 4) and graph capture on the satisfiable circuit of gates_model.
* Errors: a tensor with fewer columns than an operand reaches, too few challenges, and an image
  over the instruction cap, each BJ_EINVAL with the accumulator untouched."""
import functools

import numpy as np
import pytest

import gates_model as M
import quotient_model as Q
import stage2_model as S

from boojum_amd import gates as G

pytestmark = pytest.mark.gpu

P = M.P
BETA, GAMMA = (0x1234567890ABCDEF % P, 0x0FEDCBA987654321), (0xDEADBEEFCAFEF00D % P, 0x1122334455667788)
PATH8 = [True, False, False, True, True, False, True, False]


@pytest.fixture(scope="module")
def bj():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import boojum_amd
    from boojum_amd import _lib, field, lde, quotient, stage2
    boojum_amd.load()
    return type("BJ", (), dict(torch=torch, field=field, stage2=stage2, quotient=quotient, lde=lde, lib=_lib))


def rand(shape, seed):
    a = np.random.default_rng(seed).integers(0, P, size=shape, dtype=np.uint64)
    a.reshape(-1)[:3] = [0, 1, P - 1][:a.size]
    return a


def challenges(count, seed):
    return [tuple(int(v) for v in pair) for pair in rand((count, 2), 3000 + seed)]


def columns(n_cols, d, n, seed):
    """(C, D, n) random words; None for no columns."""
    return rand((n_cols, d, n), seed) if n_cols else None


def leaf_columns(a, q):
    """The first q cosets of a (C, D, n) array as the model's leaf-order columns."""
    return [] if a is None else [[int(v) for v in col[:q].reshape(-1)] for col in a]


def run(bj, placements, shape, q, d=None, n=8, seed=1, gate_set=None, alphas=None, start=None):
    """Evaluates on the device and in the model; shape = (variables, witnesses, constants)."""
    d = d or q
    v, w, c = (columns(k, d, n, 10 * seed + i) for i, k in enumerate(shape))
    alphas = alphas or challenges(M.total_terms(placements), seed)
    start = rand((2, q * n), 77 + seed) if start is None else start
    dst = bj.field.to_device(start)
    to = lambda a: None if a is None else bj.field.to_device(a)   # noqa: E731
    gate_set = gate_set or G.GateSet(placements)
    G.evaluate_gate_terms(gate_set, to(v), to(w), to(c), alphas, q, dst[0], dst[1])
    ext = [(int(start[0][i]), int(start[1][i])) for i in range(q * n)]
    want = M.gate_terms(placements, leaf_columns(v, q), leaf_columns(w, q), leaf_columns(c, q), alphas, start=ext)
    return bj.field.to_host(dst), Q.acc_columns(want)


def small_set():
    fma, ps = G.FmaGateInBaseFieldWithoutConstant(), M.PowerSumEvaluator()
    return [G.GatePlacement(G.capture(fma), 2, None, [True]), G.GatePlacement(G.capture(ps), 2, None, [False, True]),
            G.GatePlacement(G.capture(G.ConstantsAllocatorGate()), 2, None, [False, False])], (8, 2, 4)


# ------------------------------------------------------------------ 1. points
@pytest.mark.parametrize("q,log_n,d", [(2, 0, 2), (2, 3, 2), (2, 7, 2), (2, 9, 2), (8, 4, 8), (2, 3, 8)])
def test_point_counts(bj, q, log_n, d):
    placements, shape = small_set()
    got, want = run(bj, placements, shape, q, d, 1 << log_n, seed=log_n + d)
    assert np.array_equal(got, want)


# ------------------------------------------------------------------ 2. selectors
@pytest.mark.parametrize("paths", [[[]], [[True]], [[False]], [[True, False, True]], [PATH8],
                                   [[True, False], [True, True]], [[], [False], PATH8]],
                         ids=["empty", "one", "zero", "mixed3", "cap8", "shared-prefix", "mixed-depths"])
def test_selector_paths(bj, paths):
    sg = G.SelectionGate()
    placements = [G.GatePlacement(G.capture(sg), 2, None, path) for path in paths]
    got, want = run(bj, placements, (8, 0, 8), 2, seed=len(paths[0]))
    assert np.array_equal(got, want)


def test_selector_polarity_on_binary_columns(bj):
    """With 0 / 1 selector columns exactly one of two complementary gates contributes per point."""
    bc = G.BooleanConstraintGate()
    placements = [G.GatePlacement(G.capture(bc), 1, None, [True]), G.GatePlacement(G.capture(bc), 1, None, [False])]
    n, q = 8, 2
    v = rand((1, q, n), 5)
    c = (np.arange(q * n, dtype=np.uint64) % 2).reshape(1, q, n)
    alphas = challenges(2, 6)
    dst = bj.torch.zeros((2, q * n), dtype=bj.torch.int64, device="cuda")
    G.evaluate_gate_terms(G.GateSet(placements), bj.field.to_device(v), None, bj.field.to_device(c), alphas, q,
                          dst[0], dst[1])
    want = M.gate_terms(placements, leaf_columns(v, q), [], leaf_columns(c, q), alphas)
    assert np.array_equal(bj.field.to_host(dst), Q.acc_columns(want))
    for L, value in enumerate(want):
        a = int(v.reshape(-1)[L])
        assert value == M.IntOps.scale(alphas[0] if L % 2 else alphas[1], a * (1 - a) % P)


# ------------------------------------------------------------------ 3. programs
GEOMETRY = G.CSGeometry(128, 4, 8, 8)


@pytest.mark.parametrize("full", [False, True], ids=["once", "geometry"])
@pytest.mark.parametrize("evaluator", G.library() + [M.PowerSumEvaluator()], ids=lambda e: e.name)
def test_every_evaluator(bj, evaluator, full):
    reps = evaluator.num_repetitions_in_geometry(GEOMETRY) if full else 1
    if evaluator.name == "power_sum":
        reps = min(reps, 4)
    assert not full or evaluator.name != "fma_gate_in_base_without_constant" or reps == 32
    pl = G.GatePlacement(G.capture(evaluator), reps, None, [True, False])
    got, want = run(bj, [pl], (128, 4, 10), 2, seed=reps)
    assert np.array_equal(got, want)


def test_specialized_placement(bj):
    """No selector; the columns start at the initial offset; the constants after the 3 of the
    general-purpose set; FMA's two coefficients shared by its repetitions, the allocator's constant
    advancing with them.  A general-purpose gate runs in the same set."""
    fma = G.specialized_placement(G.FmaGateInBaseFieldWithoutConstant(), 3, True, G.PerChunkOffset(2, 0, 1), 3)
    alloc = G.specialized_placement(G.ConstantsAllocatorGate(), 3, False, G.PerChunkOffset(14, 0, 3), 3)
    general = G.GatePlacement(G.capture(G.ZeroCheckGate(True)), 1, None, [False, True, True])
    assert fma.bases() == (2, 0, 4) and alloc.bases() == (14, 0, 6) and alloc.per_chunk_offset.as_tuple() == (1, 0, 1)
    got, want = run(bj, [fma, alloc, general], (17, 1, 9), 2, seed=4)
    assert np.array_equal(got, want)


def test_chain_of_300_temporaries(bj):
    pl = G.GatePlacement(M.chain_program(300), 1)
    assert G.allocate_slots(pl.program)[1] == 3
    got, want = run(bj, [pl], (1, 0, 0), 2, seed=3)
    assert np.array_equal(got, want)


def test_two_launches_agree_with_sets_that_fit(bj):
    chains = [G.GatePlacement(M.chain_program(300), 1, G.PerChunkOffset(), [bool(i & 1)]) for i in range(16)]
    whole = G.GateSet(chains)
    assert whole.num_segments == 2
    alphas = challenges(16, 8)
    start = rand((2, 16), 9)
    got, want = run(bj, chains, (1, 0, 1), 2, seed=5, gate_set=whole, alphas=alphas, start=start)
    assert np.array_equal(got, want)
    first, second = G.GateSet(chains[:13]), G.GateSet(chains[13:])
    assert first.num_segments == second.num_segments == 1
    half, _ = run(bj, chains[:13], (1, 0, 1), 2, seed=5, gate_set=first, alphas=alphas[:13], start=start)
    both, _ = run(bj, chains[13:], (1, 0, 1), 2, seed=5, gate_set=second, alphas=alphas[13:], start=half)
    assert np.array_equal(both, got)


# ------------------------------------------------------------------ 4. end to end on the device
@functools.lru_cache(maxsize=None)
def circuit_case(seed):
    c = M.satisfiable_circuit(seed=seed)
    gate_alphas = challenges(M.total_terms(c.placements), 20 + seed)
    cp_alphas = challenges(c.n_vars // 4 + 1, 30)
    return c, gate_alphas, cp_alphas, M.circuit_quotient(c, BETA, GAMMA, gate_alphas, cp_alphas)


def test_end_to_end_on_the_device(bj):
    """Stage 2, the LDEs, the gate terms, the copy-permutation terms, the division and the
    monomials on the device for the satisfiable circuit; then one corrupted trace cell."""
    c, gate_alphas, cp_alphas, r = circuit_case(7)
    q = 1 << c.log_q
    to = bj.field.to_device
    gate_set = G.GateSet(c.placements)

    def pipeline(variables):
        wd, sd = to(variables), to(c.sigma)
        st = bj.stage2.second_stage_trace(wd, sd, BETA, GAMMA, q, check=False)
        lde = lambda t: bj.lde.transform_raw_storages_to_lde(t, q)   # noqa: E731
        return bj.quotient.quotient_from_arguments(
            lde(wd), lde(sd), lde(st.trace), BETA, GAMMA, cp_alphas, q,
            gates=dict(gate_set=gate_set, witnesses_lde=lde(to(c.witnesses)), constants_lde=lde(to(c.constants)),
                       alphas=gate_alphas))

    chunks, top_is_zero = pipeline(c.variables)
    assert top_is_zero == (True, True)
    assert np.array_equal(bj.field.to_host(chunks), r.q.chunks) and r.q.chunks.any()

    bad = c.variables.copy()
    bad[7, 0] = (int(bad[7, 0]) + 1) % P   # d of the second FMA on row 0: term 1, whose challenge has c0 = p - 1
    rb = M.circuit_quotient(c, BETA, GAMMA, gate_alphas, cp_alphas, variables=bad)
    model_top = (rb.q.mono[0][-1] == 0, rb.q.mono[1][-1] == 0)
    assert model_top[0] is False
    chunks, top_is_zero = pipeline(bad)
    assert top_is_zero == model_top
    assert np.array_equal(bj.field.to_host(chunks), rb.q.chunks)


def test_gate_terms_and_caller_terms_both_add(bj):
    c, gate_alphas, cp_alphas, r = circuit_case(7)
    q = 1 << c.log_q
    total = q << c.log_n
    start = rand((2, total), 40)
    lde = lambda cols: bj.field.to_device(np.array(cols, dtype=np.uint64).reshape(len(cols), q, -1))   # noqa: E731
    d = bj.field.to_device(start)
    G.evaluate_gate_terms(G.GateSet(c.placements), lde(r.q.w_lde), lde(r.wit_lde), lde(r.const_lde), gate_alphas, q,
                          d[0], d[1])
    ext = [(int(start[0][i]), int(start[1][i])) for i in range(total)]
    want = [Q.T.e_add(a, b) for a, b in zip(ext, r.gate_terms)]
    assert np.array_equal(bj.field.to_host(d), Q.acc_columns(want))


# ------------------------------------------------------------------ 5. graph capture
def test_gate_terms_capture_into_one_graph_with_the_rest(bj):
    """The gate call, the copy-permutation call and the division captured on one stream; after
    every input, the gate challenges included, is overwritten in place, a replay gives the second
    circuit's divided accumulator."""
    torch = bj.torch
    runs = [circuit_case(7), circuit_case(8)]
    c0, _, cp_alphas, _ = runs[0]
    q, log_n = 1 << c0.log_q, c0.log_n
    total = q << log_n
    lde = lambda cols: bj.field.to_device(np.array(cols, dtype=np.uint64).reshape(len(cols), q, -1))   # noqa: E731

    def tensors(c, gate_alphas, r):
        return [lde(r.q.w_lde), lde(r.wit_lde), lde(r.const_lde), lde(r.q.sigma_lde), lde(S.ext_columns(r.q.s2_lde)),
                G.challenges_tensor(gate_alphas, "cuda")]

    v, w, k, s, z, a = tensors(runs[0][0], runs[0][1], runs[0][3])
    gate_set = G.GateSet(c0.placements)   # both circuits have the same gates; the traces differ
    dst = torch.zeros((2, total), dtype=torch.int64, device="cuda")

    def calls():
        G.evaluate_gate_terms(gate_set, v, w, k, a, q, dst[0], dst[1])
        bj.quotient.compute_quotient_terms_in_extension(v, s, z, BETA, GAMMA, cp_alphas, q, dst[0], dst[1])
        bj.quotient.divide_by_vanishing_for_bitreversed_coset_enumeration(dst[0], dst[1], log_n)

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):   # load the kernels before the capture
        calls()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        calls()
    assert runs[0][1] != runs[1][1]
    for c, gate_alphas, _, r in runs:
        for t, new in zip((v, w, k, s, z, a), tensors(c, gate_alphas, r)):
            t.copy_(new)
        dst.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bj.field.to_host(dst), Q.acc_columns(r.q.divided))


# ------------------------------------------------------------------ 6. errors
def test_errors_leave_the_accumulator_untouched(bj):
    placements, shape = small_set()
    gate_set = G.GateSet(placements)
    n, q = 8, 2
    start = rand((2, q * n), 50)
    dst = bj.field.to_device(start)
    to = bj.field.to_device
    v, w, c = (to(columns(k, q, n, 60 + i)) for i, k in enumerate(shape))
    alphas = challenges(M.total_terms(placements), 51)
    for args in ((v[:7], w, c, alphas), (v, w[:1], c, alphas), (v, w, c[:3], alphas), (v, None, c, alphas),
                 (v, w, c, alphas[:-1])):
        with pytest.raises(bj.lib.BoojumError, match=r"\(-22\)"):
            G.evaluate_gate_terms(gate_set, *args, q, dst[0], dst[1])
    with pytest.raises(bj.lib.BoojumError, match=r"\(-22\)"):   # over the instruction cap: refused at upload
        image = G.compile_gate_set([G.GatePlacement(M.chain_program(300), 1)] * 13)
        image[image[2] + 1] = G.MAX_INSTRUCTIONS + 1
        G.GateSet.from_image(image)
    with pytest.raises(ValueError):   # one gate over the cap cannot be split
        G.GateSet([G.GatePlacement(M.chain_program(G.MAX_INSTRUCTIONS + 1), 1)])
    bj.torch.cuda.synchronize()
    assert np.array_equal(bj.field.to_host(dst), start)
    G.evaluate_gate_terms(gate_set, v, w, c, alphas, q, dst[0], dst[1])   # and the same call with good arguments runs
    assert not np.array_equal(bj.field.to_host(dst), start)
