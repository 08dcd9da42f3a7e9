"""The Poseidon2 flattened gate's terms on the GPU (a native segment of a gate set: boojum_amd/gates.py,
csrc/gates_poseidon2.hpp) against the Python model (tests/poseidon2_gate_model.py), every word equal.

The kernel takes one point per lane, 256 lanes per workgroup, and is pointwise, so the columns hold
seeded random words with the representatives p, p + 1 and 2^64 - 1 among them; the accumulator always
starts from random Ext2 values, so every case checks that the call adds.  Sizes: q n = 16 (n = 8,
q = 2), a partly filled workgroup, and q n = 1024 (n = 128, q = 8), four workgroups.  Splits
nw = 0, 5 (the cells change kind inside the first reset) and 106 (every cell a witness); one and two
repetitions (260 columns); no selector and depth 3 with mixed bits; D > q and a column stride above
D n.  The model at 1024 points is the structured one, pinned to the evaluator and its capture by
test_poseidon2_gate_cpu.py; at 16 points the mixed set runs the captured program itself."""
import ctypes

import numpy as np
import pytest

import gates_model as M
import poseidon2_gate_model as PM
import quotient_model as Q

from boojum_amd import gates as G

pytestmark = pytest.mark.gpu

P = M.P
BETA, GAMMA = (0x1234567890ABCDEF % P, 0x0FEDCBA987654321), (0xDEADBEEFCAFEF00D % P, 0x1122334455667788)
EDGES = [P, P + 1, (1 << 64) - 1, 0, 1, P - 1]


@pytest.fixture(scope="module")
def bj():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import boojum_amd
    from boojum_amd import _lib, field, lde, quotient, stage2
    boojum_amd.load()
    return type("BJ", (), dict(torch=torch, field=field, stage2=stage2, quotient=quotient, lde=lde, lib=_lib))


def words(shape, seed, edges=True):
    """Random u64 words, any representative; the edge representatives first."""
    a = np.random.default_rng(seed).integers(0, 1 << 64, size=shape, dtype=np.uint64)
    if edges and a.size:
        flat = a.reshape(-1)
        flat[:len(EDGES)] = EDGES[:flat.size]
        flat[-1] = P
    return a


def challenges(count, seed):
    return [tuple(int(v) % P for v in pair) for pair in words((count, 2), 3000 + seed, edges=False)]


def device_lde(bj, a, pad):
    """(C, D, n) host words -> a device tensor of that shape whose column stride is D n + pad."""
    if a is None:
        return None
    c, d, n = a.shape
    buf = np.zeros((c, d * n + pad), dtype=np.uint64)
    buf[:, :d * n] = a.reshape(c, d * n)
    t = bj.field.to_device(buf)[:, :d * n].view(c, d, n) if pad else bj.field.to_device(a)
    assert t.stride(0) == d * n + pad or c == 1
    return t


def leaf_columns(a, q):
    return [] if a is None else [[int(v) for v in col[:q].reshape(-1)] for col in a]


def run(bj, placements, shape, q, n, d=None, pad=0, seed=1):
    d = d or q
    v, w, c = (words((k, d, n), 10 * seed + i) if k else None for i, k in enumerate(shape))
    alphas = challenges(M.total_terms(placements), seed)
    start = words((2, q * n), 77 + seed, edges=False) % np.uint64(P)
    dst = bj.field.to_device(start)
    gate_set = G.GateSet(placements)
    G.evaluate_gate_terms(gate_set, device_lde(bj, v, pad), device_lde(bj, w, pad), device_lde(bj, c, pad), alphas, q,
                          dst[0], dst[1])
    ext = [(int(start[0][i]), int(start[1][i])) for i in range(q * n)]
    want = PM.gate_sum(placements, leaf_columns(v, q), leaf_columns(w, q), leaf_columns(c, q), alphas, ext)
    return bj.field.to_host(dst), Q.acc_columns(want), gate_set


CASES = [
    # nw, reps, path, q, n, D, pad
    (0, 1, [], 2, 8, 2, 0),
    (5, 1, [True, False, True], 2, 8, 2, 0),
    (106, 1, [], 2, 8, 2, 0),
    (5, 2, [False, True, True], 2, 8, 4, 3),
    (106, 2, [True, False, False], 2, 8, 2, 0),
    (0, 1, [], 8, 128, 8, 0),
    (5, 1, [True, True, False], 8, 128, 16, 5),
    (106, 1, [False, True, False], 8, 128, 8, 0),
]


@pytest.mark.parametrize("nw,reps,path,q,n,d,pad", CASES)
def test_gate_terms(bj, nw, reps, path, q, n, d, pad):
    pl = PM.placement(nw, reps, path)
    shape = (reps * (PM.CELLS - nw), reps * nw, len(path))
    if reps == 2:
        assert shape[0] + shape[1] == 260
    got, want, gate_set = run(bj, [pl], shape, q, n, d, pad, seed=nw + reps)
    assert gate_set.num_segments == 1 and gate_set.num_terms == 118 * reps
    assert np.array_equal(got, want)


def test_initial_offsets_and_wider_repetitions(bj):
    """The instance starts at variable 3 and witness 2, and a repetition is wider than its cells."""
    pl = PM.placement(5, 2, [True], G.PerChunkOffset(3, 2, 0), ncu=127)
    got, want, _ = run(bj, [pl], (3 + 127 + 125, 2 + 10, 1), 2, 8, seed=9)
    assert np.array_equal(got, want)


def mixed_placements(nw=5):
    return [G.GatePlacement(G.capture(G.FmaGateInBaseFieldWithoutConstant()), 2, None, [True]),
            G.GatePlacement(G.capture(G.BooleanConstraintGate()), 3, None, [False, True]),
            G.GatePlacement(PM.captured(PM.CELLS - nw, nw), 2, None, [False, False, True]),
            G.GatePlacement(G.capture(G.ReductionGate(4)), 1, None, [False, False, False])]


def test_mixed_set_carries_the_alpha_base_across_kinds(bj):
    """FMA and Boolean before the gate, Reduction after it: three segments; the model's sum is the
    captured programs' (gates_model.gate_terms), the Poseidon2 capture included."""
    placements = mixed_placements()
    q, n = 2, 8
    v, w, c = words((250, q, n), 1) % np.uint64(P), words((10, q, n), 2) % np.uint64(P), words((7, q, n), 3) % np.uint64(P)
    alphas = challenges(M.total_terms(placements), 4)
    start = words((2, q * n), 5, edges=False) % np.uint64(P)
    dst = bj.field.to_device(start)
    gate_set = G.GateSet(placements)
    assert gate_set.num_segments == 3 and gate_set.num_terms == 2 + 3 + 236 + 1
    assert [gate_set.image[gate_set.image[2 + s] + 7] for s in range(3)] == [0, 1, 0]
    to = bj.field.to_device
    G.evaluate_gate_terms(gate_set, to(v), to(w), to(c), alphas, q, dst[0], dst[1])
    ext = [(int(start[0][i]), int(start[1][i])) for i in range(q * n)]
    want = M.gate_terms(placements, leaf_columns(v, q), leaf_columns(w, q), leaf_columns(c, q), alphas, start=ext)
    assert np.array_equal(bj.field.to_host(dst), Q.acc_columns(want))
    assert want == PM.gate_sum(placements, leaf_columns(v, q), leaf_columns(w, q), leaf_columns(c, q), alphas, ext)


def test_satisfying_rows_give_nothing_and_match_the_library_permutation(bj):
    """On satisfying instances every term is 0, so the accumulator is unchanged; the output cells
    are the library's own permutation of the inputs."""
    q, n, nw = 2, 8, 5
    rows = [PM.satisfying_row([int(x) for x in words((12,), 40 + L)], nw) for L in range(q * n)]
    v = np.array([r[0] for r in rows], dtype=np.uint64).T.reshape(PM.CELLS - nw, q, n).copy()
    w = np.array([r[1] for r in rows], dtype=np.uint64).T.reshape(nw, q, n).copy()
    state = (ctypes.c_uint64 * 12)(*[int(x) for x in v[:12, 0, 0]])
    bj.lib.call("bj_poseidon2_permute_h", state)
    assert list(state) == [int(x) for x in v[12:24, 0, 0]]
    start = words((2, q * n), 6, edges=False) % np.uint64(P)
    dst = bj.field.to_device(start)
    G.evaluate_gate_terms(G.GateSet([PM.placement(nw)]), bj.field.to_device(v), bj.field.to_device(w), None,
                          challenges(118, 7), q, dst[0], dst[1])
    assert np.array_equal(bj.field.to_host(dst), start)


def test_captures_into_a_graph(bj):
    """One launch per call, so the captured graph is a chain; one replay."""
    torch = bj.torch
    q, n, nw = 2, 8, 5
    pl = PM.placement(nw, 1, [True, False])
    v, w, c = words((125, q, n), 11), words((5, q, n), 12), words((2, q, n), 13)
    alphas = challenges(118, 14)
    gate_set = G.GateSet([pl])
    to = bj.field.to_device
    vd, wd, cd, ad = to(v), to(w), to(c), G.challenges_tensor(alphas, "cuda")
    dst = torch.zeros((2, q * n), dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):   # load the kernel before the capture
        G.evaluate_gate_terms(gate_set, vd, wd, cd, ad, q, dst[0], dst[1])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = bj.field.to_host(dst)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        G.evaluate_gate_terms(gate_set, vd, wd, cd, ad, q, dst[0], dst[1])
    dst.zero_()
    graph.replay()
    torch.cuda.synchronize()
    want = PM.gate_sum([pl], leaf_columns(v, q), leaf_columns(w, q), leaf_columns(c, q), alphas, [M.ZERO] * (q * n))
    assert np.array_equal(bj.field.to_host(dst), Q.acc_columns(want))
    assert np.array_equal(eager, Q.acc_columns(want))


def test_too_few_columns_are_refused(bj):
    pl = PM.placement(5, 2, [True])
    gate_set = G.GateSet([pl])
    q, n = 2, 8
    to = bj.field.to_device
    v, w, c = to(words((250, q, n), 1)), to(words((10, q, n), 2)), to(words((1, q, n), 3))
    start = words((2, q * n), 8, edges=False)
    dst = to(start)
    alphas = challenges(236, 9)
    for args in ((v[:249], w, c, alphas), (v, w[:9], c, alphas), (v, w, None, alphas), (v, w, c, alphas[:-1])):
        with pytest.raises(bj.lib.BoojumError, match=r"\(-22\)"):
            G.evaluate_gate_terms(gate_set, *args, q, dst[0], dst[1])
    bj.torch.cuda.synchronize()
    assert np.array_equal(bj.field.to_host(dst), start)


# ------------------------------------------------------------------ end to end
def poseidon2_circuit(seed=7):
    """n = 8 rows over 125 variable, 5 witness and 3 constant columns: even rows hold a Poseidon2
    instance (path [1]), odd rows two FMAs (path [0], coefficients in constants 1 and 2).  Degree 7
    plus a selector of depth 1: quotient degree 8."""
    rng = np.random.default_rng(seed)
    r = lambda: int(rng.integers(0, P, dtype=np.uint64))   # noqa: E731
    c = M.Circuit()
    c.log_n, c.log_q, c.n_vars, c.n_wits, c.n_consts = 3, 3, 125, 5, 3
    n = 8
    c.placements = [G.GatePlacement(PM.captured(125, 5), 1, None, [True]),
                    G.GatePlacement(G.capture(G.FmaGateInBaseFieldWithoutConstant()), 2, None, [False])]
    c.variables = rng.integers(0, P, size=(125, n), dtype=np.uint64)
    c.witnesses = rng.integers(0, P, size=(5, n), dtype=np.uint64)
    c.constants = rng.integers(0, P, size=(3, n), dtype=np.uint64)
    for i in range(n):
        c.constants[0, i] = 1 - i % 2
        if i % 2 == 0:
            v, w = PM.satisfying_row([r() for _ in range(12)], 5)
            c.variables[:, i], c.witnesses[:, i] = v, w
        else:
            for rep in range(2):
                a, b, x = r(), r(), r()
                c.variables[4 * rep:4 * rep + 4, i] = [a, b, x, (int(c.constants[1, i]) * a % P * b
                                                                 + int(c.constants[2, i]) * x) % P]
    c.sigma = M.sigma_for(c.variables, c.log_n)
    return c


def test_end_to_end_quotient(bj):
    """Stage 2, the LDEs and quotient_from_arguments(gates=...) on the device: the top coefficients
    are zero for the satisfying trace and not for one corrupted cell; chunks equal the model's."""
    c = poseidon2_circuit()
    q = 1 << c.log_q
    gate_alphas = challenges(M.total_terms(c.placements), 21)
    cp_alphas = challenges((c.n_vars + q - 1) // q + 1, 22)
    to = bj.field.to_device
    gate_set = G.GateSet(c.placements)
    assert [gate_set.image[gate_set.image[2 + s] + 7] for s in range(gate_set.num_segments)] == [1, 0]

    def pipeline(variables):
        wd, sd = to(variables), to(c.sigma)
        st = bj.stage2.second_stage_trace(wd, sd, BETA, GAMMA, q, check=False)
        lde = lambda t: bj.lde.transform_raw_storages_to_lde(t, q)   # noqa: E731
        return bj.quotient.quotient_from_arguments(
            lde(wd), lde(sd), lde(st.trace), BETA, GAMMA, cp_alphas, q,
            gates=dict(gate_set=gate_set, witnesses_lde=lde(to(c.witnesses)), constants_lde=lde(to(c.constants)),
                       alphas=gate_alphas))

    r = M.circuit_quotient(c, BETA, GAMMA, gate_alphas, cp_alphas)
    chunks, top_is_zero = pipeline(c.variables)
    assert top_is_zero == (True, True)
    assert np.array_equal(bj.field.to_host(chunks), r.q.chunks) and r.q.chunks.any()

    bad = c.variables.copy()
    bad[24 + 40, 2] = (int(bad[24 + 40, 2]) + 1) % P   # a partial-round cell of the instance on row 2
    chunks, top_is_zero = pipeline(bad)
    assert top_is_zero != (True, True)
