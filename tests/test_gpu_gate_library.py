"""Library segments on the GPU (kind 3: csrc/gates_library.hpp under the frames of csrc/gates.hip): the
image compiled with native_library=True against the interpreted image of the same placements on the
same inputs, word for word, and both against the integer models (tests/gates_model.py,
tests/gates_check_model.py).

The kernels take one point (or row) per lane, 256 lanes per workgroup, and are pointwise.  Sizes:
n = 32 with q = 2, 64 points, so three quarters of the one workgroup are lanes past the end; and
n = 256 with q = 4 inside tensors of D = 8 cosets, four workgroups with column strides twice the
window.  The columns are random u64 words with representatives >= p among them, the accumulator
starts from random contents, and every status record starts from garbage."""
import functools

import numpy as np
import pytest

import gate_library_cases as L
import gates_check_model as C
import gates_model as M
import quotient_model as Q

from boojum_amd import gates as G

pytestmark = pytest.mark.gpu

P = M.P
GARBAGE = [11, 22, 33, 44]
PATHS = {0: [], 1: [False], 3: [True, False, True]}
SIZES = [(32, 2, 2), (256, 4, 8)]   # n, q, D


@pytest.fixture(scope="module")
def bj():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import boojum_amd
    from boojum_amd import _lib, field
    boojum_amd.load()
    return type("BJ", (), dict(torch=torch, field=field, lib=_lib))


def challenges(count, seed):
    return [tuple(int(v) % P for v in pair) for pair in
            np.random.default_rng(3000 + seed).integers(0, 1 << 64, size=(count, 2), dtype=np.uint64)]


def leaf_columns(a, q):
    return [] if a is None else [[int(v) for v in col[:q].reshape(-1)] for col in a]


def both_sets(placements):
    """(interpreted set, library set); the second holds at least one segment of kind 3."""
    plain, library = G.GateSet(placements), G.GateSet(placements, native_library=True)
    assert 3 not in L.kinds_of(plain.image) and 3 in L.kinds_of(library.image)
    assert library.need == dict(plain.need, segments=library.num_segments)
    return plain, library


def terms_three_ways(bj, placements, n, q, d, seed):
    """Runs both images on the same columns, challenges and start; returns the library set."""
    plain, library = both_sets(placements)
    need = plain.need
    v, w, c = (L.words((need[k], d, n), 10 * seed + i) if need[k] else None
               for i, k in enumerate(("variables", "witnesses", "constants")))
    alphas = challenges(need["alphas"], seed)
    start = np.random.default_rng(77 + seed).integers(0, P, size=(2, q * n), dtype=np.uint64)
    dev = lambda a: None if a is None else bj.field.to_device(a)   # noqa: E731
    vd, wd, cd = dev(v), dev(w), dev(c)
    got = []
    for gate_set in (plain, library):
        dst = bj.field.to_device(start)
        G.evaluate_gate_terms(gate_set, vd, wd, cd, alphas, q, dst[0], dst[1])
        got.append(dst)
    assert bj.torch.equal(got[0], got[1])
    ext = [(int(start[0][i]), int(start[1][i])) for i in range(q * n)]
    want = M.gate_terms(placements, leaf_columns(v, q), leaf_columns(w, q), leaf_columns(c, q), alphas, start=ext)
    assert np.array_equal(bj.field.to_host(got[1]), Q.acc_columns(want))
    return library


# ------------------------------------------------------------------ 1. every gate alone
@pytest.mark.parametrize("n,q,d", SIZES, ids=["64-points", "1024-points-in-D8"])
@pytest.mark.parametrize("evaluator", G.library(), ids=lambda e: e.name)
def test_each_gate_alone(bj, evaluator, n, q, d):
    program = G.capture(evaluator)
    for reps in (1, 3):
        for depth, path in PATHS.items():
            pl = G.GatePlacement(program, reps, None, path, None, G.PerChunkOffset(2, 1, 1))
            library = terms_three_ways(bj, [pl], n, q, d, seed=10 * reps + depth)
            assert L.kinds_of(library.image) == [3] and library.num_terms == reps * evaluator.num_quotient_terms


# ------------------------------------------------------------------ 2. specialized placement
@pytest.mark.parametrize("share_constants", [True, False], ids=["shared", "own"])
def test_specialized_fma(bj, share_constants):
    pl = G.specialized_placement(G.FmaGateInBaseFieldWithoutConstant(), 3, share_constants, G.PerChunkOffset(5, 0, 1),
                                 2)
    for n, q, d in SIZES:
        library = terms_three_ways(bj, [pl], n, q, d, seed=40 + share_constants)
        assert library.need["constants"] == (2 + 1 + 2 if share_constants else 2 + 1 + 2 * 2 + 2)


# ------------------------------------------------------------------ 3. the mixed set
def test_mixed_set_carries_the_alpha_base_across_kinds(bj):
    placements = L.mixed_set()
    library = terms_three_ways(bj, placements, 32, 2, 2, seed=50)
    image = library.image
    assert L.kinds_of(image) == [3, 1, 0, 3]
    assert [image[image[2 + s] + 4] for s in range(4)] == [0, 8, 126, 128] and library.num_terms == 133


def test_bench_set(bj):
    library = terms_three_ways(bj, L.bench_set(), 256, 4, 8, seed=51)
    assert L.kinds_of(library.image) == [3] and library.num_segments == 1


# ------------------------------------------------------------------ 4. the satisfiability check
N_ROWS = 80   # one workgroup of 256 lanes: a full wave, sixteen rows of a second, 176 lanes past the end


@functools.lru_cache(maxsize=None)
def check_case(which):
    """(placements, satisfying trace, random trace), built once; tests corrupt copies."""
    placements = L.mixed_set() if which == "mixed" else L.bench_set()
    need = G.check_image(G.compile_gate_set(placements))
    shape = (need["variables"], need["witnesses"], need["constants"])
    good = L.satisfying_trace(placements, shape, N_ROWS, seed=60)
    # any u64 word, without the planted 0 / 1 / p cells: no zero term and no zero selector product (seeds 70 ..)
    noise = tuple(np.random.default_rng(70 + i).integers(0, 1 << 64, size=(k, N_ROWS), dtype=np.uint64)
                  for i, k in enumerate(shape))
    return placements, good, noise


@functools.lru_cache(maxsize=None)
def sets_of(which):
    return both_sets(check_case(which)[0])


def records(bj, which, trace, rows=None):
    """The record of the interpreted image, of the library image and of the model."""
    placements = check_case(which)[0]
    dev = lambda a: bj.field.to_device(a) if a.shape[0] else None   # noqa: E731
    v, w, c = (dev(a) for a in trace)
    got = []
    for gate_set in sets_of(which):
        status = bj.field.to_device(np.array(GARBAGE, dtype=np.uint64))
        report = G.check_if_satisfied(gate_set, v, w, c, rows, status=status)
        got.append([int(x) for x in bj.field.to_host(status)])
        assert report.num_unsatisfied == got[-1][0]
    return got[0], got[1], C.status_record(placements, *trace, rows)


@pytest.mark.parametrize("which", ["mixed", "bench"])
def test_check_satisfying_trace(bj, which):
    plain, library, want = records(bj, which, check_case(which)[1])
    assert want == [0, C.NO_KEY, 0, 0] and plain == want and library == want


@pytest.mark.parametrize("which", ["mixed", "bench"])
def test_check_one_corrupted_cell(bj, which):
    """Variable 0 of a row that runs gate 0 (FMA in both sets): its first repetition's term, k = 0."""
    placements, good, _ = check_case(which)
    row = 3 * len(placements)
    bad = good[0].copy()
    bad[0, row] = (int(bad[0, row]) + 1) % P
    plain, library, want = records(bj, which, (bad, good[1], good[2]))
    assert want[:2] == [1, row << 32 | 0] and want[2] != 0
    assert plain == want and library == want
    report = G.check_if_satisfied(sets_of(which)[1], *(bj.field.to_device(a) if a.shape[0] else None
                                                       for a in (bad, good[1], good[2])))
    assert (report.row, report.gate, report.subinstance, report.term, report.value) == (row, 0, 0, 0, want[2])
    assert report.gate_name == "fma_gate_in_base_without_constant"


@pytest.mark.parametrize("which", ["mixed", "bench"])
def test_check_every_term_fails(bj, which):
    placements, _, noise = check_case(which)
    plain, library, want = records(bj, which, noise)
    assert want[:2] == [N_ROWS * M.total_terms(placements), 0]
    assert plain == want and library == want


@pytest.mark.parametrize("which", ["mixed", "bench"])
def test_check_window_that_ends_inside_a_wave(bj, which):
    """Rows 30 .. 69: the window starts inside the first wave of the trace's rows and ends inside the
    second; failures planted before it, on its first and last row and after it."""
    placements, good, _ = check_case(which)
    bad = good[0].copy()
    for r in (0, 29, 30, 69, 70, 79):
        bad[0, r] = (int(bad[0, r]) + 2) % P
    trace = (bad, good[1], good[2])
    plain, library, want = records(bj, which, trace, (30, 40))
    assert want[0] >= 1 and 30 <= want[1] >> 32 < 70
    assert want[0] == C.check(placements, *trace, (30, 1))[0] + C.check(placements, *trace, (69, 1))[0]
    assert plain == want and library == want


@pytest.mark.parametrize("which", ["mixed", "bench"])
def test_check_two_windows_on_one_record(bj, which):
    """The second window's calls go without the begin flag: the counts add, the smaller key and its value win."""
    placements, good, noise = check_case(which)
    bad = good[0].copy()
    bad[0, 60] = (int(bad[0, 60]) + 1) % P
    bad[0, 12] = (int(bad[0, 12]) + 1) % P
    trace = (bad, good[1], good[2])
    dev = lambda a: bj.field.to_device(a) if a.shape[0] else None   # noqa: E731
    v, w, c = dev(bad), dev(good[1]), dev(good[2])   # held to the end: the raw calls take their addresses
    columns, _ = G._bind(G._trace, variables=v, witnesses=w, constants=c)
    stream = bj.field.stream_of(v)
    got = []
    for gate_set in sets_of(which):
        status = bj.field.to_device(np.array(GARBAGE, dtype=np.uint64))
        for window, (begin, count) in enumerate(((40, 40), (0, 40))):
            for segment in range(gate_set.num_segments):
                flag = G.CHECK_BEGIN if window == 0 and segment == 0 else 0
                bj.lib.call("bj_gate_set_satisfied_d", gate_set._handle, segment | flag, *columns, begin, count,
                            status.data_ptr(), stream)
        got.append([int(x) for x in bj.field.to_host(status)])
    first, second = C.status_record(placements, *trace, (40, 40)), C.status_record(placements, *trace, (0, 40))
    assert first[0] >= 1 and second[0] >= 1 and second[1] < first[1]
    want = [first[0] + second[0], second[1], second[2], 0]
    assert want == C.status_record(placements, *trace)
    assert got[0] == want and got[1] == want


# ------------------------------------------------------------------ 5. graph capture and refusal
def test_captures_into_a_graph(bj):
    torch = bj.torch
    n, q = 32, 2
    placements = [G.GatePlacement(G.capture(G.DotProductGate(4)), 2, None, [True, False]),
                  G.GatePlacement(G.capture(G.ZeroCheckGate(True)), 3, None, [False])]
    library = G.GateSet(placements, native_library=True)
    assert L.kinds_of(library.image) == [3]
    v, w, c = L.words((18, q, n), 1), L.words((3, q, n), 2), L.words((2, q, n), 3)
    alphas = challenges(library.num_terms, 4)
    to = bj.field.to_device
    vd, wd, cd, ad = to(v), to(w), to(c), G.challenges_tensor(alphas, "cuda")
    dst = torch.zeros((2, q * n), dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):   # load the kernel before the capture
        G.evaluate_gate_terms(library, vd, wd, cd, ad, q, dst[0], dst[1])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = bj.field.to_host(dst)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        G.evaluate_gate_terms(library, vd, wd, cd, ad, q, dst[0], dst[1])
    dst.zero_()
    graph.replay()
    torch.cuda.synchronize()
    want = Q.acc_columns(M.gate_terms(placements, leaf_columns(v, q), leaf_columns(w, q), leaf_columns(c, q), alphas))
    assert np.array_equal(bj.field.to_host(dst), want) and np.array_equal(eager, want)


def test_too_few_columns_are_refused(bj):
    placements = [G.GatePlacement(G.capture(G.FmaGateInBaseFieldWithoutConstant()), 2, None, [True]),
                  G.GatePlacement(G.capture(G.ZeroCheckGate(True)), 3, None, [False])]
    library = G.GateSet(placements, native_library=True)
    assert L.kinds_of(library.image) == [3]
    assert library.need == dict(variables=8, witnesses=3, constants=3, alphas=8, segments=1)
    n, q = 32, 2
    to = bj.field.to_device
    v, w, c = to(L.words((8, q, n), 1)), to(L.words((3, q, n), 2)), to(L.words((3, q, n), 3))
    start = L.words((2, q * n), 8)
    dst = to(start)
    alphas = challenges(8, 9)
    for args, message in (((v[:7], w, c, alphas), "an operand reaches variables column 7 of 7"),
                          ((v, w[:2], c, alphas), "an operand reaches witnesses column 2 of 2"),
                          ((v, w, None, alphas), "an operand reaches constants column 2 of 0"),
                          ((v, w, c, alphas[:-1]), "fewer challenges than terms")):
        with pytest.raises(bj.lib.BoojumError, match=r"\(-22\)") as info:
            G.evaluate_gate_terms(library, *args, q, dst[0], dst[1])
        assert message in str(info.value)
    bj.torch.cuda.synchronize()
    assert np.array_equal(bj.field.to_host(dst), start)
