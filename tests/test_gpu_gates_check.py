"""The gate satisfiability check on the device (boojum_amd.gates.check_if_satisfied,
bj_gate_set_satisfied_d in csrc/gates.hip) against the integer model (tests/gates_check_model.py):
the whole status record -- the count, the key row << 32 | k and the term's value -- bit for bit,
and the report's gate, subinstance and term against a brute-force enumeration.

The kernel takes one row per lane, 64 lanes per wave, 256 per workgroup; a wave that saw a failure
issues one add and one min on the record, and a second one-wave launch fetches the value.  So the
sizes are n = 2^10 rows (four workgroups, sixteen waves) and, for the partly filled wave, 2^3; the
windows end inside a wave, inside a workgroup and on the last row.  Every status record starts
from garbage, so every test also checks that the first call of a check initialises it."""
import functools

import numpy as np
import pytest

import gates_check_model as C
import gates_model as M

from boojum_amd import gates as G

pytestmark = pytest.mark.gpu

P = M.P
N = 1 << 10
PATH8 = [True, False, False, True, True, False, True, False]
GARBAGE = [11, 22, 33, 44]


@pytest.fixture(scope="module")
def bj():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import boojum_amd
    from boojum_amd import _lib, field
    boojum_amd.load()
    return type("BJ", (), dict(torch=torch, field=field, lib=_lib))


def rand(shape, seed):
    return np.random.default_rng(seed).integers(0, P, size=shape, dtype=np.uint64)


def bits(shape, seed):
    return np.random.default_rng(seed).integers(0, 2, size=shape, dtype=np.uint64)


def bump(a, col, row, by=1):
    a[col, row] = (int(a[col, row]) % P + by) % P


def cols_of(a):
    return [] if a is None else a


def run(bj, placements, v, w, c, rows=None, gate_set=None):
    """The device's record and report, and the model's record."""
    dev = lambda a: None if a is None else bj.field.to_device(a)   # noqa: E731
    status = bj.field.to_device(np.array(GARBAGE, dtype=np.uint64))
    report = G.check_if_satisfied(gate_set or G.GateSet(placements), dev(v), dev(w), dev(c), rows, status=status)
    got = [int(x) for x in bj.field.to_host(status)]
    return report, got, C.status_record(placements, cols_of(v), cols_of(w), cols_of(c), rows)


def assert_same(placements, report, got, want):
    assert got == want
    assert report.num_unsatisfied == want[0] and report.satisfied == (want[0] == 0)
    if want[0] == 0:
        assert got[1] == C.NO_KEY and report.row is None and report.message() is None
        return
    row, k = want[1] >> 32, want[1] & 0xffffffff
    gate, sub, term = C.locate_brute(placements, k)
    assert (report.row, report.k, report.gate, report.subinstance, report.term, report.value) == \
        (row, k, gate, sub, term, want[2])
    evaluator = placements[gate].program.evaluator
    assert report.gate_name == (evaluator.name if evaluator else None)
    assert report.message() == \
        "Unsatisfied at row %d with value 0x%016x for term number %d for subinstance number %d of gate %s" % (
            row, want[2], term, sub, report.gate_name if evaluator else "#%d" % gate)


@functools.lru_cache(maxsize=None)
def circuit(log_n):
    """gates_model.satisfiable_circuit, shared: tests corrupt copies."""
    return M.satisfiable_circuit(log_n)


# ------------------------------------------------------------------ 1. a satisfied circuit
@pytest.mark.parametrize("log_n", [3, 10])
def test_satisfied_circuit(bj, log_n):
    c = circuit(log_n)
    report, got, want = run(bj, c.placements, c.variables, c.witnesses, c.constants)
    assert want == [0, C.NO_KEY, 0, 0]
    assert_same(c.placements, report, got, want)
    assert report.satisfied is True


# ------------------------------------------------------------------ 2. one corrupted cell
@pytest.mark.parametrize("log_n,row", [(3, 4), (10, 516)])
def test_one_corrupted_cell(bj, log_n, row):
    c = circuit(log_n)
    bad = c.variables.copy()
    bump(bad, 7, row)   # d of the second FMA of an FMA row: term k = 1, value -1
    report, got, want = run(bj, c.placements, bad, c.witnesses, c.constants)
    assert want == [1, row << 32 | 1, P - 1, 0]
    assert_same(c.placements, report, got, want)
    assert (report.gate_name, report.subinstance, report.term) == ("fma_gate_in_base_without_constant", 1, 0)


# ------------------------------------------------------------------ 3. ordering
def test_smaller_row_wins_across_workgroups(bj):
    c = circuit(10)
    bad = c.variables.copy()
    bump(bad, 7, 700)
    bump(bad, 3, 300)   # d of the first FMA: k = 0; row 300 is in the second workgroup, 700 in the third
    report, got, want = run(bj, c.placements, bad, c.witnesses, c.constants)
    assert want[:2] == [2, 300 << 32 | 0]
    assert_same(c.placements, report, got, want)


def two_gate_trace(seed=3):
    """Boolean x 4 on variables 0..3 and a Selection on variables 4..7, neither under a selector,
    and a trace that satisfies both on every row."""
    sel = G.SelectionGate()
    placements = [G.GatePlacement(G.capture(G.BooleanConstraintGate()), 4),
                  G.GatePlacement(G.capture(sel), 1, None, (), 0, G.PerChunkOffset(4, 0, 0))]
    v = np.concatenate([bits((4, N), seed), rand((4, N), seed + 1)])
    for r in range(N):
        a, b, s = (int(v[4 + i, r]) for i in range(3))
        v[7, r] = (a * s + (1 - s) * b) % P
    return placements, v


def test_smaller_k_wins_on_one_row(bj):
    placements, v = two_gate_trace()
    assert C.check(placements, v, [], []) == (0, None)
    bump(v, 7, 500)      # the Selection's result: k = 4
    bump(v, 2, 500, 2)   # the third Boolean: k = 2
    bump(v, 7, 501)
    report, got, want = run(bj, placements, v, None, None)
    assert want[:2] == [3, 500 << 32 | 2]
    assert_same(placements, report, got, want)
    assert (report.gate, report.subinstance) == (0, 2)


# ------------------------------------------------------------------ 4. windows
WINDOWS = [(0, 1), (1, 1023), (300, 257), (5, 3)]


@pytest.mark.parametrize("rows", WINDOWS, ids=lambda w: "%d+%d" % w)
def test_windows(bj, rows):
    """Failures before, at both ends of and after each window: rows 0, 5, 7, 299, 300, 556, 557 and
    1023 (variable 0 is an input of every gate kind of the circuit)."""
    c = circuit(10)
    bad = c.variables.copy()
    for r in (0, 5, 7, 299, 300, 556, 557, 1023):
        bump(bad, 0, r, 2)
    report, got, want = run(bj, c.placements, bad, c.witnesses, c.constants, rows)
    assert want[0] > 0 and rows[0] <= want[1] >> 32 < rows[0] + rows[1]
    assert_same(c.placements, report, got, want)


@pytest.mark.parametrize("rows", [(1, 1023), (5, 3), (1, 1), (300, 257)], ids=lambda w: "%d+%d" % w)
def test_window_that_excludes_the_corrupted_row_0(bj, rows):
    """Lanes past the window must count nothing: a lane that fell back to row 0 would report it."""
    c = circuit(10)
    bad = c.variables.copy()
    for col in range(8):
        bump(bad, col, 0, 2)
    assert C.check(c.placements, bad, c.witnesses, c.constants, (0, 1))[0] > 0
    report, got, want = run(bj, c.placements, bad, c.witnesses, c.constants, rows)
    assert want == [0, C.NO_KEY, 0, 0]
    assert_same(c.placements, report, got, want)


def test_window_past_its_first_row_is_not_charged_to_it(bj):
    """A window that ends inside a wave, with its own first row failing: that row counts once."""
    c = circuit(10)
    bad = c.variables.copy()
    bump(bad, 7, 300)
    report, got, want = run(bj, c.placements, bad, c.witnesses, c.constants, (300, 5))
    assert want == [1, 300 << 32 | 1, P - 1, 0]
    assert_same(c.placements, report, got, want)


# ------------------------------------------------------------------ 5. selectors
@functools.lru_cache(maxsize=None)
def selector_case():
    """Three Booleans on variables 0, 1, 2 under paths of depth 1, 3 and 8; 0 / 1 selector columns;
    a non-boolean cell planted on every seventh row, in the gate r mod 3, whose selector is
    alternately made 1 (the row's cells follow its path) and 0 (level 0 against its path)."""
    bc = G.capture(G.BooleanConstraintGate())
    paths = [[True], [False, True, False], PATH8]
    placements = [G.GatePlacement(bc, 1, None, path, None, G.PerChunkOffset(g, 0, 0)) for g, path in enumerate(paths)]
    v, k = bits((3, N), 11), bits((8, N), 12)
    planted = [(r % 3, r) for r in range(0, N, 7)]
    for j, (g, r) in enumerate(planted):
        v[g, r] = 2 + r
        if (j // 3) % 2:
            k[0, r] = 0 if paths[g][0] else 1
        else:
            k[:len(paths[g]), r] = paths[g]
    return placements, v, k, planted


def selector_of(placements, k, g, r):
    return M.selector_at(placements[g].selector_path, [int(x) % P for x in k[:, r]])


def test_selectors_hide_and_show(bj):
    placements, v, k, planted = selector_case()
    shown = [(g, r) for g, r in planted if selector_of(placements, k, g, r)]
    for g in range(3):   # every depth both hides a non-zero term and shows one
        assert any(x == g for x, _ in shown) and any(x == g and (x, r) not in shown for x, r in planted)
    report, got, want = run(bj, placements, v, None, k)
    assert want[0] == len(shown) and want[1] == shown[0][1] << 32 | shown[0][0]
    assert_same(placements, report, got, want)


@pytest.mark.parametrize("g", [0, 1, 2], ids=["depth1", "depth3", "depth8"])
def test_selector_cell_of_5_is_reported(bj, g):
    placements, v, k, planted = selector_case()
    k = k.copy()
    row = next(r for x, r in planted if x == g and not selector_of(placements, k, g, r))   # hidden so far
    path = placements[g].selector_path
    for level, bit in enumerate(path):   # the path's cells to 1 (or 0 for a negated level): selector 1 ...
        k[level, row] = int(bit)
    k[0, row] = 5                        # ... and now 5 at a taken level, 1 - 5 at a negated one
    assert selector_of(placements, k, g, row) == (5 if path[0] else P - 4)
    report, got, want = run(bj, placements, v, None, k, (row, 1))
    assert want[:3] == [1, row << 32 | g, (2 + row) * (1 - (2 + row)) % P]
    assert_same(placements, report, got, want)


# ------------------------------------------------------------------ 6. non-canonical words
def lifted(a):
    """Every cell + p where that still fits 64 bits."""
    a = a.copy()
    small = a < np.uint64((1 << 64) - P)
    a[small] += np.uint64(P)
    return a, int(small.sum())


def test_non_canonical_cells_change_nothing(bj):
    placements, v, k, _ = selector_case()
    (v2, nv), (k2, nk) = lifted(v), lifted(k)
    assert nv == v.size and nk == k.size   # bits and small planted values: every cell moves
    report, got, want = run(bj, placements, v2, None, k2)
    assert want == C.status_record(placements, v, [], k) and want[0] > 0
    assert_same(placements, report, got, want)
    c = circuit(10)   # here the selector cells, the flags and the zero inputs move
    bad = c.variables.copy()
    bump(bad, 7, 516)
    (v3, nv), (w3, _), (k3, nk) = lifted(bad), lifted(c.witnesses), lifted(c.constants)
    assert nk >= 2 * N and nv > 0
    report, got, want = run(bj, c.placements, v3, w3, k3)
    assert want == [1, 516 << 32 | 1, P - 1, 0]
    assert_same(c.placements, report, got, want)


def test_a_term_that_is_the_word_p_is_satisfied(bj):
    """A pushed column cell holding p, p - 1 + 1 formed by an addition, and both under a selector."""
    idx, rel = G.Index, G.Relation
    bare = G.GateProgram([], [idx.VariablePoly(0)], 1)
    plus = G.GateProgram([(0, rel.Add(idx.VariablePoly(1), idx.ConstantValue(1)))], [idx.TemporaryValue(0)], 1)
    placements = [G.GatePlacement(bare, 1), G.GatePlacement(plus, 1), G.GatePlacement(bare, 1, None, [True]),
                  G.GatePlacement(plus, 1, None, [True])]
    v = np.zeros((2, 8), dtype=np.uint64)
    v[0], v[1] = P, P - 1
    k = np.full((1, 8), 3, dtype=np.uint64)
    report, got, want = run(bj, placements, v, None, k)
    assert want == [0, C.NO_KEY, 0, 0]
    assert_same(placements, report, got, want)
    v[0, 5] = P + 1   # the word p + 1 is the value 1
    report, got, want = run(bj, placements, v, None, k)
    assert want == [2, 5 << 32 | 0, 1, 0]
    assert_same(placements, report, got, want)


# ------------------------------------------------------------------ 7. every term of every row fails
@pytest.mark.parametrize("rows", [(0, N), (300, 257)], ids=lambda w: "%d+%d" % w)
def test_every_term_of_every_row_fails(bj, rows):
    c = circuit(10)
    v, w, k = rand((8, N), 71), rand((1, N), 72), rand((5, N), 73)
    terms = M.total_terms(c.placements)
    for r in range(rows[0], rows[0] + rows[1]):   # seeds 71..73: no accidental zero term or selector product
        assert all(sel * term % P for _, sel, term in C.row_terms(c.placements, v[:, r], w[:, r], k[:, r]))
    report, got, want = run(bj, c.placements, v, w, k, rows)
    assert want[:2] == [rows[1] * terms, rows[0] << 32 | 0]
    assert_same(c.placements, report, got, want)


# ------------------------------------------------------------------ 8. several segments
@functools.lru_cache(maxsize=None)
def many_booleans():
    bc = G.capture(G.BooleanConstraintGate())
    placements = [G.GatePlacement(bc, 1, None, (), 0, G.PerChunkOffset(g, 0, 0)) for g in range(66)]
    assert G.compile_gate_set(placements)[1] == 2
    return placements, bits((66, N), 81)


@pytest.mark.parametrize("cells,first", [([(65, 900)], (900, 65)), ([(3, 950), (65, 900), (64, 900)], (900, 64)),
                                         ([(3, 100), (65, 900)], (100, 3))],
                         ids=["last-segment-only", "later-segment-wins", "first-segment-keeps-its-value"])
def test_several_segments(bj, cells, first):
    placements, v = many_booleans()
    v = v.copy()
    for g, r in cells:
        v[g, r] = 7 + g
    report, got, want = run(bj, placements, v, None, None)
    g = first[1]
    assert want == [len(cells), first[0] << 32 | g, (7 + g) * (1 - (7 + g)) % P, 0]
    assert_same(placements, report, got, want)
    assert report.gate == g and report.gate_name == "boolean_constraint"


# ------------------------------------------------------------------ 9. every evaluator
GEOMETRY = G.CSGeometry(128, 4, 8, 8)
RESULT_LAST = (G.ReductionGate, G.SelectionGate, G.DotProductGate)


def satisfy(e, rng, row_v, row_w, row_c, off):
    """One repetition's cells of a row so that e's terms vanish (PowerSum's cannot: its term 5)."""
    v0, width = off[0], e.principal_width[0]
    if isinstance(e, G.BooleanConstraintGate):
        row_v[v0] = int(rng.integers(0, 2))
    elif isinstance(e, RESULT_LAST):   # term = f(inputs) - result
        row_v[v0 + width - 1] = 0
        row_v[v0 + width - 1] = M.run_evaluator(e, row_v, row_w, row_c, off)[0]
    elif not isinstance(e, M.PowerSumEvaluator):
        M._satisfy(e, rng, row_v, row_w, row_c, off)


@pytest.mark.parametrize("full", [False, True], ids=["once", "geometry"])
@pytest.mark.parametrize("evaluator", G.library() + [M.PowerSumEvaluator()], ids=lambda e: e.name)
def test_every_evaluator(bj, evaluator, full):
    """A trace that satisfies the gate in every repetition of every row (under the path [1, 0]),
    then variable 0 of the last repetition of row 777 moved by 2."""
    reps = evaluator.num_repetitions_in_geometry(GEOMETRY) if full else 1
    if evaluator.name == "power_sum":
        reps = min(reps, 4)
    pl = G.GatePlacement(G.capture(evaluator), reps, None, [True, False])
    rng = np.random.default_rng(90 + reps)
    v, w, k = rand((128, N), 91), rand((4, N), 92), rand((10, N), 93)
    k[0], k[1] = 1, 0
    bases, per = pl.bases(), pl.per_chunk_offset.as_tuple()
    for r in range(N):
        row = [[int(x) for x in a[:, r]] for a in (v, w, k)]
        for rep in range(reps):
            satisfy(evaluator, rng, *row, tuple(b + rep * p for b, p in zip(bases, per)))
        v[:, r], w[:, r], k[:, r] = row
    bump(v, bases[0] + (reps - 1) * per[0], 777, 2)
    report, got, want = run(bj, [pl], v, w, k)
    if evaluator.name != "power_sum":
        assert want[1] >> 32 == 777 and 1 <= want[0] <= evaluator.num_quotient_terms
        assert (want[1] & 0xffffffff) // evaluator.num_quotient_terms == reps - 1
    else:
        assert want[0] >= N * reps
    assert_same([pl], report, got, want)


# ------------------------------------------------------------------ 10. errors
def test_errors_leave_the_status_untouched(bj):
    c = circuit(10)
    gate_set = G.GateSet(c.placements)
    dev = bj.field.to_device
    bad = c.variables.copy()
    bump(bad, 7, 516)
    v, w, k = dev(bad), dev(c.witnesses), dev(c.constants)
    status = dev(np.array(GARBAGE, dtype=np.uint64))
    stream = bj.field.stream_of(v)
    good = dict(set=gate_set._handle, segment=G.CHECK_BEGIN, vars=v.data_ptr(), vars_stride=N, n_vars=8,
                wits=w.data_ptr(), wits_stride=N, n_wits=1, consts=k.data_ptr(), consts_stride=N, n_consts=5,
                row_begin=0, n_rows=N, status=status.data_ptr(), stream=stream)

    def call(**over):
        bj.lib.call("bj_gate_set_satisfied_d", *dict(good, **over).values())

    for over in (dict(set=None), dict(segment=1), dict(segment=G.CHECK_BEGIN | 1), dict(n_vars=7), dict(n_wits=0),
                 dict(n_consts=4), dict(vars=None), dict(wits=None), dict(consts=None), dict(vars_stride=N - 1),
                 dict(consts_stride=N - 1), dict(row_begin=1), dict(row_begin=N, n_rows=1), dict(n_rows=0),
                 dict(n_rows=N + 1), dict(row_begin=1 << 32, n_rows=1, vars_stride=1 << 40, wits_stride=1 << 40,
                                          consts_stride=1 << 40),
                 dict(row_begin=(1 << 32) - 1, n_rows=2, vars_stride=1 << 40, wits_stride=1 << 40,
                      consts_stride=1 << 40),
                 dict(row_begin=(1 << 64) - 1, n_rows=2, vars_stride=1 << 40, wits_stride=1 << 40,
                      consts_stride=1 << 40)):
        with pytest.raises(bj.lib.BoojumError, match=r"\(-22\)"):
            call(**over)
    with pytest.raises(bj.lib.BoojumError, match=r"\(-22\)"):
        call(status=None)
    for rows in ((0, 0), (1, N), (-1, 2), (N, 1)):   # the Python call refuses these itself
        with pytest.raises(ValueError):
            G.check_if_satisfied(gate_set, v, w, k, rows, status=status)
    with pytest.raises(ValueError):
        G.check_if_satisfied(gate_set, v, w[:, :8], k, status=status)
    bj.torch.cuda.synchronize()
    assert [int(x) for x in bj.field.to_host(status)] == GARBAGE
    call()   # and the same call with good arguments runs
    assert [int(x) for x in bj.field.to_host(status)] == [1, 516 << 32 | 1, P - 1, 0]
    call(segment=0)   # without the begin flag a second call combines: the count adds, the key and value stay
    assert [int(x) for x in bj.field.to_host(status)] == [2, 516 << 32 | 1, P - 1, 0]


# ------------------------------------------------------------------ 11. two windows on one record
def test_a_second_window_leaves_the_value_of_a_key_outside_it(bj):
    """The record holds a key of row 516 from a first call.  A second call without the begin flag
    checks another window, over a trace in which row 516 is satisfied: the key does not move, and
    the value must not be fetched again from a row the call does not cover (it would read 0)."""
    c = circuit(10)
    gate_set = G.GateSet(c.placements)
    dev = bj.field.to_device
    bad = c.variables.copy()
    bump(bad, 7, 516)
    worse = c.variables.copy()
    bump(worse, 7, 40)
    v1, v2, v3, w, k = dev(bad), dev(c.variables), dev(worse), dev(c.witnesses), dev(c.constants)
    status = dev(np.array(GARBAGE, dtype=np.uint64))

    def call(v, segment, begin, count):
        bj.lib.call("bj_gate_set_satisfied_d", gate_set._handle, segment, v.data_ptr(), N, 8, w.data_ptr(), N, 1,
                    k.data_ptr(), N, 5, begin, count, status.data_ptr(), bj.field.stream_of(v))
        return [int(x) for x in bj.field.to_host(status)]

    first = [1, 516 << 32 | 1, P - 1, 0]
    assert call(v1, G.CHECK_BEGIN, 0, N) == first
    assert call(v2, 0, 0, 100) == first          # window before the key's row
    assert call(v2, 0, 517, N - 517) == first    # window after it
    assert call(v2, 0, 516, 1) == [1, 516 << 32 | 1, 0, 0]   # a window that covers the row does fetch: 0 in this trace
    assert call(v3, 0, 0, 100) == [2, 40 << 32 | 1, P - 1, 0]   # and a smaller key moves key and value
