"""check_if_satisfied on sets with a native Poseidon2 segment (bj_gate_set_satisfied_d on kind 1,
csrc/gates_poseidon2.hpp) against the model's record (tests/poseidon2_gate_model.status_record):
count, the smallest key row << 32 | k and that term's canonical value, every word equal.

Traces: 8 rows (a partly filled wave) and 300 rows (two workgroups) of satisfying instances, two
repetitions, nw = 5, behind a Boolean gate x 3 and before a Reduction gate, none under a selector
unless the test says so; tests corrupt copies."""
import functools

import numpy as np
import pytest

import gates_model as M
import poseidon2_gate_model as PM

from boojum_amd import gates as G

pytestmark = pytest.mark.gpu

P = M.P
NW = 5
GARBAGE = [0x1111, 0x2222, 0x3333, 0x4444]   # the record is initialised by the first call, not by the caller


@pytest.fixture(scope="module")
def bj():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import boojum_amd
    from boojum_amd import _lib, field
    boojum_amd.load()
    return type("BJ", (), dict(torch=torch, field=field, lib=_lib))


def placements(path=()):
    """Boolean x 3 on variables 0..2 (k = 0..2), Poseidon2 x 2 from variable 3 and witness 0
    (k = 3..238), Reduction<4> on variables 253..257 with constants after the path (k = 239)."""
    depth = len(path)
    return [G.GatePlacement(G.capture(G.BooleanConstraintGate()), 3, None, path),
            PM.placement(NW, 2, path, G.PerChunkOffset(3, 0, 0)),
            G.GatePlacement(G.capture(G.ReductionGate(4)), 1, None, path, depth, G.PerChunkOffset(253, 0, 0))]


@functools.lru_cache(maxsize=None)
def trace(n, depth=0):
    rng = np.random.default_rng(n + depth)
    v = np.zeros((258, n), dtype=np.uint64)
    w = np.zeros((2 * NW, n), dtype=np.uint64)
    c = rng.integers(0, P, size=(depth + 4, n), dtype=np.uint64)
    v[:3] = rng.integers(0, 2, size=(3, n), dtype=np.uint64)
    for r in range(n):
        for rep in range(2):
            cells, wit = PM.satisfying_row([int(x) for x in rng.integers(0, P, size=12, dtype=np.uint64)], NW)
            v[3 + 125 * rep:3 + 125 * (rep + 1), r], w[NW * rep:NW * (rep + 1), r] = cells, wit
        x = [int(t) for t in rng.integers(0, P, size=4, dtype=np.uint64)]
        v[253:257, r] = x
        v[257, r] = sum(a * int(k) for a, k in zip(x, c[depth:depth + 4, r])) % P
    return v, w, c


def bump(a, col, row, by=1):
    a[col, row] = (int(a[col, row]) % P + by) % P


def run(bj, pls, v, w, c, rows=None):
    dev = bj.field.to_device
    status = dev(np.array(GARBAGE, dtype=np.uint64))
    gate_set = G.GateSet(pls)
    assert [gate_set.image[gate_set.image[2 + s] + 7] for s in range(gate_set.num_segments)] == [0, 1, 0]
    report = G.check_if_satisfied(gate_set, dev(v), dev(w), dev(c), rows, status=status)
    return report, [int(x) for x in bj.field.to_host(status)], PM.status_record(pls, v, w, c, rows)


def assert_report(report, want, gate, subinstance, term):
    row, k = want[1] >> 32, want[1] & 0xffffffff
    assert (report.num_unsatisfied, report.row, report.k, report.value) == (want[0], row, k, want[2])
    assert (report.gate, report.subinstance, report.term) == (gate, subinstance, term)
    name = ["boolean_constraint", "poseidon2_flattened", "reduction_gate_4"][gate]
    assert report.gate_name == name
    assert report.message() == \
        "Unsatisfied at row %d with value 0x%016x for term number %d for subinstance number %d of gate %s" % (
            row, want[2], term, subinstance, name)


@pytest.mark.parametrize("n", [8, 300])
def test_satisfying_trace(bj, n):
    v, w, c = trace(n)
    report, got, want = run(bj, placements(), v, w, c)
    assert want == [0, PM.NO_KEY, 0, 0] and got == want
    assert report.satisfied is True and report.num_unsatisfied == 0 and report.message() is None


@pytest.mark.parametrize("n,row", [(8, 5), (300, 270)])
def test_one_corrupted_cell(bj, n, row):
    """Cell s = 40 (a partial-round cell) of the second instance: its own term, k = 3 + 118 + 40,
    fails with value -1 and so does every term up to the next reset of the whole state (30 in all)."""
    v, w, c = (a.copy() for a in trace(n))
    bump(v, 3 + 125 + 24 + 40 - NW, row)
    report, got, want = run(bj, placements(), v, w, c)
    assert want[:3] == [30, row << 32 | (3 + 118 + 40), P - 1] and got == want
    assert_report(report, want, 1, 1, 40)


def test_a_witness_cell_and_an_output_cell(bj):
    v, w, c = (a.copy() for a in trace(8))
    bump(w, 2, 6)           # cell s = 2 of the first instance on row 6: term 2 and the next reset's 12
    bump(v, 3 + 12 + 7, 3)  # output 7 of the first instance on row 3: term 106 + 7 alone, value +1
    report, got, want = run(bj, placements(), v, w, c)
    assert want[:3] == [14, 3 << 32 | (3 + 113), 1] and got == want
    assert_report(report, want, 1, 0, 113)


def test_keys_across_kinds(bj):
    """The smallest key wins whichever kind of segment holds it, in both directions."""
    v, w, c = (a.copy() for a in trace(300))
    bump(v, 3 + 24 + 50 - NW, 200)   # Poseidon2, row 200
    bump(v, 257, 260)                # Reduction (after the native segment), row 260
    bump(v, 1, 280, 2)               # Boolean (before it), row 280
    report, got, want = run(bj, placements(), v, w, c)
    assert want[1] == 200 << 32 | (3 + 50) and got == want
    assert_report(report, want, 1, 0, 50)
    bump(v, 2, 100, 2)               # now an interpreted gate fails on a smaller row
    report, got, want = run(bj, placements(), v, w, c)
    assert want[1] == 100 << 32 | 2 and got == want
    assert_report(report, want, 0, 2, 0)
    bump(v, 257, 100)                # the same row: the native segment's k lies between the two
    bump(v, 3 + 125 + 5, 100)        # input 5 of the second instance: terms 0..11, k = 3 + 118
    bump(v, 2, 100, P - 2)           # the Boolean cell is put right again
    report, got, want = run(bj, placements(), v, w, c)
    assert want[1] == 100 << 32 | (3 + 118) and got == want
    assert_report(report, want, 1, 1, 0)


def test_row_window(bj):
    v, w, c = (a.copy() for a in trace(300))
    bump(v, 3 + 24 + 50 - NW, 200)
    report, got, want = run(bj, placements(), v, w, c, rows=(201, 99))
    assert want == [0, PM.NO_KEY, 0, 0] and got == want and report.satisfied
    report, got, want = run(bj, placements(), v, w, c, rows=(190, 11))
    assert want[1] == 200 << 32 | 53 and got == want
    assert_report(report, want, 1, 0, 50)


def test_selector_masks_failures(bj):
    """Under path [1, 0] a failing instance counts only on rows the selector does not vanish on."""
    path = (True, False)
    v, w, c = (a.copy() for a in trace(8, 2))
    c[0], c[1] = [1, 1, 0, 0, 1, 1, 0, 1], [0, 1, 0, 0, 0, 1, 1, 0]   # selected: rows 0, 4 and 7
    for r in range(8):
        bump(v, 3 + 12 + 1, r)   # output 1 of the first instance: one term per row
    report, got, want = run(bj, placements(path), v, w, c)
    assert want[:3] == [3, 0 << 32 | (3 + 107), 1] and got == want
    assert_report(report, want, 1, 0, 107)
