"""What the library-segment tests share (test_gate_library_cpu.py, test_gpu_gate_library.py): the
bench set, a mixed set over all three segment kinds, an evaluator the library does not know, and
traces that satisfy a set row by row."""
import os
import sys

import numpy as np

import gates_model as M
import poseidon2_gate_model as PM

from boojum_amd import gates as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = M.P
RESULT_LAST = (G.ReductionGate, G.SelectionGate, G.DotProductGate)


class ProductGate(G.Evaluator):
    """a b - c: a captured evaluator that is not in the library."""
    name = "test_product_gate"
    principal_width = (3, 0, 0)

    def evaluate_once(self, src, dst, shared):
        a, b, c = (src.get_variable_value(i) for i in range(3))
        r = a.copy()
        r.mul_assign(b)
        r.sub_assign(c)
        dst.push_evaluation_result(r)


RESULT_LAST += (ProductGate,)


class AlteredSelectionGate(G.SelectionGate):
    """SelectionGate's name over other relations: b s + (1 - s) a - result."""

    def evaluate_once(self, src, dst, shared):
        a, b, s, result = (src.get_variable_value(i) for i in range(4))
        r = b.copy()
        r.mul_assign(s)
        t = src.field().one()
        t.sub_assign(s)
        r.mul_and_accumulate_into(t, a)
        r.sub_assign(result)
        dst.push_evaluation_result(r)


def bench_set(n_vars=130):
    """tools/gates_bench.py's set: eight gates under the leaves of a depth-3 selector tree."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gates_bench
    return gates_bench.bench_set(G, n_vars)


def path_of(i, depth=3):
    return [bool(i >> b & 1) for b in range(depth)]


def mixed_set():
    """Two library gates, the Poseidon2 flattened gate (5 witness cells), an evaluator the library does
    not know, two library gates: segments of kinds 3, 1, 0, 3.  Leaves 0 .. 5 of a depth-3 selector
    tree; 125 variable, 5 witness and 3 + 4 constant columns.  The Poseidon2 placement carries the
    capture, so the integer models run it; compile_gate_set goes by the evaluator's native kind."""
    gates = [(G.FmaGateInBaseFieldWithoutConstant(), 2), (G.ZeroCheckGate(True), 3), (None, 1), (ProductGate(), 2),
             (G.ReductionGate(4), 1), (G.ConditionalSwapGate(1), 2)]
    return [G.GatePlacement(PM.captured(125, 5) if e is None else G.capture(e), reps, None, path_of(i))
            for i, (e, reps) in enumerate(gates)]


def kinds_of(image):
    return [image[image[2 + s] + 7] for s in range(image[1])]


def words(shape, seed):
    """Random u64 words, values >= p among them (about one in 2^32, and the first cells)."""
    a = np.random.default_rng(seed).integers(0, 1 << 64, size=shape, dtype=np.uint64)
    flat = a.reshape(-1)
    edges = [P, P + 1, (1 << 64) - 1, 0, 1, P - 1]
    flat[:len(edges)] = edges[:flat.size]
    return a


def satisfy(e, rng, row_v, row_w, row_c, off):
    """One repetition's cells of a row so that e's terms vanish."""
    v0, w0 = off[0], off[1]
    if isinstance(e, G.Poseidon2FlattenedGate):
        nw = e.num_witness_columns_used
        v, w = PM.satisfying_row([int(rng.integers(0, P, dtype=np.uint64)) for _ in range(12)], nw)
        row_v[v0:v0 + len(v)], row_w[w0:w0 + nw] = v, w
    elif isinstance(e, G.BooleanConstraintGate):
        row_v[v0] = int(rng.integers(0, 2))
    elif isinstance(e, RESULT_LAST):   # term = f(inputs) - result
        last = v0 + e.principal_width[0] - 1
        row_v[last] = 0
        row_v[last] = M.run_evaluator(e, row_v, row_w, row_c, off)[0]
    else:
        M._satisfy(e, rng, row_v, row_w, row_c, off)


def satisfying_trace(placements, shape, n, seed):
    """(variables, witnesses, constants) of `shape` columns by n rows, canonical: row r carries the
    selector cells of gate r mod len(placements) (distinct leaves of one tree, so every other selector
    is 0) and satisfies every repetition of it."""
    rng = np.random.default_rng(seed)
    v, w, c = (rng.integers(0, P, size=(k, n), dtype=np.uint64) for k in shape)
    for r in range(n):
        pl = placements[r % len(placements)]
        row = [[int(x) for x in a[:, r]] for a in (v, w, c)]
        for level, bit in enumerate(pl.selector_path):
            row[2][level] = int(bit)
        bases, per = pl.bases(), pl.per_chunk_offset.as_tuple()
        for rep in range(pl.num_repetitions):
            satisfy(pl.program.evaluator, rng, *row, tuple(b + rep * p for b, p in zip(bases, per)))
        v[:, r], w[:, r], c[:, r] = row
    return v, w, c
