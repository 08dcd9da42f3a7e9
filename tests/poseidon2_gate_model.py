"""Plain-Python model of the Poseidon2 flattened gate (boojum_amd.gates.Poseidon2FlattenedGate,
csrc/gates_poseidon2.hpp), independent of the evaluator's code:

* `satisfying_row`: from 12 inputs the 130 cells of one instance -- the input, the permutation's
  output, and the state at every "reset" (before the round constant in the full rounds, element 0
  after it in the partial rounds) -- split into variable and witness cells for a given
  num_witness_columns_used;
* `terms`: the 118 terms of one instance in push order, by the structured formulas
  (test_poseidon2_sched's matrices, S-box and constants).  test_poseidon2_gate_cpu.py pins it to
  `evaluator_terms` / `captured_terms`, the evaluator run directly (gates_model.run_evaluator) and its
  capture interpreted (gates_model.interpret: Python has no caps), which are what define the gate;
  the GPU tests use it where thousands of points would make the interpreted capture slow;
* `gate_sum` / `status_record`: a set's sum at every point and its satisfiability record, Poseidon2
  placements through `terms`, every other placement through its evaluator."""
import functools

import gates_model as M
import test_poseidon2_sched as R
import transcript as T

from boojum_amd import gates as G

P = M.P
CELLS, TERMS, SBOX_CELLS = 130, 118, 106
NO_KEY = (1 << 64) - 1


def _full(x, r):
    return R._mds([R._sbox((x[i] + R.RC[r][i]) % P) for i in range(12)])


def permutation_cells(inputs):
    """(the 106 reset cells in the order they are met, the 12 outputs)."""
    x = _full(R._mds([v % P for v in inputs]), 0)
    cells = []
    for r in range(1, 4):
        cells += x
        x = _full(x, r)
    for r in range(4, 26):
        cells.append((x[0] + R.RC[r][0]) % P)
        x[0] = R._sbox(cells[-1])
        x = R._mi(x)
    for r in range(26, 30):
        cells += x
        x = _full(x, r)
    return cells, x


def satisfying_row(inputs, nw):
    """(variables, witnesses) of one instance: 130 - nw and nw cells."""
    cells, out = permutation_cells(inputs)
    assert len(cells) == SBOX_CELLS
    return [v % P for v in inputs] + out + cells[nw:], cells[:nw]


def terms(variables, witnesses, nw, offsets=(0, 0)):
    """The 118 terms of the instance at (variables offset, witnesses offset), in push order."""
    v0, w0 = offsets[0], offsets[1]
    cell = lambda s: (witnesses[w0 + s] if s < nw else variables[v0 + 24 + s - nw]) % P   # noqa: E731
    x = _full(R._mds([variables[v0 + i] % P for i in range(12)]), 0)
    out, s = [], 0
    for r in list(range(1, 4)) + list(range(4, 26)) + list(range(26, 30)):
        if 4 <= r < 26:
            c = cell(s)
            out.append((x[0] + R.RC[r][0] - c) % P)
            x[0] = R._sbox(c)
            x = R._mi(x)
            s += 1
        else:
            c = [cell(s + i) for i in range(12)]
            out += [(x[i] - c[i]) % P for i in range(12)]
            x = _full(c, r)
            s += 12
    return out + [(variables[v0 + 12 + i] - x[i]) % P for i in range(12)]


@functools.lru_cache(maxsize=None)
def captured(ncu, nw):
    """The capture of the evaluator (several thousand relations), shared."""
    return G.capture(G.Poseidon2FlattenedGate(ncu, nw))


def evaluator_terms(evaluator, variables, witnesses, offsets=(0, 0, 0)):
    return M.run_evaluator(evaluator, [v % P for v in variables], [w % P for w in witnesses], [], offsets)


def captured_terms(evaluator, variables, witnesses, offsets=(0, 0, 0)):
    program = captured(evaluator.num_copiable_columns_used, evaluator.num_witness_columns_used)
    return M.interpret(program, [v % P for v in variables], [w % P for w in witnesses], [], offsets)


def placement(nw, reps=1, path=(), initial_offset=None, ncu=None):
    """A general-purpose placement of the gate; the program is the evaluator's stand-in, uncaptured."""
    e = G.Poseidon2FlattenedGate(CELLS - nw if ncu is None else ncu, nw)
    return G.GatePlacement(G.program_of(e), reps, None, path, None, initial_offset)


def _terms_of(pl, v, w, c, off, bases):
    e = pl.program.evaluator
    if isinstance(e, G.Poseidon2FlattenedGate):
        return terms(v, w, e.num_witness_columns_used, off)
    return M.run_evaluator(e, v, w, c, off, bases)


def _instances(pl):
    bases, per = pl.bases(), pl.per_chunk_offset.as_tuple()
    return bases, [tuple(b + rep * p for b, p in zip(bases, per)) for rep in range(pl.num_repetitions)]


def gate_sum(placements, variables, witnesses, constants, alphas, start):
    """start[L] + sum_gates selector sum_rep sum_term alpha[k] term at every point L; the column
    lists hold one list of q * n words each; returns the list of Ext2 values."""
    alphas = [(int(a[0]) % P, int(a[1]) % P) for a in alphas]
    out = []
    for L in range(len(start)):
        v, w, c = ([int(col[L]) % P for col in cols] for cols in (variables, witnesses, constants))
        acc, k = start[L], 0
        for pl in placements:
            gate = M.ZERO
            bases, offs = _instances(pl)
            for off in offs:
                for t in _terms_of(pl, v, w, c, off, bases):
                    gate = T.e_add(gate, M.IntOps.scale(alphas[k], t))
                    k += 1
            if pl.selector_path:
                gate = M.IntOps.scale(gate, M.selector_at(pl.selector_path, c))
            acc = T.e_add(acc, gate)
        out.append(acc)
    return out


def status_record(placements, variables, witnesses, constants, rows=None):
    """[count, smallest row << 32 | k or all ones, that term's value, 0] over (C, n) trace columns."""
    n = len((variables if len(variables) else constants)[0])
    begin, count = rows or (0, n)
    fails = []
    for r in range(begin, begin + count):
        v, w, c = ([int(col[r]) % P for col in cols] for cols in (variables, witnesses, constants))
        k = 0
        for pl in placements:
            sel = M.selector_at(pl.selector_path, c)
            bases, offs = _instances(pl)
            for off in offs:
                for t in _terms_of(pl, v, w, c, off, bases):
                    if sel * t % P:
                        fails.append((r << 32 | k, t))
                    k += 1
    if not fails:
        return [0, NO_KEY, 0, 0]
    key, value = min(fails)
    return [len(fails), key, value, 0]
