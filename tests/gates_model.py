"""Plain-Python model of the quotient's gate terms (boojum_amd/gates.py, csrc/gates.hip):

* `interpret`: the relation IR (gpu_synthesizer/mod.rs:113-133) on Python integers, or on Ext2
  pairs for a point off the domain;
* `selector_at`: compute_selector_subpath (prover.rs:2775-2916) at one point;
* `gate_terms_at` / `gate_terms`: acc += sum_gates selector_g sum_rep sum_term alpha[k] term, k
  running on across repetitions and gates and restarting per point (buffering_source.rs:157-221,
  303-377; cs/traits/evaluator.rs:376-397; prover.rs:651-801 for the form without a selector);
* `direct_terms_at`: the same sum with the evaluators run directly on field-like values, which
  is the verifier's use of them (verifier.rs:215-271);
* `satisfiable_circuit`: a small circuit over four gate kinds under a selector tree, with a trace
  whose rows satisfy the gate selected on them, the setup constants (selector columns first) and
  a sigma that links equal cells; stage 2 and the LDE come from stage2_model and quotient_model.

Base values are Python integers mod P, Ext2 values (c0, c1) tuples (oracle/transcript.py)."""
import numpy as np

import quotient_model as Q
import stage2_model as S
import transcript as T

from boojum_amd import gates as G

P = T.P
ZERO = (0, 0)


# ------------------------------------------------------------------ arithmetic the IR runs on
class IntOps:
    const = staticmethod(lambda v: v % P)
    add = staticmethod(lambda a, b: (a + b) % P)
    sub = staticmethod(lambda a, b: (a - b) % P)
    mul = staticmethod(lambda a, b: a * b % P)
    scale = staticmethod(lambda alpha, v: (alpha[0] * v % P, alpha[1] * v % P))   # Ext2 challenge * base term


class ExtOps:
    const = staticmethod(lambda v: (v % P, 0))
    add = staticmethod(T.e_add)
    sub = staticmethod(T.e_sub)
    mul = staticmethod(T.e_mul)
    scale = staticmethod(T.e_mul)


class ModelField:
    """A field-like with TracingField's surface that computes: the evaluators of boojum_amd.gates
    run over it unchanged."""

    def __init__(self, value, ops=IntOps):
        self.v, self.ops = value, ops

    def copy(self):
        return ModelField(self.v, self.ops)

    def zero(self):
        return ModelField(self.ops.const(0), self.ops)

    def one(self):
        return ModelField(self.ops.const(1), self.ops)

    def minus_one(self):
        return ModelField(self.ops.const(P - 1), self.ops)

    def constant(self, value):
        return ModelField(self.ops.const(value), self.ops)

    def add_assign(self, other):
        self.v = self.ops.add(self.v, other.v)
        return self

    def sub_assign(self, other):
        self.v = self.ops.sub(self.v, other.v)
        return self

    def mul_assign(self, other):
        self.v = self.ops.mul(self.v, other.v)
        return self

    def double(self):
        self.v = self.ops.add(self.v, self.v)
        return self

    def negate(self):
        self.v = self.ops.sub(self.ops.const(0), self.v)
        return self

    def square(self):
        self.v = self.ops.mul(self.v, self.v)
        return self

    def mul_by_base(self, value):
        self.v = self.ops.mul(self.v, self.ops.const(value))
        return self

    def mul_and_accumulate_into(self, a, b):
        self.v = self.ops.add(self.v, self.ops.mul(a.v, b.v))
        return self


class ModelSource:
    """A row (or point) as a TraceSource: the three value lists with the gate's bases and the
    repetition's offset (BufferingPolyStorage, buffering_source.rs:54-126)."""

    def __init__(self, variables, witnesses, constants, offsets=(0, 0, 0), ops=IntOps):
        self.cols, self.off, self.ops = (variables, witnesses, constants), offsets, ops

    def _get(self, kind, i):
        return ModelField(self.cols[kind][self.off[kind] + i], self.ops)

    def get_variable_value(self, i):
        return self._get(0, i)

    def get_witness_value(self, i):
        return self._get(1, i)

    def get_constant_value(self, i):
        return self._get(2, i)

    def field(self):
        return ModelField(self.ops.const(0), self.ops)


class ModelDestination:
    def __init__(self):
        self.terms = []

    def push_evaluation_result(self, value):
        self.terms.append(value.v)


def run_evaluator(evaluator, variables, witnesses, constants, offsets=(0, 0, 0), shared_offsets=None, ops=IntOps):
    """evaluate_once on values: the terms in push order.  The row-shared constants are loaded at
    shared_offsets (default: offsets), as the reference loads them before the repetitions."""
    shared = evaluator.load_row_shared_constants(
        ModelSource(variables, witnesses, constants, shared_offsets or offsets, ops))
    dst = ModelDestination()
    evaluator.evaluate_once(ModelSource(variables, witnesses, constants, offsets, ops), dst, shared)
    return dst.terms


# ------------------------------------------------------------------ the IR
_KIND = {"VariablePoly": 0, "WitnessPoly": 1, "ConstantPoly": 2}


def interpret(program, variables, witnesses, constants, offsets=(0, 0, 0), ops=IntOps):
    """The terms of one repetition of a captured program, in push order."""
    cols = (variables, witnesses, constants)
    temps = {}

    def value(o):
        if o.kind == "TemporaryValue":
            return temps[o.value]
        if o.kind == "ConstantValue":
            return ops.const(o.value)
        k = _KIND[o.kind]
        return cols[k][offsets[k] + o.value]

    for dst, rel in program.relations:
        a = value(rel.operands[0])
        kind = rel.kind
        if kind == "Add":
            r = ops.add(a, value(rel.operands[1]))
        elif kind == "Sub":
            r = ops.sub(a, value(rel.operands[1]))
        elif kind == "Mul":
            r = ops.mul(a, value(rel.operands[1]))
        elif kind == "Double":
            r = ops.add(a, a)
        elif kind == "Negate":
            r = ops.sub(ops.const(0), a)
        elif kind == "Square":
            r = ops.mul(a, a)
        else:
            raise ValueError("Relation.%s is not evaluated" % kind)
        assert dst not in temps
        temps[dst] = r
    return [value(o) for o in program.writes]


def selector_at(path, constants, ops=IntOps):
    """prod_i (constants[i] if path[i] else 1 - constants[i]); an empty path is one."""
    sel = ops.const(1)
    for i, bit in enumerate(path):
        f = constants[i] if bit else ops.sub(ops.const(1), constants[i])
        sel = ops.mul(sel, f)
    return sel


def _sum_terms(placements, variables, witnesses, constants, alphas, ops, terms_of):
    acc, k = ZERO, 0
    for pl in placements:
        gate = ZERO
        bases, per = pl.bases(), pl.per_chunk_offset.as_tuple()
        for rep in range(pl.num_repetitions):
            off = tuple(b + rep * p for b, p in zip(bases, per))
            for t in terms_of(pl, off, bases):
                gate = T.e_add(gate, ops.scale(alphas[k], t))
                k += 1
        if pl.selector_path:
            sel = selector_at(pl.selector_path, constants, ops)
            gate = ops.scale(gate, sel) if ops is IntOps else T.e_mul(gate, sel)
        acc = T.e_add(acc, gate)
    return acc, k


def gate_terms_at(placements, variables, witnesses, constants, alphas, ops=IntOps):
    """The gate sum at one point from the captured programs; returns (Ext2 value, challenges used)."""
    return _sum_terms(placements, variables, witnesses, constants, alphas, ops,
                      lambda pl, off, bases: interpret(pl.program, variables, witnesses, constants, off, ops))


def direct_terms_at(placements, variables, witnesses, constants, alphas, ops=IntOps):
    """The same sum with each placement's evaluator run directly on the values."""
    return _sum_terms(placements, variables, witnesses, constants, alphas, ops,
                      lambda pl, off, bases: run_evaluator(pl.program.evaluator, variables, witnesses, constants, off,
                                                           bases, ops))


def gate_terms(placements, variables_lde, witnesses_lde, constants_lde, alphas, start=None):
    """Over the domain: *_lde are lists of leaf-order columns; returns the list of Ext2 values
    start[L] + gate sum at L."""
    alphas = [(int(a[0]) % P, int(a[1]) % P) for a in alphas]
    total = len((variables_lde or constants_lde or witnesses_lde)[0])
    out = []
    for L in range(total):
        v = [int(c[L]) for c in variables_lde]
        w = [int(c[L]) for c in witnesses_lde]
        c = [int(col[L]) for col in constants_lde]
        s, used = gate_terms_at(placements, v, w, c, alphas)
        assert used == sum(pl.num_terms() for pl in placements)
        out.append(T.e_add(start[L], s) if start is not None else s)
    return out


def total_terms(placements):
    return sum(pl.num_terms() for pl in placements)


# ------------------------------------------------------------------ programs the tests add
class PowerSumEvaluator(G.Evaluator):
    """Not a gate of the reference: it exists to exercise Double, Negate, Square, mul_by_base, a
    bare column and a ConstantValue as written operands, Mul(x, x) and the constants 0, 1 and
    p - 1.  Terms: 2 a - (-(b^2)) * 3 + w, a * a, a, 5, (a + 0) * 1 * (p - 1)."""
    name = "power_sum"
    num_quotient_terms = 5
    principal_width = (2, 1, 0)

    def evaluate_once(self, src, dst, shared):
        a, b, w = src.get_variable_value(0), src.get_variable_value(1), src.get_witness_value(0)
        t = a.copy()
        t.double()
        s = b.copy()
        s.square()
        s.negate()
        s.mul_by_base(3)
        t.sub_assign(s)
        t.add_assign(w)
        dst.push_evaluation_result(t)
        x = a.copy()
        x.mul_assign(a)
        dst.push_evaluation_result(x)
        dst.push_evaluation_result(a)
        dst.push_evaluation_result(src.field().constant(5))
        y = a.copy()
        y.add_assign(src.field().zero())
        y.mul_assign(src.field().one())
        y.mul_assign(src.field().minus_one())
        dst.push_evaluation_result(y)


def chain_program(length, live=3):
    """`length` temporaries of which `live` are live at once: t_i = t_{i-1} * t_{i-live}."""
    rel = [(0, G.Relation.Add(G.Index.VariablePoly(0), G.Index.ConstantValue(1)))]
    for i in range(1, length):
        back = G.Index.TemporaryValue(max(0, i - live))
        rel.append((i, G.Relation.Mul(G.Index.TemporaryValue(i - 1), back)))
    return G.GateProgram(rel, [G.Index.TemporaryValue(length - 1)], 1)


def wide_program(width):
    """`width` temporaries all live at the end."""
    rel = [(i, G.Relation.Add(G.Index.VariablePoly(0), G.Index.ConstantValue(i))) for i in range(width)]
    acc = width
    rel.append((acc, G.Relation.Add(G.Index.TemporaryValue(0), G.Index.TemporaryValue(1))))
    for i in range(2, width):
        rel.append((acc + 1, G.Relation.Add(G.Index.TemporaryValue(acc), G.Index.TemporaryValue(i))))
        acc += 1
    return G.GateProgram(rel, [G.Index.TemporaryValue(acc)], 1)


# ------------------------------------------------------------------ a satisfiable circuit
class Circuit:
    pass


def _satisfy(evaluator, rng, row_v, row_w, row_c, off):
    """Fills one repetition's cells of a row so that the evaluator's terms vanish."""
    r = lambda: int(rng.integers(0, P, dtype=np.uint64))  # noqa: E731
    v0, w0, c0 = off
    if isinstance(evaluator, G.FmaGateInBaseFieldWithoutConstant):
        a, b, c = r(), r(), r()
        row_v[v0:v0 + 4] = [a, b, c, (row_c[c0] * a % P * b + row_c[c0 + 1] * c) % P]
    elif isinstance(evaluator, G.ZeroCheckGate):
        inp = r() if rng.integers(0, 2) else 0
        flag = 1 if inp == 0 else 0
        inv = pow(inp, P - 2, P) if inp else r()
        row_v[v0:v0 + 2] = [inp, flag]
        if evaluator.use_witness_column_for_inversion:
            row_w[w0] = inv
        else:
            row_v[v0 + 2] = inv
    elif isinstance(evaluator, G.ConstantsAllocatorGate):
        row_v[v0] = row_c[c0]
    elif isinstance(evaluator, G.ConditionalSwapGate):
        s, a, b = int(rng.integers(0, 2)), r(), r()
        row_v[v0:v0 + 5] = [s, a, b, b if s else a, a if s else b]
    else:
        raise NotImplementedError(evaluator.name)


def sigma_for(w, log_n):
    """A sigma under which w satisfies the copy permutation: the cells of equal value form one
    cycle each (stage2_model.valid_inputs builds the values from the cycles; here the values come
    first)."""
    n_cols, n = w.shape
    k, x = S.non_residues_for_copy_permutation(n, n_cols), S.domain(log_n)
    groups = {}
    for cell, value in enumerate(w.reshape(-1)):
        groups.setdefault(int(value), []).append(cell)
    sigma = np.zeros(n_cols * n, dtype=np.uint64)
    for cells in groups.values():
        for i, cell in enumerate(cells):
            image = cells[(i + 1) % len(cells)]
            sigma[cell] = k[image // n] * x[image % n] % P
    return sigma.reshape(n_cols, n)


def satisfiable_circuit(log_n=3, seed=7):
    """Four gate kinds on 8 variable columns, 1 witness column and 5 constant columns, row i of the
    trace (natural order) running gate i mod 4:
      FMA x 2                 path [1]        own constants in columns 1, 2 (shared by the repetitions)
      ZeroCheck(witness) x 1  path [0, 1]
      ConstantsAllocator x 2  path [0, 0, 1]  own constants in columns 3 and 4, one per repetition
      ConditionalSwap<1> x 1  path [0, 0, 0]
    Constraint degree + path length is at most 5, so the quotient degree is 4."""
    n = 1 << log_n
    rng = np.random.default_rng(seed)
    kinds = [(G.FmaGateInBaseFieldWithoutConstant(), [True], 2), (G.ZeroCheckGate(True), [False, True], 1),
             (G.ConstantsAllocatorGate(), [False, False, True], 2), (G.ConditionalSwapGate(1), [False, False, False], 1)]
    c = Circuit()
    c.log_n, c.log_q, c.n_vars, c.n_wits, c.n_consts = log_n, 2, 8, 1, 5
    c.placements = [G.GatePlacement(G.capture(e), reps, e.per_chunk_offset, path) for e, path, reps in kinds]
    c.variables = rng.integers(0, P, size=(c.n_vars, n), dtype=np.uint64)
    c.witnesses = rng.integers(0, P, size=(c.n_wits, n), dtype=np.uint64)
    c.constants = rng.integers(0, P, size=(c.n_consts, n), dtype=np.uint64)
    c.gate_of_row = [i % len(kinds) for i in range(n)]
    for i in range(n):
        pl = c.placements[c.gate_of_row[i]]
        row_v = [int(v) for v in c.variables[:, i]]
        row_w = [int(v) for v in c.witnesses[:, i]]
        row_c = [int(v) for v in c.constants[:, i]]
        for level, bit in enumerate(pl.selector_path):
            row_c[level] = int(bit)
        bases, per = pl.bases(), pl.per_chunk_offset.as_tuple()
        for rep in range(pl.num_repetitions):
            _satisfy(pl.program.evaluator, rng, row_v, row_w, row_c, tuple(b + rep * p for b, p in zip(bases, per)))
        c.variables[:, i], c.witnesses[:, i], c.constants[:, i] = row_v, row_w, row_c
    c.sigma = sigma_for(c.variables, log_n)
    return c


def circuit_quotient(c, beta, gamma, gate_alphas, cp_alphas, variables=None):
    """The whole block for a circuit: the LDEs, the gate terms, then quotient_model.quotient with
    them as the accumulator's start.  variables: a replacement trace (a corrupted one)."""
    w = c.variables if variables is None else variables
    r = Circuit()
    r.wit_lde = [Q.coset_lde(col, c.log_q) for col in c.witnesses]
    r.const_lde = [Q.coset_lde(col, c.log_q) for col in c.constants]
    var_lde = [Q.coset_lde(col, c.log_q) for col in w]
    r.gate_terms = gate_terms(c.placements, var_lde, r.wit_lde, r.const_lde, gate_alphas)
    r.q = Q.quotient(w, c.sigma, beta, gamma, c.log_q, cp_alphas, start=r.gate_terms)
    return r
