"""The two small satisfiable circuits of the prover tests (boojum_amd/prover.py), as the data
`prepare_setup` and `prove` take: placements, constant columns, dense copy hints, lookup tables,
and WitnessVecs.  Everything here is host data; nothing needs a device.

Both run, on the 8 general-purpose variable columns, the four gate kinds of
gates_model.satisfiable_circuit under its selector tree (row i runs gate i mod 4; FMA x 2 under
[1] with its coefficients in constants 1 and 2, ZeroCheck with a witness column under [0, 1],
ConstantsAllocator x 2 under [0, 0, 1] with constants 3 and 4, ConditionalSwap<1> under [0, 0, 0]),
so num_constant_columns = 2 and extra_constant_polys_for_selectors = 3, and one
ConstantsAllocator over specialized columns on every row.

  A  no lookup.  The specialized gate once: variable column 8, constant 5.
     V = 9, W = 1, C = 6, I = 2.
  B  a width-3 lookup over specialized columns, two repetitions (variable columns 8..13), the table
     id in constant column 5 (num_constant_columns + extra, setup.rs:964-988), one table of n rows
     with id 7; the specialized gate three times: variable columns 14..16, constants 6..8.
     V = 17, W = 1, C = 9, M = 1, L = 2, I = 4, four table columns.

The numbers of variable columns are the first that give their I, which makes the geometry that
oracle/transcript.py's `geometries` finds for B unique.

The hints are structural, not by value: every cell a gate uses names a fresh variable, except the
swap gate's outputs, which name its inputs (the swap bit of a row belongs to the circuit), and
column 5 of every ZeroCheck row, which no gate reads there and which names the variable of column 0
of the row above.  Unused cells are placeholders.  So one circuit has many witnesses (`witness`),
and a cell can be re-pointed at another variable without breaking a gate (`broken_copy_hint`).

Public inputs: (0, 0) and (3, 0) in one row, (1, 7) in another."""
import numpy as np

import gates_model as M
import transcript as T

from boojum_amd import gates as G
from boojum_amd import openings, stage2, witness as W

P = T.P
LOG_N = 10
N = 1 << LOG_N
LDE_FACTOR, QUOTIENT_DEGREE, CAP, SECURITY = 2, 4, 4, 8
PUBLIC_INPUTS = [(0, 0), (3, 0), (1, 7)]
GENERAL = dict(num_columns_under_copy_permutation=8, num_witness_columns=1, num_constant_columns=2,
               max_allowed_constraint_degree=4)
EXTRA_SELECTORS = 3
GENERAL_CONSTANTS = GENERAL["num_constant_columns"] + EXTRA_SELECTORS
TABLE_ID = 7
LOOKUP = stage2.LookupParameters("constant", 3, 2)
PH = W.placeholder()


class Case:
    """kind "A" or "B".  placements_general, placements_specialized, set_order (specialized first:
    the order of the uploaded set and of the challenges); layout; constants (C, n); tables
    (4, n) or None; variables_maps (V, n), witness_maps (1, n) uint64 hint words."""

    def __init__(self, kind, seed=11, log_n=LOG_N):
        assert kind in "AB"
        self.kind, self.log_n, self.n = kind, log_n, 1 << log_n
        n = self.n
        rng = np.random.default_rng(seed)
        self.lookup = LOOKUP if kind == "B" else None
        self.lookup_first = GENERAL["num_columns_under_copy_permutation"]
        lookup_cols = 6 if kind == "B" else 0
        self.spec_reps = 3 if kind == "B" else 1
        self.spec_var0 = self.lookup_first + lookup_cols
        self.spec_const0 = GENERAL_CONSTANTS + (1 if kind == "B" else 0)
        v, c = self.spec_var0 + self.spec_reps, self.spec_const0 + self.spec_reps
        self.layout = openings.OpeningLayout(
            V=v, W=1, C=c, M=1 if kind == "B" else 0, L=2 if kind == "B" else 0,
            I=stage2.num_intermediate_partial_product_relations(v, QUOTIENT_DEGREE),
            lookup_setups=4 if kind == "B" else 0, quotient_degree=QUOTIENT_DEGREE)
        kinds = [(G.FmaGateInBaseFieldWithoutConstant(), [True], 2), (G.ZeroCheckGate(True), [False, True], 1),
                 (G.ConstantsAllocatorGate(), [False, False, True], 2),
                 (G.ConditionalSwapGate(1), [False, False, False], 1)]
        self.placements_general = [G.GatePlacement(G.capture(e), reps, e.per_chunk_offset, path)
                                   for e, path, reps in kinds]
        self.placements_specialized = [G.specialized_placement(
            G.ConstantsAllocatorGate(), self.spec_reps, False,
            G.PerChunkOffset(self.spec_var0, 0, self.spec_const0 - GENERAL_CONSTANTS), GENERAL_CONSTANTS)]
        self.set_order = self.placements_specialized + self.placements_general
        self.gate_of_row = [i % 4 for i in range(n)]
        # constants: selector bits on the path, random words elsewhere, the table id column
        self.constants = rng.integers(0, P, size=(c, n), dtype=np.uint64)
        for i in range(n):
            for level, bit in enumerate(self.placements_general[self.gate_of_row[i]].selector_path):
                self.constants[level, i] = int(bit)
        self.swap_bit = rng.integers(0, 2, size=n)
        self.tables = None
        if kind == "B":
            self.constants[GENERAL_CONSTANTS] = TABLE_ID
            self.tables = rng.integers(0, P, size=(4, n), dtype=np.uint64)
            self.tables[3] = TABLE_ID
        # the hints
        idx = -np.ones((v, n), dtype=np.int64)
        widx = -np.ones((1, n), dtype=np.int64)
        fresh = iter(range(1 << 40))
        used = {0: range(8), 1: range(2), 2: range(2), 3: range(3)}
        for i in range(n):
            g = self.gate_of_row[i]
            for col in used[g]:
                idx[col, i] = next(fresh)
            if g == 3:
                s = self.swap_bit[i]
                idx[3, i], idx[4, i] = (idx[2, i], idx[1, i]) if s else (idx[1, i], idx[2, i])
            if g == 1:
                widx[0, i] = next(fresh)
                idx[5, i] = idx[0, i - 1]
            for col in range(self.lookup_first, v):
                idx[col, i] = next(fresh)
        self.num_values = next(fresh)
        self.var_idx, self.wit_idx = idx, widx
        self.variables_maps = np.where(idx < 0, np.uint64(PH), idx.astype(np.uint64))
        self.witness_maps = np.where(widx < 0, np.uint64(PH), widx.astype(np.uint64))

    # -------------------------------------------------------------- witnesses
    def witness(self, seed):
        """A satisfying assignment: (WitnessVec, variables (V, n), witnesses (1, n)), the two arrays
        being what the hints materialise from the vector."""
        rng = np.random.default_rng(1000 + seed)
        n, g = self.n, self.layout
        var = np.zeros((g.V, n), dtype=np.uint64)
        wit = np.zeros((1, n), dtype=np.uint64)
        mult = np.zeros(n, dtype=np.uint32)
        r = lambda: int(rng.integers(0, P, dtype=np.uint64))   # noqa: E731
        for i in range(n):
            pl = self.placements_general[self.gate_of_row[i]]
            row_v = [int(x) for x in var[:, i]]
            row_w = [int(x) for x in wit[:, i]]
            row_c = [int(x) for x in self.constants[:, i]]
            if self.gate_of_row[i] == 3:
                s, a, b = int(self.swap_bit[i]), r(), r()
                row_v[0:5] = [s, a, b, b if s else a, a if s else b]
            else:
                bases, per = pl.bases(), pl.per_chunk_offset.as_tuple()
                for rep in range(pl.num_repetitions):
                    M._satisfy(pl.program.evaluator, rng, row_v, row_w, row_c,
                               tuple(b + rep * p for b, p in zip(bases, per)))
            if self.gate_of_row[i] == 1:
                row_v[5] = int(var[0, i - 1])
            if self.kind == "B":
                for s in range(2):
                    t = int(rng.integers(0, n))
                    mult[t] += 1
                    first = self.lookup_first + 3 * s
                    row_v[first:first + 3] = [int(x) for x in self.tables[:3, t]]
            for rep in range(self.spec_reps):
                row_v[self.spec_var0 + rep] = row_c[self.spec_const0 + rep]
            var[:, i], wit[:, i] = row_v, row_w
        values = np.zeros(self.num_values, dtype=np.uint64)
        for cells, index in ((var, self.var_idx), (wit, self.wit_idx)):
            keep = index >= 0
            values[index[keep]] = cells[keep]
        # the structure holds: every cell carries its variable's value
        for cells, index in ((var, self.var_idx), (wit, self.wit_idx)):
            assert np.array_equal(np.where(index >= 0, values[np.maximum(index, 0)], 0), cells)
        vec = W.WitnessVec(PUBLIC_INPUTS, values, mult if self.kind == "B" else [])
        return vec, var, wit

    def broken_copy_hint(self):
        """The variables hint with cell (5, 1) -- unused by the gate of its row, a copy of (0, 0) --
        naming the variable of (1, 0) instead: consistent as a hint, every gate still satisfied,
        the copy constraint the setup's sigmas hold broken."""
        maps = self.variables_maps.copy()
        assert self.var_idx[5, 1] == self.var_idx[0, 0] and self.var_idx[1, 0] not in (-1, self.var_idx[0, 0])
        maps[5, 1] = np.uint64(self.var_idx[1, 0])
        return maps

    # -------------------------------------------------------------- the calls
    def config(self, P_):
        return P_.ProofConfig(LDE_FACTOR, CAP, SECURITY)

    def setup_arguments(self, P_, **over):
        kw = dict(constants=self.constants, variables_hint=W.DenseVariablesCopyHint(self.variables_maps),
                  witness_hint=W.DenseWitnessCopyHint(self.witness_maps), gates=self.placements_general,
                  specialized_gates=self.placements_specialized, lookup_tables=self.tables,
                  lookup_parameters=self.lookup, public_inputs_locations=PUBLIC_INPUTS, layout=self.layout,
                  config=self.config(P_), parameters=G.CSGeometry(**GENERAL))
        kw.update(over)
        return kw

    def prepare(self, P_, **over):
        return P_.prepare_setup(**self.setup_arguments(P_, **over))


def fixture_of(setup, proof):
    """What oracle.transcript.replay takes: the vk and the proof's JSON, with the `queries` alias
    of the reference's fixture."""
    fx = dict(vk=setup.vk, **proof.to_json())
    fx["queries"] = fx["queries_per_fri_repetition"]
    return fx
