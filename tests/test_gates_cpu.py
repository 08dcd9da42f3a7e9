"""The gate-program layer without a GPU (boojum_amd/gates.py, tests/gates_model.py and the
library's host-side validator bj_gate_set_check_h): capture against direct evaluation, coverage of
the IR, slot allocation, the challenge index, a satisfiable circuit through the whole quotient
model, and the rejection of malformed images."""
import functools

import numpy as np
import pytest

import gates_model as M
import quotient_model as Q

from boojum_amd import BoojumError
from boojum_amd import gates as G

P = M.P
BETA, GAMMA = (0x1234567890ABCDEF % P, 0x0FEDCBA987654321), (0xDEADBEEFCAFEF00D % P, 0x1122334455667788)
AT = (0x0123456789ABCDEF, 0x0FEDCBA987654321 % P)


def challenges(count, seed):
    return [tuple(int(v) for v in pair) for pair in
            np.random.default_rng(2000 + seed).integers(0, P, size=(count, 2), dtype=np.uint64)]


PowerSumEvaluator, chain_program, wide_program = M.PowerSumEvaluator, M.chain_program, M.wide_program
EVALUATORS = G.library() + [PowerSumEvaluator()]


# ------------------------------------------------------------------ capture
@pytest.mark.parametrize("evaluator", EVALUATORS, ids=lambda e: e.name)
def test_captured_program_equals_direct_evaluation(evaluator):
    program = G.capture(evaluator)
    assert len(program.writes) == evaluator.num_quotient_terms
    rng = np.random.default_rng(5)
    nv, nw, nc = (x + 3 for x in evaluator.principal_width)
    for trial in range(8):
        v, w, c = ([int(x) for x in rng.integers(0, P, size=k, dtype=np.uint64)] for k in (nv, nw, nc))
        off = (trial % 3, trial % 2, 0)
        assert M.interpret(program, v, w, c, off) == M.run_evaluator(evaluator, v, w, c, off)


def test_library_terms_vanish_on_satisfying_rows():
    """The restated evaluators are the gates they claim to be: c0 a b + c1 c = d and a (1 - a)."""
    a, b, c, c0, c1 = 3, 5, 7, 11, 13
    assert M.run_evaluator(G.FmaGateInBaseFieldWithoutConstant(), [a, b, c, (c0 * a * b + c1 * c) % P], [],
                           [c0, c1]) == [0]
    assert M.run_evaluator(G.BooleanConstraintGate(), [1], [], []) == [0]
    assert M.run_evaluator(G.BooleanConstraintGate(), [2], [], []) == [P - 2]
    assert M.run_evaluator(G.ReductionGate(4), [1, 2, 3, 4, 30], [], [1, 2, 3, 4]) == [0]
    assert M.run_evaluator(G.SelectionGate(), [8, 9, 1, 8], [], []) == [0]
    assert M.run_evaluator(G.SelectionGate(), [8, 9, 0, 9], [], []) == [0]
    assert M.run_evaluator(G.DotProductGate(4), [1, 2, 3, 4, 5, 6, 7, 8, 100], [], []) == [0]
    assert M.run_evaluator(G.ZeroCheckGate(False), [0, 1, 9], [], []) == [0, 0]
    assert M.run_evaluator(G.ZeroCheckGate(True), [4, 0], [pow(4, P - 2, P)], []) == [0, 0]
    assert M.run_evaluator(G.ConditionalSwapGate(1), [1, 5, 6, 6, 5], [], []) == [0, 0]


def test_every_relation_and_index_kind_is_covered():
    relations, kinds = set(), set()
    for e in EVALUATORS:
        program = G.capture(e)
        for _, rel in program.relations:
            relations.add(rel.kind)
            kinds.update(o.kind for o in rel.operands)
        kinds.update(o.kind for o in program.writes)
    assert relations == {"Add", "Double", "Sub", "Negate", "Mul", "Square"}
    assert kinds == {"VariablePoly", "WitnessPoly", "ConstantPoly", "TemporaryValue", "ConstantValue"}


def test_geometry_counts():
    """num_repetitions_in_geometry at the reference proof's geometry (130 copiable columns)."""
    geo = G.CSGeometry(130, 4, 8, 8)
    reps = {e.name: e.num_repetitions_in_geometry(geo) for e in G.library()}
    assert reps == {"fma_gate_in_base_without_constant": 32, "boolean_constraint": 130, "constants_allocator": 8,
                    "reduction_gate_4": 26, "selection_gate": 32, "zero_check_variable": 43, "zero_check_witness": 4,
                    "dot_product_gate_4": 14, "conditional_swap_gate_1": 26}


# ------------------------------------------------------------------ slots
def check_allocation(program, slots):
    """Replays the program on slot contents: every read must find the temporary it names."""
    holds, slot_of = {}, {}
    for (dst, rel), s in zip(program.relations, slots):
        for o in rel.operands:
            if o.kind == "TemporaryValue":
                assert holds[slot_of[o.value]] == o.value, "slot reused while TemporaryValue(%d) is live" % o.value
        holds[s] = dst
        slot_of[dst] = s
    for o in program.writes:
        if o.kind == "TemporaryValue":
            assert holds[slot_of[o.value]] == o.value, "a pushed temporary was overwritten"


@pytest.mark.parametrize("program", [G.capture(e) for e in EVALUATORS] + [chain_program(300), wide_program(16)],
                         ids=lambda p: p.evaluator.name if p.evaluator else "synthetic")
def test_slots_are_never_reused_while_live(program):
    slots, used = G.allocate_slots(program)
    assert used <= G.MAX_SLOTS and max(slots) < used
    check_allocation(program, slots)


def test_chain_of_300_temporaries_needs_three_slots():
    slots, used = G.allocate_slots(chain_program(300, live=3))
    assert used == 3
    x = 12345
    temps = [x + 1]
    for i in range(1, 300):
        temps.append(temps[-1] * temps[max(0, i - 3)] % P)
    assert M.interpret(chain_program(300, live=3), [x], [], []) == [temps[-1]]


def test_too_many_live_values_are_rejected():
    G.allocate_slots(wide_program(G.MAX_SLOTS))
    with pytest.raises(ValueError):
        G.allocate_slots(wide_program(G.MAX_SLOTS + 1))
    with pytest.raises(ValueError):
        G.compile_gate_set([G.GatePlacement(wide_program(G.MAX_SLOTS + 1))])
    with pytest.raises(ValueError):   # read before written
        G.allocate_slots(G.GateProgram([(0, G.Relation.Double(G.Index.TemporaryValue(1)))],
                                       [G.Index.TemporaryValue(0)], 1))


# ------------------------------------------------------------------ the challenge index
def test_challenge_index_runs_on_and_restarts_per_point():
    """Two gates, 3 and 2 repetitions, 2 and 1 terms: challenge k multiplies term k of the point in
    the order gate, repetition, push; a unit challenge at k picks out exactly that term."""
    zc, bc = G.ZeroCheckGate(False), G.BooleanConstraintGate()
    pls = [G.GatePlacement(G.capture(zc), 3), G.GatePlacement(G.capture(bc), 2)]
    assert M.total_terms(pls) == 8
    rng = np.random.default_rng(9)
    points = [[int(x) for x in rng.integers(0, P, size=9, dtype=np.uint64)] for _ in range(2)]
    for v in points:
        expect = []
        for rep in range(3):
            expect += M.run_evaluator(zc, v, [], [], (3 * rep, 0, 0))
        for rep in range(2):
            expect += M.run_evaluator(bc, v, [], [], (rep, 0, 0))
        for k in range(8):
            unit = [(0, 0)] * 8
            unit[k] = (1, 0)
            got, used = M.gate_terms_at(pls, v, [], [], unit)
            assert used == 8 and got == (expect[k], 0)
    image = G.compile_gate_set(pls)
    assert G.check_image(image) == dict(variables=9, witnesses=0, constants=0, alphas=8, segments=1)


def test_segments_carry_the_challenge_index():
    pl = G.GatePlacement(chain_program(300), 2)
    image = G.compile_gate_set([pl] * 30)   # 9000 instructions: 13 gates fit the 4096 of a launch
    need = G.check_image(image)
    assert need["segments"] == 3 and need["alphas"] == 60
    bases = [image[image[2 + s] + 4] for s in range(3)]
    assert bases == [0, 26, 52]


# ------------------------------------------------------------------ the satisfiable circuit
@functools.lru_cache(maxsize=None)
def circuit_case():
    c = M.satisfiable_circuit()
    gate_alphas = challenges(M.total_terms(c.placements), 1)
    cp_alphas = challenges(c.n_vars // 4 + 1, 2)
    return c, gate_alphas, cp_alphas, M.circuit_quotient(c, BETA, GAMMA, gate_alphas, cp_alphas)


def test_circuit_rows_satisfy_their_gates():
    c, _, _, _ = circuit_case()
    for i, g in enumerate(c.gate_of_row):
        row = [[int(v) for v in a[:, i]] for a in (c.variables, c.witnesses, c.constants)]
        for j, pl in enumerate(c.placements):
            assert M.selector_at(pl.selector_path, row[2]) == (1 if j == g else 0)
        ones = [(1, 0)] * M.total_terms(c.placements)
        assert M.gate_terms_at(c.placements, *row, ones)[0] == (0, 0)


def test_gate_terms_and_copy_permutation_divide_by_the_vanishing_polynomial():
    c, _, _, r = circuit_case()
    assert r.q.cp.zeros == 0 and r.q.cp.total == (1, 0)
    q = 1 << c.log_q
    assert any(v != (0, 0) for v in r.gate_terms)
    for half in r.q.mono:
        assert half[-q:] == [0] * q


def test_gate_sum_at_a_point_off_the_domain_is_the_verifiers():
    c, gate_alphas, _, _ = circuit_case()
    at = [[Q.horner(Q.monomials([int(v) for v in col]), AT) for col in a]
          for a in (c.variables, c.witnesses, c.constants)]
    model, used = M.gate_terms_at(c.placements, *at, gate_alphas, ops=M.ExtOps)
    direct, _ = M.direct_terms_at(c.placements, *at, gate_alphas, ops=M.ExtOps)
    assert used == len(gate_alphas) and model == direct and model != (0, 0)


def test_a_corrupted_cell_leaves_a_remainder():
    c, gate_alphas, cp_alphas, _ = circuit_case()
    bad = c.variables.copy()
    bad[3, 0] = (int(bad[3, 0]) + 1) % P   # d of the first FMA on row 0, a value of its own cycle
    r = M.circuit_quotient(c, BETA, GAMMA, gate_alphas, cp_alphas, variables=bad)
    assert r.q.cp.total == (1, 0)          # the copy permutation still holds: the gate is what fails
    assert r.q.mono[0][-1] != 0 or r.q.mono[1][-1] != 0


# ------------------------------------------------------------------ the library's validator
def good_image():
    return G.compile_gate_set([G.GatePlacement(G.capture(G.FmaGateInBaseFieldWithoutConstant()), 2, None, [True]),
                               G.GatePlacement(G.capture(PowerSumEvaluator()), 1, None, [False, True])])


def segment(image):
    return image[2]


def test_validator_accepts_and_reports_needs():
    need = G.check_image(good_image())
    assert need == dict(variables=8, witnesses=1, constants=3, alphas=7, segments=1)


def mutations():
    s = 3   # one segment: its header starts at word 3
    instr0 = s + 8 + 2 * 8

    def patch(at, value):
        def f(image):
            image[at] = value
        return f

    def inverse(image):
        image[instr0] = (image[instr0] & ~0xff) | 6

    def slot_over_cap(image):
        image[instr0] = (image[instr0] & ~0xff00) | G.MAX_SLOTS << 8

    def temp_before_write(image):   # operand a of the first instruction: slot 5
        image[instr0] = (image[instr0] & ~(0xffffff << 16)) | (3 << 21 | 5) << 16

    def immediate_outside(image):
        image[instr0] = (image[instr0] & ~(0xffffff << 16)) | (4 << 21 | 4000) << 16

    return {"magic": patch(0, 1), "no segments": patch(1, 0), "segment offset": patch(2, 10 ** 6),
            "instruction cap": patch(s + 1, G.MAX_INSTRUCTIONS + 1), "gate cap": patch(s + 0, G.MAX_GATES + 1),
            "alpha base": patch(s + 4, 1), "term count": patch(s + 5, 9), "selector depth": patch(s + 6, 9),
            "instruction range": patch(s + 8, 0 | 10 ** 4 << 32), "path over the cap": patch(s + 8 + 2, 2 | 9 << 32),
            "mask outside the path": patch(s + 8 + 3, 2), "zero repetitions": patch(s + 8 + 2, 0 | 1 << 32),
            "Inverse": inverse, "slot over the cap": slot_over_cap, "temporary read before written": temp_before_write,
            "immediate outside": immediate_outside}


@pytest.mark.parametrize("name", sorted(mutations()))
def test_validator_rejects(name):
    image = good_image()
    mutations()[name](image)
    with pytest.raises(BoojumError, match=r"\(-22\)"):
        G.check_image(image)


def test_validator_rejects_truncation_and_inverse_from_capture():
    image = good_image()
    for cut in (1, 2, 5, len(image) - 1):
        with pytest.raises(BoojumError, match=r"\(-22\)"):
            G.check_image(image[:cut])

    class Inverting(G.Evaluator):
        name, principal_width = "inverting", (1, 0, 0)

        def evaluate_once(self, src, dst, shared):
            dst.push_evaluation_result(src.get_variable_value(0).inverse())

    with pytest.raises(BoojumError, match="Inverse"):
        G.check_image(G.compile_gate_set([G.GatePlacement(G.capture(Inverting()))]))
