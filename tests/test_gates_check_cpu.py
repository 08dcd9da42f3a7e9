"""The gate satisfiability check without a GPU: the map from the running term index to (gate,
subinstance, term) (boojum_amd.gates.TermMap, GateSet.locate_term), the report and its message,
and the integer model (tests/gates_check_model.py) on the satisfiable circuit of gates_model and
on corrupted copies of it."""
import numpy as np
import pytest

import gates_check_model as C
import gates_model as M

from boojum_amd import gates as G

P = M.P
GEOMETRY = G.CSGeometry(30, 4, 8, 8)


class HostSet:
    """GateSet's host side without the upload: the image's term map and the placements."""
    locate_term = G.GateSet.locate_term
    gate_name = G.GateSet.gate_name

    def __init__(self, placements, from_image=False):
        self.term_map = G.TermMap(G.compile_gate_set(placements))
        self.placements = None if from_image else list(placements)


def mixed_placements():
    """The library's evaluators and PowerSum, alternately once and at their geometry counts, then a
    specialized placement."""
    out = []
    for i, e in enumerate(G.library() + [M.PowerSumEvaluator()]):
        reps = e.num_repetitions_in_geometry(GEOMETRY) if i % 2 else 1 + i % 3
        out.append(G.GatePlacement(G.capture(e), reps, None, [bool(i & 1), bool(i & 2)]))
    out.append(G.specialized_placement(G.ZeroCheckGate(False), 3, True, G.PerChunkOffset(2, 0, 1), 3))
    return out


def assert_locates(placements):
    hs = HostSet(placements)
    total = M.total_terms(placements)
    assert hs.term_map.num_terms == total
    assert [hs.locate_term(k) for k in range(total)] == [C.locate_brute(placements, k) for k in range(total)]
    for k in (-1, total):
        with pytest.raises(IndexError):
            hs.locate_term(k)
    return hs


# ------------------------------------------------------------------ locate_term
def test_locate_term_library_and_specialized():
    placements = mixed_placements()
    assert len({pl.num_repetitions for pl in placements}) > 3
    assert {e.name for e in G.library()} <= {pl.program.evaluator.name for pl in placements}
    hs = assert_locates(placements)
    assert hs.gate_name(0) == "fma_gate_in_base_without_constant" and hs.gate_name(len(placements) - 1) == \
        "zero_check_variable"


@pytest.mark.parametrize("kind", ["gates", "instructions"])
def test_locate_term_multi_segment(kind):
    """65 gates pass BJ_GATE_MAX_GATES; 16 chains of 300 relations pass BJ_GATE_MAX_INSTRUCTIONS."""
    if kind == "gates":
        bc = G.capture(G.BooleanConstraintGate())
        placements = [G.GatePlacement(bc, 1 + i % 3, None, [bool(i & 1)]) for i in range(65)]
    else:
        placements = [G.GatePlacement(M.chain_program(300), 1) for _ in range(16)]
        placements.insert(5, G.GatePlacement(G.capture(G.ZeroCheckGate(False)), 2))
    image = G.compile_gate_set(placements)
    assert image[1] == 2
    assert_locates(placements)


def test_locate_term_of_an_image_has_no_names():
    placements = mixed_placements()
    hs = HostSet(placements, from_image=True)
    assert hs.locate_term(3) == C.locate_brute(placements, 3) and hs.gate_name(0) is None
    assert HostSet([G.GatePlacement(M.chain_program(5), 1)]).gate_name(0) is None   # no evaluator behind the program


# ------------------------------------------------------------------ the report
def test_message_is_the_reference_sentence():
    r = G.SatisfiabilityReport(3, row=12, gate=1, gate_name="zero_check_witness", subinstance=4, term=1, k=9, value=P - 1)
    assert not r.satisfied and r.num_unsatisfied == 3
    assert r.message() == ("Unsatisfied at row 12 with value 0xffffffff00000000 for term number 1 for subinstance "
                           "number 4 of gate zero_check_witness")
    r = G.SatisfiabilityReport(1, row=0, gate=2, gate_name=None, subinstance=0, term=0, k=2, value=5)
    assert r.message() == ("Unsatisfied at row 0 with value 0x0000000000000005 for term number 0 for subinstance "
                           "number 0 of gate #2")
    ok = G.SatisfiabilityReport(0)
    assert ok.satisfied and ok.num_unsatisfied == 0 and ok.message() is None
    assert (ok.row, ok.gate, ok.gate_name, ok.subinstance, ok.term, ok.value) == (None,) * 6


def test_report_from_status():
    placements = mixed_placements()
    hs = HostSet(placements)
    k = M.total_terms(placements) - 2
    r = G.report_from_status(hs, [7, 41 << 32 | k, 99, 0])
    assert (r.num_unsatisfied, r.row, r.k, r.value) == (7, 41, k, 99)
    assert (r.gate, r.subinstance, r.term) == C.locate_brute(placements, k)
    assert r.gate_name == "zero_check_variable"
    assert G.report_from_status(hs, [0, C.NO_KEY, 0, 0]).satisfied
    with pytest.raises(ValueError):
        G.report_from_status(hs, [0, 5, 0, 0])


def test_product_does_not_reach_into_the_tests():
    text = open(G.__file__).read()
    assert "gates_model" not in text and "gates_check_model" not in text and "import oracle" not in text


# ------------------------------------------------------------------ the model on a circuit
@pytest.mark.parametrize("log_n", [3, 5])
def test_satisfiable_circuit_is_satisfied(log_n):
    c = M.satisfiable_circuit(log_n)
    assert C.check(c.placements, c.variables, c.witnesses, c.constants) == (0, None)
    assert C.status_record(c.placements, c.variables, c.witnesses, c.constants) == [0, C.NO_KEY, 0, 0]


def test_corrupted_cells_are_located():
    """The circuit's terms: k 0, 1 the two FMAs, 2, 3 the ZeroCheck, 4, 5 the allocators, 6, 7 the
    swap; row i runs gate i mod 4."""
    c = M.satisfiable_circuit(3)
    bad = c.variables.copy()
    bad[7, 4] = (int(bad[7, 4]) + 1) % P          # d of the second FMA of row 4: c1 c + c0 a b - d = -1
    assert C.check(c.placements, bad, c.witnesses, c.constants) == (1, (4, 1, P - 1))
    bad[1, 6] = (int(bad[1, 6]) + 3) % P          # the second allocator of row 6: a - constant = 3
    bad[0, 1] = (int(bad[0, 1]) + 1) % P          # input of row 1's ZeroCheck: both of its terms move
    count, first = C.check(c.placements, bad, c.witnesses, c.constants)
    assert first[:2] == (1, 2) and 3 <= count <= 4
    assert C.check(c.placements, bad, c.witnesses, c.constants, rows=(2, 6)) == (2, (4, 1, P - 1))
    assert C.check(c.placements, bad, c.witnesses, c.constants, rows=(5, 3)) == (1, (6, 5, 3))
    assert C.check(c.placements, bad, c.witnesses, c.constants, rows=(7, 1)) == (0, None)
    rec = C.status_record(c.placements, bad, c.witnesses, c.constants, rows=(4, 4))
    assert rec == [2, 4 << 32 | 1, P - 1, 0]
    hs = HostSet(c.placements)
    r = G.report_from_status(hs, rec)
    assert (r.row, r.gate, r.gate_name, r.subinstance, r.term, r.value) == \
        (4, 0, "fma_gate_in_base_without_constant", 1, 0, P - 1)


def test_selector_rules_of_the_model():
    """A zero selector hides a non-zero term, a selector of 5 does not, the word p is zero and
    other representatives of a cell change nothing."""
    bc = G.GatePlacement(G.capture(G.BooleanConstraintGate()), 1, None, [True])
    v, k = np.array([[2, 2, 2, 1]], dtype=np.uint64), np.array([[0, 5, 1, 1]], dtype=np.uint64)
    assert C.check([bc], v, [], k) == (2, (1, 0, P - 2))
    k[0, 0], v[0, 3] = P, P + 1
    assert C.check([bc], v, [], k) == (2, (1, 0, P - 2))
    push = G.GatePlacement(G.GateProgram([], [G.Index.VariablePoly(0)], 1), 1)   # the term is the cell itself
    assert C.check([push], np.array([[P, 0, 7]], dtype=np.uint64), [], []) == (1, (2, 0, 7))
