"""The Poseidon2 flattened gate on the host (no GPU): the evaluator of boojum_amd/gates.py against
the permutation the oracle pins to the reference, its capture, the native segment compile_gate_set
emits for it and the library's validator (bj_gate_set_check_h, bj_gate_native_info_h)."""
import ctypes
import random

import numpy as np
import pytest

import gates_model as M
import oracle
import poseidon2_gate_model as PM
import test_poseidon2_sched as R

from boojum_amd import _lib
from boojum_amd import gates as G

P = M.P
SPLITS = [0, 5, 106]


def rnd(seed, count):
    rng = random.Random(seed)
    return [rng.randrange(P) for _ in range(count)]


def gate(nw):
    return G.Poseidon2FlattenedGate(PM.CELLS - nw, nw)


# ------------------------------------------------------------------ the evaluator
def test_inner_matrix_is_ones_plus_shifted_diagonal():
    """InternalMatrixParams::COEFFS (params.rs:96-105) is ones with diag 2^SH + 1, ExternalMatrixParams
    (:63-94) circ(2 M4, M4, M4): the matrices the evaluator applies naively are the structured ones."""
    x = rnd(1, 12)
    naive = lambda m: [sum(c * v for c, v in zip(row, x)) % P for row in m]   # noqa: E731
    assert naive(G.poseidon2_inner_matrix()) == R._mi(x)
    assert naive(G.poseidon2_external_matrix()) == R._mds(x)
    assert list(G.POSEIDON2_SHIFTS) == R.SH and [list(r) for r in G.POSEIDON2_M4] == R.M4
    assert G.poseidon2_round_constants() == R.RC


@pytest.mark.parametrize("nw", SPLITS)
def test_satisfying_rows_have_zero_terms_and_the_permutation_as_output(nw):
    e = gate(nw)
    for inputs in ([0] * 12, list(range(12)), [P - 1] * 12, rnd(nw, 12)):
        v, w = PM.satisfying_row(inputs, nw)
        assert len(v) == PM.CELLS - nw and len(w) == nw
        assert PM.evaluator_terms(e, v, w) == [0] * PM.TERMS
        assert v[12:24] == R.reference_permutation(inputs)
        assert v[12:24] == [int(x) for x in oracle.poseidon2_permutation(np.array(inputs, dtype=np.uint64))]


@pytest.mark.parametrize("nw", SPLITS)
def test_evaluator_capture_and_model_agree_on_random_rows(nw):
    e = gate(nw)
    for seed in (1, 2):
        v, w = rnd(10 * nw + seed, PM.CELLS - nw), rnd(20 * nw + seed, nw)
        direct = PM.evaluator_terms(e, v, w)
        assert len(direct) == PM.TERMS and all(direct)
        assert PM.captured_terms(e, v, w) == direct
        assert PM.terms(v, w, nw) == direct


def test_capture_passes_both_caps():
    program = PM.captured(130, 0)
    assert len(program.relations) > 2 * G.MAX_INSTRUCTIONS
    with pytest.raises(ValueError, match="temporaries are live"):
        G.allocate_slots(program)


@pytest.mark.parametrize("nw", SPLITS)
def test_push_order(nw):
    """Corrupting S-box output cell s changes its own reset term and every term up to the next reset
    of the whole state; corrupting an input changes the first 12, an output cell only its own term."""
    e = gate(nw)
    v, w = PM.satisfying_row(rnd(3, 12), nw)

    def changed(s=None, var=None):
        bv, bw = list(v), list(w)
        if var is not None:
            bv[var] = (bv[var] + 1) % P
        elif s < nw:
            bw[s] = (bw[s] + 1) % P
        else:
            bv[24 + s - nw] = (bv[24 + s - nw] + 1) % P
        return [k for k, t in enumerate(PM.evaluator_terms(e, bv, bw)) if t]

    assert changed(var=0) == list(range(12))
    assert changed(var=12 + 5) == [106 + 5]
    assert changed(s=0) == [0] + list(range(12, 24))              # first reset -> the second
    # the third reset and the partial cells feed the state that is not reset before the second half
    assert changed(s=24 + 3) == [27] + list(range(36, 70))
    assert changed(s=36) == list(range(36, 70))
    assert changed(s=36 + 21) == [57] + list(range(58, 70))        # the last partial cell -> the whole state
    assert changed(s=58 + 36 + 11) == [105] + list(range(106, 118))   # the last reset -> the outputs


def test_geometry_properties_match_the_reference():
    """compute_strategy and num_repetitions_in_geometry on the two geometries of test_properties
    (poseidon2.rs:968-1005)."""
    for geometry, want in ((G.CSGeometry(80, 80, 10, 8), (1, (50, 80))), (G.CSGeometry(140, 0, 8, 8), (1, (130, 0)))):
        got = G.Poseidon2FlattenedGate.compute_strategy(geometry)
        assert got == want
        e = G.Poseidon2FlattenedGate(*got[1])
        assert e.num_repetitions_in_geometry(geometry) == 1
        assert e.principal_width == (got[1][0], got[1][1], 0)
        assert e.per_chunk_offset.as_tuple() == (got[1][0], got[1][1], 0)
        assert e.num_required_constants_in_geometry(geometry) == 0
    wide = G.CSGeometry(260, 10, 8, 8)
    assert G.Poseidon2FlattenedGate.compute_strategy(wide) == (2, (125, 5))
    assert G.Poseidon2FlattenedGate(125, 5).num_repetitions_in_geometry(wide) == 2
    assert G.Poseidon2FlattenedGate(130, 0).num_repetitions_in_geometry(wide) == 2
    with pytest.raises(ValueError):
        G.Poseidon2FlattenedGate.compute_strategy(G.CSGeometry(23, 200, 8, 8))
    with pytest.raises(ValueError):
        G.Poseidon2FlattenedGate(100, 5)


# ------------------------------------------------------------------ the image
def mixed_placements():
    return [G.GatePlacement(G.capture(G.FmaGateInBaseFieldWithoutConstant()), 2, None, [True]),
            G.GatePlacement(G.capture(G.BooleanConstraintGate()), 3, None, [False, True]),
            PM.placement(5, 2, [False, False, True]),
            G.GatePlacement(G.capture(G.ReductionGate(4)), 1, None, [False, False, False])]


def test_native_info():
    assert G.native_gate_info(G.KIND_POSEIDON2) == (130, 118, 7, 106)
    assert G.native_gate_info(2) is None
    out = (ctypes.c_uint64 * 4)()
    with pytest.raises(_lib.BoojumError, match=r"\(-22\)"):
        _lib.call("bj_gate_native_info_h", 0, out)


def test_compile_emits_a_native_segment_between_interpreted_ones():
    placements = mixed_placements()
    image = G.compile_gate_set(placements)
    assert image[0] == G.MAGIC and image[1] == 3
    heads = [image[image[2 + s]:image[2 + s] + 8] for s in range(3)]
    assert [h[7] for h in heads] == [0, G.KIND_POSEIDON2, 0]
    assert [h[0] for h in heads] == [2, 1, 1]
    assert [h[4] for h in heads] == [0, 5, 5 + 236] and [h[5] for h in heads] == [5, 236, 1]
    assert heads[1][1:4] == [0, 0, 0] and heads[1][6] == 3
    d = image[image[3] + 8:image[3] + 16]
    assert d == [0, 118 << 32, 2 | 3 << 32, 0b100, 0 | 125 << 32, 0 | 5 << 32, 3 | 0 << 32, 5]
    assert image[3] + 16 == image[4]   # nothing behind the descriptor
    tm = G.TermMap(image)
    assert tm.num_terms == 242
    assert [tm.locate(k) for k in (0, 1, 2, 4, 5, 122, 123, 240, 241)] == \
        [(0, 0, 0), (0, 1, 0), (1, 0, 0), (1, 2, 0), (2, 0, 0), (2, 0, 117), (2, 1, 0), (2, 1, 117), (3, 0, 0)]
    need = G.check_image(image)
    assert need == dict(variables=250, witnesses=10, constants=7, alphas=242, segments=3)


def test_need_of_a_native_segment():
    for pl, want in ((PM.placement(0), (130, 0, 0)), (PM.placement(106, 1, [True]), (24, 106, 1)),
                     (PM.placement(5, 3, [True] * 8, G.PerChunkOffset(7, 2, 0), ncu=128), (7 + 2 * 128 + 125, 17, 8))):
        need = G.check_image(G.compile_gate_set([pl]))
        assert (need["variables"], need["witnesses"], need["constants"]) == want
        assert need["alphas"] == 118 * pl.num_repetitions and need["segments"] == 1


def test_layout_does_not_capture_a_native_gate():
    e = G.Poseidon2FlattenedGate(125, 5)
    pls = G.layout_general_purpose([(G.BooleanConstraintGate(), [True]), (e, [False])], G.CSGeometry(260, 10, 8, 8))
    assert isinstance(pls[1].program, G.NativeGateProgram) and pls[1].num_repetitions == 2
    assert pls[1].num_terms() == 236
    captured = G.GatePlacement(PM.captured(125, 5), 2, None, [False])   # a capture of it is not used either
    assert G.compile_gate_set([pls[0], captured]) == G.compile_gate_set(pls)


def test_library_image_is_unchanged_word_for_word():
    """An image without native segments is what the compiler before native segments gave: one
    segment, word [7] of the head and of every descriptor zero, and the words in between rebuilt
    here from the captures by the documented layout."""
    placements = G.layout_general_purpose([(e, [bool(i & 1), bool(i & 2)]) for i, e in enumerate(G.library())],
                                          G.CSGeometry(16, 2, 4, 8))
    image = G.compile_gate_set(placements)
    seg = G._Segment(0)
    for pl in placements:
        assert G._encode_gate(seg, pl, G.MAX_SLOTS)
    head = [len(placements), len(seg.instr), len(seg.writes), len(seg.imm), 0, seg.terms, 2, 0]
    assert image == [G.MAGIC, 1, 3] + head + seg.desc + seg.instr + seg.writes + seg.imm
    assert all(seg.desc[8 * g + 7] == 0 for g in range(len(placements)))
    assert G.check_image(image)["segments"] == 1


def native_image():
    image = G.compile_gate_set([PM.placement(5, 2, [True, False])])
    return image, image[2], image[2] + 8


@pytest.mark.parametrize("case", ["kind", "gates", "instructions", "writes", "immediates", "terms", "nw", "variables",
                                  "witnesses", "path", "range"])
def test_malformed_native_segments_are_refused(case):
    image, seg, d = native_image()
    assert G.check_image(image)["alphas"] == 236
    if case == "kind":
        image[seg + 7] = 2
    elif case == "gates":
        image[seg] = 2
        image += image[d:d + 8]
    elif case in ("instructions", "writes", "immediates"):
        image[seg + {"instructions": 1, "writes": 2, "immediates": 3}[case]] = 1
        image.append(0)
    elif case == "terms":
        image[seg + 5] = 118
    elif case == "nw":
        image[d + 7] = 107
    elif case == "variables":
        image[d + 4] = 0 | 124 << 32
    elif case == "witnesses":
        image[d + 5] = 0 | 4 << 32
    elif case == "path":
        image[d + 2] = 2 | 9 << 32
        image[seg + 6] = 9
    elif case == "range":
        image[d + 1] = 0 | 117 << 32
    with pytest.raises(_lib.BoojumError, match=r"\(-22\)"):
        G.check_image(image)


def test_a_library_without_the_symbol_refuses_the_gate(monkeypatch):
    monkeypatch.setattr(G, "native_gate_info", lambda kind: None)
    with pytest.raises(ValueError, match="exceeds the caps of a launch"):
        G.compile_gate_set([PM.placement(0)])
