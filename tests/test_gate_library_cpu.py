"""Library segments on the host (no GPU): the generated header against its generator, the library's
table (bj_gate_library_find_h) against the Python captures, the images compile_gate_set emits with and
without native_library, and the validator's rules for kind 3 (bj_gate_set_check_h)."""
import ctypes
import os
import subprocess
import sys

import pytest

import gate_library_cases as L
import gates_model as M

from boojum_amd import _lib
from boojum_amd import gates as G

ROOT = L.ROOT
NAMES = ["fma_gate_in_base_without_constant", "boolean_constraint", "constants_allocator", "reduction_gate_4",
         "selection_gate", "zero_check_variable", "zero_check_witness", "dot_product_gate_4",
         "conditional_swap_gate_1"]


# ------------------------------------------------------------------ the header
def test_header_is_generated(tmp_path):
    out = tmp_path / "gates_library.hpp"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_gate_library.py"), "--out", str(out)], check=True,
                   capture_output=True)
    committed = open(os.path.join(ROOT, "era-boojum_amd", "csrc", "gates_library.hpp")).read()
    assert out.read_text() == committed, "csrc/gates_library.hpp differs from tools/gen_gate_library.py's output"


# ------------------------------------------------------------------ the table
def columns_read(program):
    width = {"VariablePoly": 0, "WitnessPoly": 0, "ConstantPoly": 0}
    for o in [o for _, rel in program.relations for o in rel.operands] + list(program.writes):
        if o.kind in width:
            width[o.kind] = max(width[o.kind], o.value + 1)
    return tuple(width.values())


def test_table_lookup():
    evaluators = G.library()
    assert [e.name for e in evaluators] == NAMES
    for i, e in enumerate(evaluators):
        program = G.capture(e)
        assert G.library_gate_info(e.name) == (i + 1, e.num_quotient_terms) + columns_read(program) + \
            (G.program_digest(program),)
    assert len({G.library_gate_info(n)[5] for n in NAMES}) == 9
    assert G.library_gate_info("reduction_gate_5") is None and G.library_gate_info("") is None
    assert G.library_gate_info(None) is None
    out = (ctypes.c_uint64 * 6)()
    for name in (b"no_such_gate", None):
        assert _lib.load().bj_gate_library_find_h(name, out) == -22
        with pytest.raises(_lib.BoojumError, match=r"\(-22\)"):
            _lib.call("bj_gate_library_find_h", name, out)
    assert G.native_gate_info(G.KIND_LIBRARY) is None and G.KIND_LIBRARY == 3
    assert G.native_gate_info(2) is None


def test_digest_is_of_the_relations_and_the_writes():
    idx, rel = G.Index, G.Relation
    base = G.GateProgram([(0, rel.Add(idx.VariablePoly(0), idx.ConstantValue(1)))], [idx.TemporaryValue(0)], 1)
    assert G.program_digest(base) == G.program_digest(G.GateProgram(list(base.relations), list(base.writes), 1))
    others = [G.GateProgram([(0, rel.Sub(idx.VariablePoly(0), idx.ConstantValue(1)))], [idx.TemporaryValue(0)], 1),
              G.GateProgram([(0, rel.Add(idx.WitnessPoly(0), idx.ConstantValue(1)))], [idx.TemporaryValue(0)], 1),
              G.GateProgram([(0, rel.Add(idx.VariablePoly(0), idx.ConstantValue(2)))], [idx.TemporaryValue(0)], 1),
              G.GateProgram([(0, rel.Add(idx.VariablePoly(0), idx.ConstantValue(1)))], [idx.VariablePoly(0)], 1),
              G.GateProgram([(0, rel.Add(idx.VariablePoly(0), idx.ConstantValue(1)))], [idx.TemporaryValue(0)] * 2, 2)]
    assert len({G.program_digest(p) for p in others + [base]}) == 6
    # FNV-1a-64 of the documented bytes, said again here
    data = (1).to_bytes(4, "little") + (1).to_bytes(4, "little") + bytes([0]) + (0).to_bytes(4, "little") + \
        bytes([2, 0]) + (0).to_bytes(8, "little") + bytes([4]) + (1).to_bytes(8, "little") + b"\xff" + bytes([3]) + \
        (0).to_bytes(8, "little")
    h = 0xCBF29CE484222325
    for byte in data:
        h = (h ^ byte) * 0x100000001B3 % (1 << 64)
    assert G.program_digest(base) == h


# ------------------------------------------------------------------ the images
def test_flag_off_changes_nothing():
    for placements in (L.bench_set(), L.mixed_set()):
        assert G.compile_gate_set(placements) == G.compile_gate_set(placements, native_library=False)
        assert G.compile_gate_set(placements) == G.compile_gate_set(placements, G.MAX_SLOTS, False)
        assert 3 not in L.kinds_of(G.compile_gate_set(placements))


def descriptors(image, s):
    seg = image[2 + s]
    return [image[seg + 8 + 8 * g:seg + 16 + 8 * g] for g in range(image[seg])]


def test_mixed_set_with_the_flag():
    placements = L.mixed_set()
    plain = G.compile_gate_set(placements)
    image = G.compile_gate_set(placements, native_library=True)
    assert L.kinds_of(plain) == [0, 1, 0] and L.kinds_of(image) == [3, 1, 0, 3]
    heads = [image[image[2 + s]:image[2 + s] + 8] for s in range(4)]
    assert [h[0] for h in heads] == [2, 1, 1, 2]
    assert [h[1:4] for h in heads] == [[0, 0, 0], [0, 0, 0], [2, 1, 0], [0, 0, 0]]
    assert [h[5] for h in heads] == [2 + 6, 118, 2, 1 + 4]
    assert [h[4] for h in heads] == [0, 8, 126, 128] and all(h[6] == 3 for h in heads)
    ids = {n: i + 1 for i, n in enumerate(NAMES)}
    want = [(0, 0, "fma_gate_in_base_without_constant", 1, placements[0]), (0, 1, "zero_check_witness", 2, placements[1]),
            (3, 0, "reduction_gate_4", 1, placements[4]), (3, 1, "conditional_swap_gate_1", 2, placements[5])]
    for s, g, name, terms, pl in want:
        d = descriptors(image, s)[g]
        assert d[0] == ids[name] and d[1] == terms << 32 and d[7] == 0
        assert d[2:7] == G._placement_words(pl)
    seg = image[2]
    assert image[3] == seg + 8 + 2 * 8   # nothing behind the descriptors of a library segment
    assert descriptors(image, 2) == descriptors(plain, 2)[:1]   # the interpreted gate keeps its encoding
    assert G.check_image(image) == dict(G.check_image(plain), segments=4)   # only the split differs: 4 for 3
    assert G.check_image(image) == dict(variables=125, witnesses=5, constants=7, alphas=133, segments=4)
    assert G.TermMap(image).gates == G.TermMap(plain).gates
    assert G.TermMap(image).num_terms == M.total_terms(placements)


def test_bench_set_with_the_flag():
    placements = L.bench_set()
    plain, image = G.compile_gate_set(placements), G.compile_gate_set(placements, native_library=True)
    assert L.kinds_of(image) == [3] and image[image[2]] == 8 and len(image) == 3 + 8 + 8 * 8
    need, want = G.check_image(image), G.check_image(plain)
    assert need == dict(want, segments=1) and want["variables"] == 130 and want["constants"] == 11
    assert G.TermMap(image).gates == G.TermMap(plain).gates


def test_more_than_64_library_gates_take_two_segments():
    bc = G.capture(G.BooleanConstraintGate())
    placements = [G.GatePlacement(bc, 1, None, (), 0, G.PerChunkOffset(g, 0, 0)) for g in range(66)]
    image = G.compile_gate_set(placements, native_library=True)
    assert L.kinds_of(image) == [3, 3] and [image[image[2 + s]] for s in range(2)] == [64, 2]
    assert image[image[3] + 4] == 64
    assert G.check_image(image) == G.check_image(G.compile_gate_set(placements))


def test_an_altered_evaluator_of_a_library_name_stays_interpreted():
    e = L.AlteredSelectionGate()
    assert e.name == "selection_gate" and G.program_digest(G.capture(e)) != G.library_gate_info(e.name)[5]
    placements = [G.GatePlacement(G.capture(G.SelectionGate()), 1), G.GatePlacement(G.capture(e), 1, None, (), 0,
                                                                                     G.PerChunkOffset(4, 0, 0))]
    image = G.compile_gate_set(placements, native_library=True)
    assert L.kinds_of(image) == [3, 0]
    alone = G.compile_gate_set(placements[1:])
    got, want = image[image[3]:], alone[alone[2]:]
    assert got[:4] == want[:4] and got[4] == 1 and got[5:] == want[5:]   # its own encoding, the alpha base carried on
    bare = G.GateProgram(G.capture(G.SelectionGate()).relations, G.capture(G.SelectionGate()).writes, 1)
    assert L.kinds_of(G.compile_gate_set([G.GatePlacement(bare, 1)], native_library=True)) == [0]   # no evaluator, no name


def test_a_library_without_the_symbol_keeps_every_gate_interpreted(monkeypatch):
    monkeypatch.setattr(G, "library_gate_info", lambda name: None)
    placements = L.mixed_set()
    assert G.compile_gate_set(placements, native_library=True) == G.compile_gate_set(placements)


# ------------------------------------------------------------------ the validator
def library_image():
    """FMA x 2 under [1, 0] and ZeroCheck(variable) x 3 under [0]: one segment of kind 3, 2 + 6 terms."""
    placements = [G.GatePlacement(G.capture(G.FmaGateInBaseFieldWithoutConstant()), 2, None, [True, False]),
                  G.GatePlacement(G.capture(G.ZeroCheckGate(False)), 3, None, [False])]
    image = G.compile_gate_set(placements, native_library=True)
    assert L.kinds_of(image) == [3]
    return image, image[2], image[2] + 8, image[2] + 16


def refused(image, message):
    with pytest.raises(_lib.BoojumError, match=r"\(-22\)") as info:
        G.check_image(image)
    assert message in str(info.value), str(info.value)


def test_the_image_under_test_is_accepted():
    image, seg, d0, d1 = library_image()
    assert G.check_image(image) == dict(variables=9, witnesses=0, constants=4, alphas=8, segments=1)
    assert image[seg:seg + 8] == [2, 0, 0, 0, 0, 8, 2, 3]


RULES = {
    "gates": "gates of a segment outside 1..BJ_GATE_MAX_GATES",
    "instructions": "a library segment carries no instructions, writes or immediates",
    "writes": "a library segment carries no instructions, writes or immediates",
    "immediates": "a library segment carries no instructions, writes or immediates",
    "id_zero": "unknown library gate id",
    "id_past_the_table": "unknown library gate id",
    "id_high_half": "unknown library gate id",
    "terms_of_the_gate": "a library gate's term count is not its entry's",
    "terms_low_half": "a library gate's term count is not its entry's",
    "word7": "word [7] of a library gate is not 0",
    "terms_of_the_segment": "a segment's term count is not the sum over its gates",
    "selector_depth": "a segment's selector columns are not its deepest path",
    "repetitions": "num_repetitions outside 1..2^20",
    "path": "malformed selector path",
    "mask": "malformed selector path",
    "offset": "a column offset is out of range",
    "alpha_base": "a segment's alpha base is not the sum of the terms before it",
    "kind_2": "unknown native segment kind",
}


@pytest.mark.parametrize("case", sorted(RULES))
def test_malformed_library_segments_are_refused(case):
    image, seg, d0, d1 = library_image()
    if case == "gates":
        image[seg] = 0
    elif case in ("instructions", "writes", "immediates"):
        image[seg + {"instructions": 1, "writes": 2, "immediates": 3}[case]] = 1
        image.append(0)
    elif case == "id_zero":
        image[d1] = 0
    elif case == "id_past_the_table":
        image[d0] = 10
    elif case == "id_high_half":
        image[d0] |= 1 << 32
    elif case == "terms_of_the_gate":
        image[d1 + 1] = 1 << 32   # ZeroCheck has two
    elif case == "terms_low_half":
        image[d0 + 1] |= 1
    elif case == "word7":
        image[d1 + 7] = 1
    elif case == "terms_of_the_segment":
        image[seg + 5] = 7
    elif case == "selector_depth":
        image[seg + 6] = 1
    elif case == "repetitions":
        image[d1 + 2] = 0 | 1 << 32
    elif case == "path":
        image[d0 + 2] = 2 | 9 << 32
    elif case == "mask":
        image[d1 + 3] = 0b10
    elif case == "offset":
        image[d0 + 6] = 2 | (1 << 10) + 1 << 32
    elif case == "alpha_base":
        image[seg + 4] = 1
    elif case == "kind_2":
        image[seg + 7] = 2
    refused(image, RULES[case])


def test_every_refusal_of_the_kind_has_its_image():
    """The kind's own messages are the named strings of namespace refusal in gates.hip (the golden of
    test_gate_check_errors.py holds the literal bad("...") texts from before library segments)."""
    import re
    src = open(os.path.join(ROOT, "era-boojum_amd", "csrc", "gates.hip")).read()
    block = src[src.index("namespace refusal {"):src.index("}  // namespace refusal")]
    texts = set(re.findall(r'constexpr const char\* \w+ = "([^"]+)";', block))
    assert len(texts) == 4 and texts <= set(RULES.values())
    assert len(re.findall(r"\bbad\(refusal::\w+\)", src)) == 4


def test_the_placement_is_checked_before_the_kind_s_own_rules():
    image, seg, d0, d1 = library_image()
    image[d0] = 10           # an unknown id on the first gate ...
    image[d1 + 2] = 0        # ... and no repetitions on the second: the placement is met first
    refused(image, "num_repetitions outside 1..2^20")
    image, seg, d0, d1 = library_image()
    image[d0 + 7] = 1
    image[d1 + 4] = (1 << 20) + 1
    refused(image, "a column offset is out of range")


def test_the_program_area_is_checked_before_the_ids_and_an_id_before_its_words():
    image, seg, d0, d1 = library_image()
    image[d0] = 10
    image[seg + 2] = 1
    image.append(0)
    refused(image, "a library segment carries no instructions, writes or immediates")
    image, seg, d0, d1 = library_image()
    image[d0] = 10
    image[d0 + 1] = 5 << 32
    image[d0 + 7] = 1
    refused(image, "unknown library gate id")
    image, seg, d0, d1 = library_image()
    image[d0 + 1] = 5 << 32
    image[d0 + 7] = 1
    refused(image, "a library gate's term count is not its entry's")


def test_need_follows_the_largest_repetition():
    """base + (repetitions - 1) * per + the columns one repetition reads, per kind, as the interpreted
    image of the same placement reports it; shared constants do not advance."""
    cases = [G.GatePlacement(G.capture(G.ZeroCheckGate(True)), 3, None, [True], None, G.PerChunkOffset(5, 2, 0)),
             G.specialized_placement(G.FmaGateInBaseFieldWithoutConstant(), 3, True, G.PerChunkOffset(7, 0, 1), 4),
             G.specialized_placement(G.FmaGateInBaseFieldWithoutConstant(), 3, False, G.PerChunkOffset(7, 0, 1), 4),
             G.GatePlacement(G.capture(G.ConstantsAllocatorGate()), 4, None, [True, False, True])]
    wants = [(5 + 2 * 2 + 2, 2 + 2 + 1, 1), (7 + 2 * 4 + 4, 0, 4 + 1 + 2), (7 + 2 * 4 + 4, 0, 4 + 1 + 2 * 2 + 2),
             (4, 0, 3 + 3 + 1)]
    for pl, want in zip(cases, wants):
        image = G.compile_gate_set([pl], native_library=True)
        assert L.kinds_of(image) == [3]
        need = G.check_image(image)
        assert need == G.check_image(G.compile_gate_set([pl]))
        assert (need["variables"], need["witnesses"], need["constants"]) == want
