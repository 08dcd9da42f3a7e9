"""The rejected images of the gate-set validator bj_gate_set_check_h whose return code and bj_last_error() text
tests/golden/gate_check_errors.json pins: every distinct rejection, and pairs of faults in one image, where the
message that wins pins the order of the checks.  tests/test_gate_check_errors.py checks them; the golden was
recorded from the library as it was before the two kinds of segment came to share their placement checks:

    python3 tools/record_host_errors.py --lib <the earlier library> --cases gate_check_cases \\
        --out tests/golden/gate_check_errors.json

The case format is that of tests/host_error_cases.py: a name and a function of the loaded library that returns
the call's code.  The call is host-only, so no case needs a device.
"""
import ctypes

from host_error_cases import run   # noqa: F401  (the recorder and the test run the cases through it)

# ------------------------------------------------------------------ bj_gate_set_check_h
# Two images and patches of single words.  Interpreted: one segment at S, the FMA gate twice under [True]
# (descriptor D, instructions 0..5, write 0) and the ZeroCheck gate with a witness under [False, True]
# (descriptor D + 8, instructions 5..9, writes 1..3), 9 instructions from I, 3 writes from W, 1 immediate.
# Native: one segment at S, the Poseidon2 gate twice (125 variables, 5 witnesses) under [True, False].
S, D, I, W, END = 3, 11, 27, 36, 40
NATIVE_END = 19
_images = {}


def _image(native):
    if native not in _images:
        from boojum_amd import gates as G
        if native:
            pls = [G.GatePlacement(G.program_of(G.Poseidon2FlattenedGate(125, 5)), 2, None, [True, False])]
        else:
            pls = [G.GatePlacement(G.capture(G.FmaGateInBaseFieldWithoutConstant()), 2, None, [True]),
                   G.GatePlacement(G.capture(G.ZeroCheckGate(True)), 1, None, [False, True])]
        _images[native] = G.compile_gate_set(pls)
        assert len(_images[native]) == (NATIVE_END if native else END)
    return list(_images[native])


def _gates(L, patch=None, native=False, words=None, extra=0):
    """The validator on an image with patch {word index: new value, or a function of the old one} applied,
    `extra` zero words appended and `words` (default: all) passed as its length."""
    image = _image(native) + [0] * extra
    for at, value in (patch or {}).items():
        image[at] = value(image[at]) if callable(value) else value
    return L.bj_gate_set_check_h((ctypes.c_uint64 * len(image))(*image), len(image) if words is None else words, None)


def _native(L, patch=None, **kw):
    return _gates(L, patch, native=True, **kw)


def _op(code):
    return lambda w: (w & ~0xff) | code


def _a(kind, idx):   # operand a of an instruction
    return lambda w: (w & ~(0xffffff << 16)) | (kind << 21 | idx) << 16


def _b(kind, idx):
    return lambda w: (w & ~(0xffffff << 40)) | (kind << 21 | idx) << 40


HOST = [
    ("gate_check/null_image", lambda L: L.bj_gate_set_check_h(None, 0, None)),
    ("gate_check/one_word", lambda L: _gates(L, words=1)),
    ("gate_check/magic", lambda L: _gates(L, {0: 1})),
    ("gate_check/segments_0", lambda L: _gates(L, {1: 0})),
    ("gate_check/segments_65", lambda L: _gates(L, {1: 65})),
    ("gate_check/segment_table_cut", lambda L: _gates(L, {1: 64})),
    ("gate_check/offset_inside_table", lambda L: _gates(L, {2: 2})),
    ("gate_check/offset_past_end", lambda L: _gates(L, {2: END + 1})),
    ("gate_check/offset_head_cut", lambda L: _gates(L, {2: END - 7})),
    ("gate_check/gates_0", lambda L: _gates(L, {S: 0})),
    ("gate_check/gates_65", lambda L: _gates(L, {S: 65})),
    ("gate_check/instructions_4097", lambda L: _gates(L, {S + 1: 4097})),
    ("gate_check/writes_4097", lambda L: _gates(L, {S + 2: 4097})),
    ("gate_check/immediates_4097", lambda L: _gates(L, {S + 3: 4097})),
    ("gate_check/segment_cut", lambda L: _gates(L, words=END - 1)),
    ("gate_check/head_selector_9", lambda L: _gates(L, {S + 6: 9})),
    ("gate_check/alpha_base_1", lambda L: _gates(L, {S + 4: 1})),
    ("gate_check/pair_magic_segments_0", lambda L: _gates(L, {0: 1, 1: 0})),
    ("gate_check/pair_segments_65_table_cut", lambda L: _gates(L, {1: 65}, words=3)),
    ("gate_check/pair_gates_0_instructions", lambda L: _gates(L, {S: 0, S + 1: 4097})),
    ("gate_check/pair_instructions_writes", lambda L: _gates(L, {S + 1: 4097, S + 2: 4097})),
    ("gate_check/pair_writes_segment_cut", lambda L: _gates(L, {S + 2: 4097}, words=END - 1)),
    ("gate_check/pair_segment_cut_head_selector", lambda L: _gates(L, {S + 6: 9}, words=END - 1)),
    ("gate_check/pair_head_selector_alpha_base", lambda L: _gates(L, {S + 6: 9, S + 4: 1})),
    ("gate_check/pair_alpha_base_unknown_kind", lambda L: _gates(L, {S + 4: 1, S + 7: 2})),
    # an interpreted gate, in the order of its checks
    ("gate_check/instr_begin_gt_end", lambda L: _gates(L, {D: 6 | 5 << 32})),
    ("gate_check/instr_end_gt_count", lambda L: _gates(L, {D + 8: 5 | 10 << 32})),
    ("gate_check/no_writes", lambda L: _gates(L, {D + 1: 1 | 1 << 32})),
    ("gate_check/write_end_gt_count", lambda L: _gates(L, {D + 9: 1 | 4 << 32})),
    ("gate_check/reps_0", lambda L: _gates(L, {D + 2: 0 | 1 << 32})),
    ("gate_check/reps_over_2_20", lambda L: _gates(L, {D + 2: (1 << 20) + 1 | 1 << 32})),
    ("gate_check/path_9", lambda L: _gates(L, {D + 2: 2 | 9 << 32})),
    ("gate_check/mask_outside_path", lambda L: _gates(L, {D + 3: 2})),
    ("gate_check/descriptor_word_7", lambda L: _gates(L, {D + 7: 1})),
    ("gate_check/variables_base_over_2_20", lambda L: _gates(L, {D + 4: (1 << 20) + 1 | 4 << 32})),
    ("gate_check/witnesses_per_over_2_10", lambda L: _gates(L, {D + 5: 0 | 1025 << 32})),
    ("gate_check/constants_base_over_2_20", lambda L: _gates(L, {D + 6: (1 << 20) + 1})),
    ("gate_check/inverse", lambda L: _gates(L, {I: _op(6)})),
    ("gate_check/opcode_7", lambda L: _gates(L, {I: _op(7)})),
    ("gate_check/slot_16", lambda L: _gates(L, {I: lambda w: (w & ~0xff00) | 16 << 8})),
    ("gate_check/slot_read_before_written", lambda L: _gates(L, {I: _a(3, 5)})),
    ("gate_check/slot_operand_16", lambda L: _gates(L, {I + 1: _a(3, 16)})),
    ("gate_check/immediate_outside", lambda L: _gates(L, {I: _a(4, 1)})),
    ("gate_check/operand_kind_5", lambda L: _gates(L, {I: _a(5, 0)})),
    ("gate_check/operand_b_immediate_outside", lambda L: _gates(L, {I: _b(4, 1)})),
    ("gate_check/unary_with_operand_b", lambda L: _gates(L, {I: _op(1)})),
    ("gate_check/write_high_bits", lambda L: _gates(L, {W: lambda w: w | 1 << 24})),
    ("gate_check/write_slot_never_written", lambda L: _gates(L, {W: 3 << 21 | 9})),
    ("gate_check/term_count_5", lambda L: _gates(L, {S + 5: 5})),
    ("gate_check/head_selector_1_of_2", lambda L: _gates(L, {S + 6: 1})),
    ("gate_check/pair_range_reps_0", lambda L: _gates(L, {D: 6 | 5 << 32, D + 2: 0 | 1 << 32})),
    ("gate_check/pair_reps_0_path_9", lambda L: _gates(L, {D + 2: 0 | 9 << 32})),
    ("gate_check/pair_mask_variables_base", lambda L: _gates(L, {D + 3: 2, D + 4: (1 << 20) + 1 | 4 << 32})),
    ("gate_check/pair_word_7_constants_base", lambda L: _gates(L, {D + 7: 1, D + 6: (1 << 20) + 1})),
    ("gate_check/pair_constants_base_inverse", lambda L: _gates(L, {D + 6: (1 << 20) + 1, I: _op(6)})),
    ("gate_check/pair_variables_per_witnesses_base",
     lambda L: _gates(L, {D + 4: 0 | 1025 << 32, D + 5: (1 << 20) + 1})),
    ("gate_check/pair_inverse_slot_16", lambda L: _gates(L, {I: lambda w: (w & ~0xffff) | 16 << 8 | 6})),
    ("gate_check/pair_slot_16_operand", lambda L: _gates(L, {I: lambda w: _a(4, 1)((w & ~0xff00) | 16 << 8)})),
    ("gate_check/pair_operand_unary", lambda L: _gates(L, {I: lambda w: _a(4, 1)(_op(1)(w))})),
    ("gate_check/pair_gate_0_write_gate_1_reps", lambda L: _gates(L, {W: 3 << 21 | 9, D + 10: 0 | 2 << 32})),
    ("gate_check/pair_gate_1_path_term_count", lambda L: _gates(L, {D + 10: 1 | 9 << 32, S + 5: 5})),
    ("gate_check/pair_term_count_head_selector", lambda L: _gates(L, {S + 5: 5, S + 6: 1})),
    # a native segment, in the order of its checks
    ("gate_check/native_kind_2", lambda L: _native(L, {S + 7: 2})),
    ("gate_check/native_two_gates", lambda L: _native(L, {S: 2}, extra=8)),
    ("gate_check/native_instructions", lambda L: _native(L, {S + 1: 1}, extra=1)),
    ("gate_check/native_writes", lambda L: _native(L, {S + 2: 1}, extra=1)),
    ("gate_check/native_immediates", lambda L: _native(L, {S + 3: 1}, extra=1)),
    ("gate_check/native_instr_range", lambda L: _native(L, {D: 1})),
    ("gate_check/native_117_terms_per_rep", lambda L: _native(L, {D + 1: 117 << 32})),
    ("gate_check/native_reps_0", lambda L: _native(L, {D + 2: 0 | 2 << 32})),
    ("gate_check/native_reps_over_2_20", lambda L: _native(L, {D + 2: (1 << 20) + 1 | 2 << 32})),
    ("gate_check/native_path_9", lambda L: _native(L, {D + 2: 2 | 9 << 32})),
    ("gate_check/native_mask_outside_path", lambda L: _native(L, {D + 3: 4})),
    ("gate_check/native_term_count", lambda L: _native(L, {S + 5: 118})),
    ("gate_check/native_head_selector_3_of_2", lambda L: _native(L, {S + 6: 3})),
    ("gate_check/native_nw_107", lambda L: _native(L, {D + 7: 107})),
    ("gate_check/native_variables_base_over_2_20", lambda L: _native(L, {D + 4: (1 << 20) + 1 | 125 << 32})),
    ("gate_check/native_witnesses_per_over_2_10", lambda L: _native(L, {D + 5: 0 | 1025 << 32})),
    ("gate_check/native_constants_per_over_2_10", lambda L: _native(L, {D + 6: 2 | 1025 << 32})),
    ("gate_check/native_variables_narrow", lambda L: _native(L, {D + 4: 0 | 124 << 32})),
    ("gate_check/native_witnesses_narrow", lambda L: _native(L, {D + 5: 0 | 4 << 32})),
    ("gate_check/native_pair_kind_two_gates", lambda L: _native(L, {S + 7: 2, S: 2}, extra=8)),
    ("gate_check/native_pair_two_gates_instructions", lambda L: _native(L, {S: 2, S + 1: 1}, extra=9)),
    ("gate_check/native_pair_immediates_range", lambda L: _native(L, {S + 3: 1, D: 1}, extra=1)),
    ("gate_check/native_pair_range_reps_0", lambda L: _native(L, {D + 1: 117 << 32, D + 2: 0 | 2 << 32})),
    ("gate_check/native_pair_reps_0_path_9", lambda L: _native(L, {D + 2: 0 | 9 << 32})),
    ("gate_check/native_pair_mask_term_count", lambda L: _native(L, {D + 3: 4, S + 5: 118})),
    ("gate_check/native_pair_term_count_head_selector", lambda L: _native(L, {S + 5: 118, S + 6: 3})),
    ("gate_check/native_pair_head_selector_nw", lambda L: _native(L, {S + 6: 3, D + 7: 107})),
    ("gate_check/native_pair_nw_variables_base",
     lambda L: _native(L, {D + 7: 107, D + 4: (1 << 20) + 1 | 125 << 32})),
    ("gate_check/native_pair_variables_narrow_witnesses_per",
     lambda L: _native(L, {D + 4: 0 | 124 << 32, D + 5: 0 | 1025 << 32})),
    ("gate_check/native_pair_witnesses_narrow_constants_per",
     lambda L: _native(L, {D + 5: 0 | 4 << 32, D + 6: 2 | 1025 << 32})),
    ("gate_check/native_pair_variables_base_narrow", lambda L: _native(L, {D + 4: (1 << 20) + 1 | 124 << 32})),
]
DEVICE = []
