"""The quotient's gate terms on the GPU: captured relation programs evaluated over LDE columns
that stay on the device (bj_quotient_gate_terms_d, csrc/gates.hip).

The circuit stays the caller's.  What the library takes is what the reference's
gpu_synthesizer/mod.rs captures from an evaluator's `evaluate_once`:

* `Index` and `Relation`, with the reference's names and fields (mod.rs:113-133);
* `TracingField`, the counterpart of GpuSynthesizerFieldLike (mod.rs:199-338): a field-like whose
  operations record relations instead of computing;
* `capture(evaluator)` -> `GateProgram` (GPUDataCapture::from_evaluator, mod.rs:386-444): the
  relations, the writes in push order and num_quotient_terms;
* `GatePlacement`: a program with its repetitions, PerChunkOffset, initial offsets, selector path
  and constants offset; `layout_general_purpose` / `specialized_placement` fill these in as the
  reference does for a CSGeometry;
* `compile_gate_set` (host only): slot allocation by liveness, the split into launches and the
  upload image; `GateSet`: validation (bj_gate_set_check_h) and the one upload;
* native segments: an evaluator that declares a `native_kind` (`Poseidon2FlattenedGate`, whose
  capture passes every cap of a launch) is not captured; it gets a segment of its own that names the
  kind, and the library runs a written-out kernel on it (csrc/gates_poseidon2.hpp);
* library segments (opt-in, `native_library=True`): a captured gate whose `program_digest` equals
  the one the library stores under the evaluator's name (`library_gate_info`) goes into a segment of
  kind 3 that names it by id, and the library runs the straight-line code generated from that
  capture (tools/gen_gate_library.py -> csrc/gates_library.hpp);
* `evaluate_gate_terms`: dst += the gate terms, one launch per segment;
* `check_if_satisfied` -> `SatisfiabilityReport`: the reference's check_if_satisfied
  (cs/implementations/satisfiability_test.rs:15-353) over the trace columns, on the device
  (bj_gate_set_satisfied_d): the number of unsatisfied (row, term) pairs and the first one's row,
  gate, subinstance, term and value; `GateSet.locate_term` maps the running term index back.

The evaluators at the end are written as plain functions over a field-like, so the same function
runs over `TracingField` to give the program and over any other field-like (the tests' Python
integers) to give the values; each restates the reference's `evaluate_once`.  There is no CPU
fallback: nothing here evaluates a program.
"""
import ctypes
import os
import re

import numpy as np
import torch

from ._lib import call, load
from .field import P, log2_exact, new_status, read_status, stream_of, to_device

MAX_SLOTS = 16              # BJ_GATE_MAX_SLOTS
MAX_SELECTOR_DEPTH = 8      # BJ_GATE_MAX_SELECTOR_DEPTH
MAX_INSTRUCTIONS = 4096     # BJ_GATE_MAX_INSTRUCTIONS, also the writes and the immediates of a launch
MAX_GATES = 64              # BJ_GATE_MAX_GATES
MAX_SEGMENTS = 64           # BJ_GATE_MAX_SEGMENTS
MAGIC = 0x3153455441474A42  # "BJGATES1"
KIND_INTERPRETED, KIND_POSEIDON2 = 0, 1   # word [7] of a segment head
KIND_LIBRARY = 3                          # a segment of library gates (csrc/gates_library.hpp); 2 stays refused

_KINDS = ("VariablePoly", "WitnessPoly", "ConstantPoly", "TemporaryValue", "ConstantValue")
_RELATIONS = ("Add", "Double", "Sub", "Negate", "Mul", "Square", "Inverse")
_UNARY = ("Double", "Negate", "Square", "Inverse")


class Index(tuple):
    """gpu_synthesizer::Index: Index.VariablePoly(i), .WitnessPoly(i), .ConstantPoly(i),
    .TemporaryValue(i), .ConstantValue(f)."""
    __slots__ = ()
    kind = property(lambda self: self[0])
    value = property(lambda self: self[1])

    def __repr__(self):
        return "%s(%d)" % self


class Relation(tuple):
    """gpu_synthesizer::Relation: Relation.Add(a, b), .Double(a), .Sub(a, b), .Negate(a),
    .Mul(a, b), .Square(a), .Inverse(a) over Index operands."""
    __slots__ = ()
    kind = property(lambda self: self[0])
    operands = property(lambda self: tuple(self[1:]))

    def __repr__(self):
        return "%s(%s)" % (self[0], ", ".join(repr(o) for o in self[1:]))


def _index_ctor(kind):
    def make(value):
        value = int(value)
        if kind == "ConstantValue":
            value %= P
        elif value < 0:
            raise ValueError("%s index must not be negative" % kind)
        return Index((kind, value))
    return staticmethod(make)


def _relation_ctor(kind):
    def make(*operands):
        if len(operands) != (1 if kind in _UNARY else 2) or not all(isinstance(o, Index) for o in operands):
            raise TypeError("Relation.%s takes %d Index operands" % (kind, 1 if kind in _UNARY else 2))
        return Relation((kind,) + tuple(operands))
    return staticmethod(make)


for _k in _KINDS:
    setattr(Index, _k, _index_ctor(_k))
for _k in _RELATIONS:
    setattr(Relation, _k, _relation_ctor(_k))


class TracingContext:
    """GPUVariablesGlobalContext (mod.rs:135-163): the temporary counter and the relations."""

    def __init__(self):
        self.counter = 0
        self.relations = []   # (TemporaryValue index, Relation)

    def push(self, relation):
        idx = self.counter
        self.counter += 1
        self.relations.append((idx, relation))
        return Index.TemporaryValue(idx)


class TracingField:
    """GpuSynthesizerFieldLike: the PrimeFieldLike surface the evaluators use.  The *_assign
    operations, double, negate and square replace the receiver by a fresh temporary and return it,
    as the reference's `&mut self` forms do; `copy()` is Rust's copy of a Copy value."""
    __slots__ = ("idx", "ctx")

    def __init__(self, idx, ctx):
        self.idx, self.ctx = idx, ctx

    def copy(self):
        return TracingField(self.idx, self.ctx)

    def zero(self):
        return TracingField(Index.ConstantValue(0), self.ctx)

    def one(self):
        return TracingField(Index.ConstantValue(1), self.ctx)

    def minus_one(self):
        return TracingField(Index.ConstantValue(P - 1), self.ctx)

    def constant(self, value):
        return TracingField(Index.ConstantValue(value), self.ctx)

    def _record(self, relation):
        self.idx = self.ctx.push(relation)
        return self

    def add_assign(self, other):
        return self._record(Relation.Add(self.idx, other.idx))

    def sub_assign(self, other):
        return self._record(Relation.Sub(self.idx, other.idx))

    def mul_assign(self, other):
        return self._record(Relation.Mul(self.idx, other.idx))

    def double(self):
        return self._record(Relation.Double(self.idx))

    def negate(self):
        return self._record(Relation.Negate(self.idx))

    def square(self):
        return self._record(Relation.Square(self.idx))

    def inverse(self):
        return TracingField(self.ctx.push(Relation.Inverse(self.idx)), self.ctx)

    def mul_by_base(self, value):
        """A product with a base-field constant (mul_all_by_base on a scalar field-like)."""
        return self._record(Relation.Mul(self.idx, Index.ConstantValue(value)))

    def mul_and_accumulate_into(self, a, b):
        """PrimeFieldLike::mul_and_accumulate_into(acc = self, a, b) (field_like.rs:71-75)."""
        tmp = a.copy()
        tmp.mul_assign(b)
        return self.add_assign(tmp)


class TracingSource:
    """GPUPolyStorage (mod.rs:19-91) at chunk offset zero: the repetition's offset is applied by
    the device, not recorded."""

    def __init__(self, ctx):
        self.ctx = ctx

    def get_variable_value(self, i):
        return TracingField(Index.VariablePoly(i), self.ctx)

    def get_witness_value(self, i):
        return TracingField(Index.WitnessPoly(i), self.ctx)

    def get_constant_value(self, i):
        return TracingField(Index.ConstantPoly(i), self.ctx)

    def field(self):
        """A field-like to draw zero / one / constants from."""
        return TracingField(Index.ConstantValue(0), self.ctx)


class TracingDestination:
    """GPUPolyDestination (mod.rs:35-111)."""

    def __init__(self):
        self.writes = []

    def push_evaluation_result(self, value):
        self.writes.append(value.idx)


class GateProgram:
    """GPUDataCapture's relations, writes_per_repetition and num_quotient_terms."""

    def __init__(self, relations, writes, num_quotient_terms, evaluator=None):
        self.relations = list(relations)
        self.writes = list(writes)
        self.num_quotient_terms = num_quotient_terms
        self.evaluator = evaluator
        if len(self.writes) != num_quotient_terms:
            raise ValueError("%d writes for %d quotient terms" % (len(self.writes), num_quotient_terms))


def capture(evaluator):
    """GPUDataCapture::from_evaluator (mod.rs:386-444)."""
    ctx = TracingContext()
    src, dst = TracingSource(ctx), TracingDestination()
    shared = evaluator.load_row_shared_constants(src)
    evaluator.evaluate_once(src, dst, shared)
    return GateProgram(ctx.relations, dst.writes, evaluator.num_quotient_terms, evaluator)


_FNV_OFFSET, _FNV_PRIME = 0xCBF29CE484222325, 0x100000001B3


def program_digest(program):
    """FNV-1a-64 of a captured program, the number the library stores per gate it has generated code for
    (tools/gen_gate_library.py -> csrc/gates_library.hpp) and compile_gate_set compares before it lets a
    placement name a library entry.  The bytes hashed, integers little-endian:

      u32 number of relations, u32 number of writes,
      per relation in order: u8 opcode (Relation's order: 0 Add .. 6 Inverse), u32 destination
      TemporaryValue index, u8 number of operands, then per operand u8 kind (Index's order:
      0 VariablePoly, 1 WitnessPoly, 2 ConstantPoly, 3 TemporaryValue, 4 ConstantValue) and u64 value
      (the index, or the canonical constant),
      u8 0xFF,
      per write in push order: u8 kind, u64 value.

    Names, placement and num_quotient_terms (the number of writes) are not part of it."""
    def operand(o):
        return bytes([_KINDS.index(o.kind)]) + int(o.value).to_bytes(8, "little")

    data = [len(program.relations).to_bytes(4, "little"), len(program.writes).to_bytes(4, "little")]
    for dst, rel in program.relations:
        data.append(bytes([_RELATIONS.index(rel.kind)]) + int(dst).to_bytes(4, "little") + bytes([len(rel.operands)]))
        data += [operand(o) for o in rel.operands]
    data.append(b"\xff")
    data += [operand(o) for o in program.writes]
    h = _FNV_OFFSET
    for byte in b"".join(data):
        h = (h ^ byte) * _FNV_PRIME & 0xFFFFFFFFFFFFFFFF
    return h


class NativeGateProgram:
    """What stands for the capture of an evaluator with a native kind: nothing is recorded, the
    library knows the gate."""
    relations = writes = None

    def __init__(self, evaluator):
        if not getattr(evaluator, "native_kind", KIND_INTERPRETED):
            raise ValueError("the evaluator declares no native kind")
        self.evaluator = evaluator
        self.num_quotient_terms = evaluator.num_quotient_terms


def program_of(evaluator):
    """The program a placement carries: the capture, or for a native kind its stand-in."""
    if getattr(evaluator, "native_kind", KIND_INTERPRETED):
        return NativeGateProgram(evaluator)
    return capture(evaluator)


def native_gate_info(kind):
    """bj_gate_native_info_h: (cells, terms, degree, most witness cells) of a native kind, or None
    when the library is older than native segments or does not know the kind."""
    fn = getattr(load(), "bj_gate_native_info_h", None)
    out = (ctypes.c_uint64 * 4)()
    if fn is None or fn(kind, out) != 0:
        return None
    return tuple(int(v) for v in out)


def library_gate_info(name):
    """bj_gate_library_find_h: (id, terms per repetition, variable, witness and constant columns one
    repetition reads, digest of the capture the code was generated from) of the library gate `name`,
    or None when the library is older than library segments or does not know the name."""
    fn = getattr(load(), "bj_gate_library_find_h", None)
    out = (ctypes.c_uint64 * 6)()
    if fn is None or name is None or fn(str(name).encode(), out) != 0:
        return None
    return tuple(int(v) for v in out)


# ------------------------------------------------------------------ placement
class PerChunkOffset:
    """cs/traits/evaluator.rs PerChunkOffset."""

    def __init__(self, variables_offset=0, witnesses_offset=0, constants_offset=0):
        self.variables_offset = variables_offset
        self.witnesses_offset = witnesses_offset
        self.constants_offset = constants_offset

    def as_tuple(self):
        return (self.variables_offset, self.witnesses_offset, self.constants_offset)


class CSGeometry:
    def __init__(self, num_columns_under_copy_permutation, num_witness_columns, num_constant_columns,
                 max_allowed_constraint_degree):
        self.num_columns_under_copy_permutation = num_columns_under_copy_permutation
        self.num_witness_columns = num_witness_columns
        self.num_constant_columns = num_constant_columns
        self.max_allowed_constraint_degree = max_allowed_constraint_degree


class GatePlacement:
    """One gate of a set.  selector_path: the list of booleans of compute_selector_subpath, level i
    reading constant column i (empty: a selector of one).  constants_offset: where the gate's own
    constants start -- len(selector_path) for a general-purpose gate, and for a specialized one the
    constants of the general-purpose set (initial_offset's constants are added on top)."""

    def __init__(self, program, num_repetitions=1, per_chunk_offset=None, selector_path=(), constants_offset=None,
                 initial_offset=None):
        self.program = program
        self.num_repetitions = int(num_repetitions)
        if per_chunk_offset is None:
            per_chunk_offset = program.evaluator.per_chunk_offset if program.evaluator else PerChunkOffset()
        self.per_chunk_offset = per_chunk_offset
        self.selector_path = [bool(b) for b in selector_path]
        self.constants_offset = len(self.selector_path) if constants_offset is None else int(constants_offset)
        self.initial_offset = initial_offset or PerChunkOffset()

    def bases(self):
        v, w, c = self.initial_offset.as_tuple()
        return (v, w, self.constants_offset + c)

    def num_terms(self):
        return self.num_repetitions * self.program.num_quotient_terms


def layout_general_purpose(evaluators_with_paths, geometry):
    """The general-purpose gates of a set: (evaluator, selector path) pairs in evaluation order ->
    placements with the geometry's repetition counts and constants_offset = len(path)
    (prover.rs:996-1015)."""
    return [GatePlacement(program_of(e), e.num_repetitions_in_geometry(geometry), e.per_chunk_offset, path)
            for e, path in evaluators_with_paths]


def specialized_placement(evaluator, num_repetitions, share_constants, initial_offset,
                          constants_for_gates_over_general_purpose_columns):
    """GatePlacementStrategy::UseSpecializedColumns (prover.rs:692-772): no selector, the source
    narrowed to the columns from initial_offset on, the constants after the general-purpose ones;
    with share_constants the repetitions do not advance the constants (:750-752)."""
    v, w, c = evaluator.principal_width
    per = PerChunkOffset(v, w, 0 if share_constants else c)
    return GatePlacement(program_of(evaluator), num_repetitions, per, (),
                         constants_for_gates_over_general_purpose_columns, initial_offset)


# ------------------------------------------------------------------ slot allocation and the image
_OPCODE = {k: i for i, k in enumerate(_RELATIONS)}
_KIND_CODE = {"VariablePoly": 0, "WitnessPoly": 1, "ConstantPoly": 2}
_K_SLOT, _K_IMM, _IDX_BITS = 3, 4, 21


def allocate_slots(program, cap=MAX_SLOTS):
    """Liveness analysis and slot reuse: TemporaryValue index -> slot, for every relation in order.
    A temporary is live from the relation that defines it to its last read; one that is pushed to
    the destination stays live to the end, because the terms are formed after the program has run.
    An instruction reads its operands before it writes, so its destination may take the slot of an
    operand that dies there.  Returns (slots, used): slots[i] the slot of relation i's destination,
    used the number of distinct slots.  ValueError when more than cap values are live at once, or a
    temporary is read before it is defined."""
    end = len(program.relations)
    last = {}
    defined = set()
    for i, (dst, rel) in enumerate(program.relations):
        for o in rel.operands:
            if o.kind == "TemporaryValue":
                if o.value not in defined:
                    raise ValueError("TemporaryValue(%d) is read before it is written" % o.value)
                last[o.value] = i
        if dst in defined:
            raise ValueError("TemporaryValue(%d) is written twice" % dst)
        defined.add(dst)
    for o in program.writes:
        if o.kind == "TemporaryValue":
            if o.value not in defined:
                raise ValueError("TemporaryValue(%d) is pushed but never written" % o.value)
            last[o.value] = end
    free, slot_of, slots, used = [], {}, [], 0
    for i, (dst, rel) in enumerate(program.relations):
        for o in set(rel.operands):
            if o.kind == "TemporaryValue" and last[o.value] == i:
                free.append(slot_of[o.value])
        if free:
            s = min(free)
            free.remove(s)
        else:
            s = used
            used += 1
            if used > cap:
                raise ValueError("more than %d temporaries are live at relation %d" % (cap, i))
        slot_of[dst] = s
        slots.append(s)
        if dst not in last:   # never read: dead at once
            free.append(s)
    return slots, used


class _Segment:
    def __init__(self, alpha_base):
        self.alpha_base = alpha_base
        self.desc, self.instr, self.writes, self.imm = [], [], [], []
        self.imm_index = {}
        self.terms = 0
        self.depth = 0
        self.kind = KIND_INTERPRETED

    def words(self):
        head = [len(self.desc) // 8, len(self.instr), len(self.writes), len(self.imm), self.alpha_base, self.terms,
                self.depth, self.kind]
        return head + self.desc + self.instr + self.writes + self.imm


def _placement_words(pl):
    """Words [2] .. [6] of a descriptor: repetitions | path length << 32, the path's mask, three base | per << 32."""
    path = pl.selector_path
    if len(path) > 63:
        raise ValueError("selector path too long")
    return [pl.num_repetitions | len(path) << 32, sum(1 << i for i, b in enumerate(path) if b)] + \
        [base | per << 32 for base, per in zip(pl.bases(), pl.per_chunk_offset.as_tuple())]


def _encode_gate(seg, pl, cap):
    """Appends one gate to a segment; returns False (segment untouched) when it does not fit."""
    prog = pl.program
    slots, _ = allocate_slots(prog, cap)
    imm, imm_index = list(seg.imm), dict(seg.imm_index)
    slot_of = {}

    def operand(o):
        if o.kind == "TemporaryValue":
            return _K_SLOT << _IDX_BITS | slot_of[o.value]
        if o.kind == "ConstantValue":
            if o.value not in imm_index:
                imm_index[o.value] = len(imm)
                imm.append(o.value)
            return _K_IMM << _IDX_BITS | imm_index[o.value]
        if o.value >> _IDX_BITS:
            raise ValueError("%r: index too large" % (o,))
        return _KIND_CODE[o.kind] << _IDX_BITS | o.value

    instr = []
    for (dst, rel), s in zip(prog.relations, slots):
        ops = [operand(o) for o in rel.operands]
        slot_of[dst] = s
        instr.append(_OPCODE[rel.kind] | s << 8 | ops[0] << 16 | (ops[1] << 40 if len(ops) > 1 else 0))
    writes = [operand(o) for o in prog.writes]
    if (len(seg.desc) // 8 + 1 > MAX_GATES or len(seg.instr) + len(instr) > MAX_INSTRUCTIONS
            or len(seg.writes) + len(writes) > MAX_INSTRUCTIONS or len(imm) > MAX_INSTRUCTIONS):
        return False
    i0, w0 = len(seg.instr), len(seg.writes)
    seg.desc += [i0 | (i0 + len(instr)) << 32, w0 | (w0 + len(writes)) << 32] + _placement_words(pl) + [0]
    seg.instr += instr
    seg.writes += writes
    seg.imm, seg.imm_index = imm, imm_index
    seg.terms += pl.num_terms()
    seg.depth = max(seg.depth, len(pl.selector_path))
    return True


def _native_kind(pl):
    return getattr(pl.program.evaluator, "native_kind", KIND_INTERPRETED)


def _encode_native(seg, pl, kind):
    """The one gate of a native segment: no program, the descriptor's words [2] .. [6] as for an
    interpreted gate, [1] the terms per repetition with no writes behind them, [7] the evaluator's
    num_witness_columns_used."""
    info = native_gate_info(kind)
    if info is None:   # a library from before native segments: the gate can only be refused
        raise ValueError("one gate exceeds the caps of a launch")
    cells, terms, _, most_witnesses = info
    evaluator = pl.program.evaluator
    nw = evaluator.num_witness_columns_used
    per = pl.per_chunk_offset.as_tuple()
    if terms != evaluator.num_quotient_terms or not 0 <= nw <= most_witnesses:
        raise ValueError("%s does not match the library's native kind %d" % (evaluator.name, kind))
    if per[0] < cells - nw or per[1] < nw:
        raise ValueError("a repetition of %s is narrower than its %d cells" % (evaluator.name, cells))
    seg.desc += [0, terms << 32] + _placement_words(pl) + [nw]
    seg.kind = kind
    seg.terms = pl.num_terms()
    seg.depth = len(pl.selector_path)


def _library_entry(pl):
    """The library's entry for a placement's gate -- bj_gate_library_find_h's tuple -- or None: the
    evaluator has a native kind of its own, the library does not know its name, or the capture is
    not the one the library's code was generated from (a same-named evaluator that records other
    relations stays interpreted)."""
    prog = pl.program
    if _native_kind(pl) or prog.evaluator is None or prog.relations is None:
        return None
    info = library_gate_info(prog.evaluator.name)
    if info is None or info[1] != prog.num_quotient_terms or info[5] != program_digest(prog):
        return None
    return info


def _encode_library(seg, pl, info):
    """One gate of a library segment: [0] the library id, [1] the terms per repetition with no writes
    behind them, [2] .. [6] the placement as for every gate, [7] 0."""
    seg.desc += [info[0], info[1] << 32] + _placement_words(pl) + [0]
    seg.kind = KIND_LIBRARY
    seg.terms += pl.num_terms()
    seg.depth = max(seg.depth, len(pl.selector_path))


def compile_gate_set(placements, slot_cap=MAX_SLOTS, native_library=False):
    """Placements in evaluation order -> the upload image, a list of u64 words
    (include/boojum_mi355x.h, "quotient gate terms").  Gates fill a segment until a cap of one launch
    would be passed; the next segment's alpha base carries the challenge index on.  A placement
    whose evaluator declares a native kind closes the segment before it and takes one of its own,
    uncaptured.  With native_library, a placement whose capture is one the library has generated code
    for (_library_entry) goes into a library segment instead of an interpreted one; consecutive ones
    share a segment of up to MAX_GATES gates.  The order of the placements, and so the challenge
    index, is the same whatever the kinds.  Host only."""
    placements = list(placements)
    if not placements:
        raise ValueError("a gate set holds at least one gate with quotient terms")
    segments, seg = [], _Segment(0)

    def close():   # a segment that holds a gate is done; the next one carries the challenge index on
        nonlocal seg
        if seg.desc:
            segments.append(seg)
            seg = _Segment(seg.alpha_base + seg.terms)

    for pl in placements:
        if pl.program.num_quotient_terms == 0:
            raise ValueError("a gate without quotient terms never reaches the library (prover.rs:922-994)")
        entry = _library_entry(pl) if native_library else None
        if _native_kind(pl):
            close()
            _encode_native(seg, pl, _native_kind(pl))
            close()
        elif entry is not None:
            if seg.kind != KIND_LIBRARY or len(seg.desc) // 8 == MAX_GATES:
                close()
            _encode_library(seg, pl, entry)
        else:
            if seg.kind == KIND_LIBRARY:
                close()
            if not _encode_gate(seg, pl, slot_cap):
                empty = not seg.desc   # an empty segment did not take the gate: none will
                close()
                if empty or not _encode_gate(seg, pl, slot_cap):
                    raise ValueError("one gate exceeds the caps of a launch")
    close()
    image = [MAGIC, len(segments)] + [0] * len(segments)
    for i, s in enumerate(segments):
        image[2 + i] = len(image)
        image += s.words()
    return image


def check_image(image):
    """bj_gate_set_check_h: the library's validator on a host image, no device.  Returns the dict
    of what the image needs; raises BoojumError (BJ_EINVAL) for a malformed one."""
    words = (ctypes.c_uint64 * len(image))(*image)
    need = (ctypes.c_uint64 * 5)()
    call("bj_gate_set_check_h", words, len(image), need)
    return dict(variables=need[0], witnesses=need[1], constants=need[2], alphas=need[3], segments=need[4])


class TermMap:
    """The running term index k of a set (the index of the challenges) -> (gate, subinstance, term):
    host arithmetic over the descriptors of an image.  Gates count on across segments, so `gate` is
    the index into the placements the image was compiled from; a gate's terms run repetition by
    repetition, its writes in push order within each."""

    def __init__(self, image):
        self.gates = []   # (first k, repetitions, terms per repetition), in order
        k = 0
        for s in range(image[1]):
            seg = image[2 + s]
            if image[seg + 4] != k:
                raise ValueError("a segment's alpha base is not the sum of the terms before it")
            for g in range(image[seg]):
                d = seg + 8 + 8 * g
                writes = (image[d + 1] >> 32) - (image[d + 1] & 0xffffffff)
                reps = image[d + 2] & 0xffffffff
                if writes <= 0 or reps == 0:
                    raise ValueError("a gate without terms or repetitions")
                self.gates.append((k, reps, writes))
                k += reps * writes
        self.num_terms = k

    def locate(self, k):
        k = int(k)
        if not 0 <= k < self.num_terms:
            raise IndexError("term %d of %d" % (k, self.num_terms))
        lo, hi = 0, len(self.gates) - 1
        while lo < hi:   # the last gate whose first k is <= k
            mid = (lo + hi + 1) // 2
            if self.gates[mid][0] <= k:
                lo = mid
            else:
                hi = mid - 1
        first, _, writes = self.gates[lo]
        return lo, (k - first) // writes, (k - first) % writes


class GateSet:
    """Slot allocation, validation and the single upload of a gate set; keeps the device buffer
    alive until it is collected or `release()`d.  `GateSet.from_image` uploads a prepared image.
    native_library: compile_gate_set's flag, library segments for the gates the library has code for."""

    def __init__(self, placements, slot_cap=MAX_SLOTS, native_library=False):
        self._handle = None
        self.placements = list(placements)
        self._upload(compile_gate_set(self.placements, slot_cap, native_library))

    @classmethod
    def from_image(cls, image):
        self = cls.__new__(cls)
        self._handle = None
        self.placements = None
        self._upload(list(image))
        return self

    def _upload(self, image):
        self.image = image
        self.need = check_image(image)
        self.term_map = TermMap(image)
        handle = ctypes.c_void_p()
        call("bj_gate_set_upload_d", (ctypes.c_uint64 * len(image))(*image), len(image), ctypes.byref(handle))
        self._handle = handle
        self.num_segments = self.need["segments"]
        self.num_terms = self.need["alphas"]

    def locate_term(self, k):
        """The running term index k -> (gate, subinstance, term): the index into the set's
        placements, the repetition and the term within it (TermMap)."""
        return self.term_map.locate(k)

    def gate_name(self, gate):
        """The name of the evaluator of placement `gate`; None for an uploaded image or a program
        that was not captured from an evaluator."""
        if self.placements is None:
            return None
        evaluator = self.placements[gate].program.evaluator
        return evaluator.name if evaluator is not None else None

    def release(self):
        if self._handle is not None:
            handle, self._handle = self._handle, None
            load().bj_gate_set_release(handle)

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


def _view(t, what, rank, shape):
    """t.shape, after the check behind _lde and _trace: u64 words on the device in `rank` dimensions."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype not in (torch.int64, torch.uint64):
        raise TypeError("%s: expected an int64 CUDA tensor of u64 field elements" % what)
    if t.dim() != rank:
        raise ValueError("%s: %s" % (what, shape))
    return t.shape


def _lde(t, q, what):
    """(data pointer, column stride, columns, n) of a (C, D, n) LDE."""
    c, d, n = _view(t, what, 3, "an LDE is (C, D, n)")
    if d < q:
        raise ValueError("%s: the LDE has %d cosets, the quotient degree is %d" % (what, d, q))
    if t.stride(2) != 1 or (d > 1 and t.stride(1) != n):
        raise ValueError("%s: the cosets of an LDE column must be contiguous" % what)
    return t.data_ptr(), (t.stride(0) if c > 1 else d * n), c, n


def _trace(t, what):
    """(data pointer, column stride, columns, n) of (C, n) trace columns."""
    c, n = _view(t, what, 2, "trace columns are (C, n)")
    if n and t.stride(1) != 1:
        raise ValueError("%s: the rows of a trace column must be contiguous" % what)
    return t.data_ptr(), (t.stride(0) if c > 1 else n), c, n


def _bind(view, **tensors):
    """The variables, witnesses and constants of a call, each through `view` (_lde or _trace) under its argument's
    name, None for a kind the set never names: the nine column arguments of the C calls and the set of row counts."""
    args, sizes = [], set()
    for what, t in tensors.items():
        p, stride, c, n = (None, 0, 0, None) if t is None else view(t, what)
        args += [p, stride, c]
        sizes.add(n)
    return args, sizes - {None}


def challenges_tensor(alphas, device):
    """Ext2 challenges [(c0, c1), ...] -> the (K, 2) device tensor the call reads."""
    flat = [int(limb) % P for pair in alphas for limb in pair]
    return to_device(np.array(flat, dtype=np.uint64).reshape(-1, 2), device)


def evaluate_gate_terms(gate_set, variables_lde, witnesses_lde, constants_lde, alphas, quotient_degree, dst_c0,
                        dst_c1):
    """dst += the gate terms of every segment of gate_set (bj_quotient_gate_terms_d, one launch
    each).  The LDEs are (C, D, n) tensors read in place at their first quotient_degree cosets;
    one the set never names may be None.  alphas: the set's Ext2 challenge powers, a list of
    (c0, c1) pairs (copied to the device here) or a (K, 2) device tensor (read in place, so a
    captured graph sees later contents).  dst_c0, dst_c1: q * n words each."""
    log_q = log2_exact(quotient_degree)
    columns, sizes = _bind(lambda t, what: _lde(t, quotient_degree, what), variables_lde=variables_lde,
                           witnesses_lde=witnesses_lde, constants_lde=constants_lde)
    total = dst_c0.numel()
    n = sizes.pop() if sizes else total // quotient_degree
    if sizes or n * quotient_degree != total:
        raise ValueError("the LDEs and the accumulator disagree on the domain size")
    for d in (dst_c0, dst_c1):
        if not d.is_cuda or d.dtype not in (torch.int64, torch.uint64) or d.numel() != total or not d.is_contiguous():
            raise ValueError("an accumulator half holds q * n = %d contiguous words on the device" % total)
    if not isinstance(alphas, torch.Tensor):
        alphas = challenges_tensor(alphas, dst_c0.device)
    if not alphas.is_cuda or alphas.dim() != 2 or alphas.shape[1] != 2 or not alphas.is_contiguous() \
            or alphas.dtype not in (torch.int64, torch.uint64):
        raise ValueError("alphas: a contiguous (K, 2) int64 device tensor")
    for segment in range(gate_set.num_segments):
        call("bj_quotient_gate_terms_d", gate_set._handle, segment, *columns, alphas.data_ptr(), alphas.shape[0],
             log2_exact(n), log_q, dst_c0.data_ptr(), dst_c1.data_ptr(), stream_of(dst_c0))


# ------------------------------------------------------------------ satisfiability check
CHECK_BEGIN = 0x80000000    # BJ_GATE_CHECK_BEGIN
_NO_KEY = (1 << 64) - 1


class SatisfiabilityReport:
    """What check_if_satisfied found.  satisfied; num_unsatisfied, the exact number of (row, term)
    pairs with selector * term != 0 in the window; and, for the first of them in (row, k) order:
    row, gate (index into the set's placements), gate_name (the evaluator's name, None for
    GateSet.from_image), subinstance (the repetition), term (within the repetition), k (the running
    term index) and value (the term's canonical value).  All None but the first two when
    satisfied."""

    def __init__(self, num_unsatisfied, row=None, gate=None, gate_name=None, subinstance=None, term=None, k=None,
                 value=None):
        self.satisfied = num_unsatisfied == 0
        self.num_unsatisfied = num_unsatisfied
        self.row, self.gate, self.gate_name = row, gate, gate_name
        self.subinstance, self.term, self.k, self.value = subinstance, term, k, value

    def message(self):
        """The reference's panic (satisfiability_test.rs:149-152), the value in GoldilocksField's
        Display form; None when satisfied.  A gate without a name is given by its index."""
        if self.satisfied:
            return None
        name = self.gate_name if self.gate_name is not None else "#%d" % self.gate
        return "Unsatisfied at row %d with value 0x%016x for term number %d for subinstance number %d of gate %s" % (
            self.row, self.value, self.term, self.subinstance, name)

    def __repr__(self):
        return "SatisfiabilityReport(satisfied)" if self.satisfied else \
            "SatisfiabilityReport(%d unsatisfied; %s)" % (self.num_unsatisfied, self.message())


def report_from_status(gate_set, status):
    """The 4 words of the status record of bj_gate_set_satisfied_d -> SatisfiabilityReport.
    gate_set: anything with locate_term and gate_name."""
    count, key, value = int(status[0]), int(status[1]), int(status[2])
    if count == 0:
        if key != _NO_KEY:
            raise ValueError("a status record without failures carries a key")
        return SatisfiabilityReport(0)
    row, k = key >> 32, key & 0xffffffff
    gate, subinstance, term = gate_set.locate_term(k)
    return SatisfiabilityReport(count, row, gate, gate_set.gate_name(gate), subinstance, term, k, value)


def check_if_satisfied(gate_set, variables, witnesses, constants, rows=None, status=None):
    """CSReferenceAssembly::check_if_satisfied (satisfiability_test.rs:15-353) on the device: every
    gate of gate_set on every row of the window, over the (C, n) trace columns the commitment takes
    (not an LDE); one the set never names may be None.  rows: a (begin, count) window, default the
    whole trace.  One bj_gate_set_satisfied_d call per segment on one status record (`status`: a
    4-word int64 device tensor to use for it), then one copy of its 4 words to the host, which
    synchronises.  Returns a SatisfiabilityReport."""
    columns, sizes = _bind(_trace, variables=variables, witnesses=witnesses, constants=constants)
    if len(sizes) != 1:
        raise ValueError("the trace columns disagree on the number of rows" if sizes else "no trace columns")
    n = sizes.pop()
    begin, count = (0, n) if rows is None else (int(rows[0]), int(rows[1]))
    if begin < 0 or count < 1 or begin + count > n:
        raise ValueError("rows (%d, %d): a window of at least one row inside the %d of the trace" % (begin, count, n))
    first = next(t for t in (variables, witnesses, constants) if t is not None)
    if status is None:
        status = new_status(first.device)
    elif not status.is_cuda or status.dtype not in (torch.int64, torch.uint64) or status.numel() != 4 \
            or not status.is_contiguous():
        raise ValueError("status: 4 contiguous int64 words on the device")
    for segment in range(gate_set.num_segments):
        call("bj_gate_set_satisfied_d", gate_set._handle, segment | (CHECK_BEGIN if segment == 0 else 0), *columns,
             begin, count, status.data_ptr(), stream_of(first))
    return report_from_status(gate_set, read_status(status))


# ------------------------------------------------------------------ evaluators
class Evaluator:
    """What the library needs of a GateConstraintEvaluator: num_quotient_terms,
    max_constraint_degree, the principal width (variables, witnesses, constants), placement_type's
    per_chunk_offset, num_repetitions_in_geometry, num_required_constants_in_geometry,
    load_row_shared_constants and evaluate_once.  Sources give field-likes with the TracingField
    surface; src.field() gives one to draw constants from."""
    name = ""
    num_quotient_terms = 1
    max_constraint_degree = 2
    principal_width = (0, 0, 0)
    native_kind = KIND_INTERPRETED   # a kind the library evaluates without a capture, or 0

    @property
    def per_chunk_offset(self):
        """MultipleOnRow: the principal width in variables and witnesses, no constants."""
        return PerChunkOffset(self.principal_width[0], self.principal_width[1], 0)

    def num_repetitions_in_geometry(self, geometry):
        return geometry.num_columns_under_copy_permutation // self.principal_width[0]

    def num_required_constants_in_geometry(self, geometry):
        return self.principal_width[2]

    def load_row_shared_constants(self, src):
        return ()

    def evaluate_once(self, src, dst, shared):
        raise NotImplementedError


class FmaGateInBaseFieldWithoutConstant(Evaluator):
    """c0 a b + c1 c - d (fma_gate_without_constant.rs:20-127): the two coefficients are row-shared
    constants 0 and 1 (:81-93), the term is c1 c + c0 (a b) - d (:108-125)."""
    name = "fma_gate_in_base_without_constant"
    max_constraint_degree = 3
    principal_width = (4, 0, 2)

    def load_row_shared_constants(self, src):
        return (src.get_constant_value(0), src.get_constant_value(1))

    def evaluate_once(self, src, dst, shared):
        a, b, c, d = (src.get_variable_value(i) for i in range(4))
        quadratic, linear = shared
        t = c.copy()
        t.mul_assign(linear)
        ab = a.copy()
        ab.mul_assign(b)
        t.mul_and_accumulate_into(quadratic, ab)
        t.sub_assign(d)
        dst.push_evaluation_result(t)


class BooleanConstraintGate(Evaluator):
    """a (1 - a) (boolean_allocator.rs:100-121)."""
    name = "boolean_constraint"
    principal_width = (1, 0, 0)

    def evaluate_once(self, src, dst, shared):
        a = src.get_variable_value(0)
        t = src.field().one()
        t.sub_assign(a)
        r = a.copy()
        r.mul_assign(t)
        dst.push_evaluation_result(r)


class ConstantsAllocatorGate(Evaluator):
    """a - constant (constant_allocator.rs:107-126); every repetition has its own constant, so the
    per-chunk offset advances the constants too (:54-62) and the repetitions are bounded by both
    column counts (:65-73)."""
    name = "constants_allocator"
    max_constraint_degree = 1
    principal_width = (1, 0, 1)

    @property
    def per_chunk_offset(self):
        return PerChunkOffset(1, 0, 1)

    def num_repetitions_in_geometry(self, geometry):
        return min(geometry.num_constant_columns, geometry.num_columns_under_copy_permutation)

    def num_required_constants_in_geometry(self, geometry):
        return geometry.num_constant_columns

    def evaluate_once(self, src, dst, shared):
        r = src.get_variable_value(0)
        r.sub_assign(src.get_constant_value(0))
        dst.push_evaluation_result(r)


class ReductionGate(Evaluator):
    """sum_i var_i constant_i - result (reduction_gate.rs:103-126), N row-shared constants
    (:91-100), N + 1 variables."""

    def __init__(self, n=4):
        self.n = n
        self.name = "reduction_gate_%d" % n
        self.principal_width = (n + 1, 0, n)

    def load_row_shared_constants(self, src):
        return tuple(src.get_constant_value(i) for i in range(self.n))

    def evaluate_once(self, src, dst, shared):
        r = src.field().zero()
        for i in range(self.n):
            r.mul_and_accumulate_into(src.get_variable_value(i), shared[i])
        r.sub_assign(src.get_variable_value(self.n))
        dst.push_evaluation_result(r)


class SelectionGate(Evaluator):
    """a s + (1 - s) b - result (selection_gate.rs:100-128)."""
    name = "selection_gate"
    principal_width = (4, 0, 0)

    def evaluate_once(self, src, dst, shared):
        a, b, s, result = (src.get_variable_value(i) for i in range(4))
        r = a.copy()
        r.mul_assign(s)
        t = src.field().one()
        t.sub_assign(s)
        r.mul_and_accumulate_into(t, b)
        r.sub_assign(result)
        dst.push_evaluation_result(r)


class ZeroCheckGate(Evaluator):
    """Two terms (zero_check.rs:143-176): flag + input * inverse - 1 and input * flag.  The
    inversion witness is variable 2, or witness column 0 when use_witness_column_for_inversion
    (:158-162), which also changes the width and the repetition count (:50-114)."""
    num_quotient_terms = 2

    def __init__(self, use_witness_column_for_inversion=False):
        self.use_witness_column_for_inversion = use_witness_column_for_inversion
        self.name = "zero_check_%s" % ("witness" if use_witness_column_for_inversion else "variable")
        self.principal_width = (2, 1, 0) if use_witness_column_for_inversion else (3, 0, 0)

    def num_repetitions_in_geometry(self, geometry):
        reps = geometry.num_columns_under_copy_permutation // self.principal_width[0]
        if self.use_witness_column_for_inversion:
            reps = min(reps, geometry.num_witness_columns)
        return reps

    def evaluate_once(self, src, dst, shared):
        one = src.field().one()
        inp, flag = src.get_variable_value(0), src.get_variable_value(1)
        inv = src.get_witness_value(0) if self.use_witness_column_for_inversion else src.get_variable_value(2)
        r = flag.copy()
        r.mul_and_accumulate_into(inp, inv)
        r.sub_assign(one)
        dst.push_evaluation_result(r)
        r = inp.copy()
        r.mul_assign(flag)
        dst.push_evaluation_result(r)


class DotProductGate(Evaluator):
    """sum_i a_i b_i - result over 2 N + 1 variables (dot_product_gate.rs:102-131)."""

    def __init__(self, n=4):
        self.n = n
        self.name = "dot_product_gate_%d" % n
        self.principal_width = (2 * n + 1, 0, 0)

    def evaluate_once(self, src, dst, shared):
        r = src.field().zero()
        for i in range(self.n):
            r.mul_and_accumulate_into(src.get_variable_value(2 * i), src.get_variable_value(2 * i + 1))
        r.sub_assign(src.get_variable_value(2 * self.n))
        dst.push_evaluation_result(r)


class ConditionalSwapGate(Evaluator):
    """2 N terms over 4 N + 1 variables (conditional_swap.rs:108-152): for each pair,
    b s + (1 - s) a - result_a and a s + (1 - s) b - result_b, the selector being variable 0."""

    def __init__(self, n=1):
        self.n = n
        self.name = "conditional_swap_gate_%d" % n
        self.num_quotient_terms = 2 * n
        self.principal_width = (4 * n + 1, 0, 0)

    def evaluate_once(self, src, dst, shared):
        s = src.get_variable_value(0)
        for i in range(self.n):
            a, b, ra, rb = (src.get_variable_value(4 * i + 1 + j) for j in range(4))
            for taken, other, result in ((b, a, ra), (a, b, rb)):
                r = taken.copy()
                r.mul_assign(s)
                t = src.field().one()
                t.sub_assign(s)
                r.mul_and_accumulate_into(t, other)
                r.sub_assign(result)
                dst.push_evaluation_result(r)


# Poseidon2 over Goldilocks as the reference parameterises it (poseidon2/params.rs:8-136): the 4x4
# block and the diagonal shifts, the matrices built from them, and the round constants of
# csrc/poseidon2_rc.inc (ROUND_CONSTANTS_ALIGNED_PER_ROUND: rounds 0..3 and 26..29 are the full
# rounds', element 0 of rounds 4..25 the partial rounds').
POSEIDON2_M4 = ((5, 7, 1, 3), (4, 6, 1, 1), (1, 3, 5, 7), (1, 1, 4, 6))
POSEIDON2_SHIFTS = (4, 14, 11, 8, 0, 5, 2, 9, 13, 6, 3, 12)
_POSEIDON2_RC = None


def poseidon2_external_matrix():
    """EXTERNAL_MDS_MATRIX (params.rs:63-94): block circulant, the diagonal blocks doubled."""
    return [[(2 if i // 4 == j // 4 else 1) * POSEIDON2_M4[i % 4][j % 4] for j in range(12)] for i in range(12)]


def poseidon2_inner_matrix():
    """INNER_ROUNDS_MATRIX (params.rs:96-105): ones, the diagonal 2^shift + 1."""
    return [[(1 << POSEIDON2_SHIFTS[i]) + 1 if i == j else 1 for j in range(12)] for i in range(12)]


def poseidon2_round_constants():
    """The 30 x 12 round constants, read once from the table the kernels are built from."""
    global _POSEIDON2_RC
    if _POSEIDON2_RC is None:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc", "poseidon2_rc.inc")
        with open(path) as f:
            values = [int(v) for v in re.findall(r"(\d+)ULL", f.read())]
        if len(values) != 360:
            raise ValueError("%s: expected 30 x 12 round constants" % path)
        _POSEIDON2_RC = [values[12 * r:12 * r + 12] for r in range(30)]
    return _POSEIDON2_RC


def _small_pow_7(x):
    """PrimeFieldLike::small_pow(7) (field_like.rs:92-101): x^2, x^4, x^6, x^7; a new value."""
    tmp = x.copy()
    tmp.square()
    pow2 = tmp.copy()
    tmp.square()
    tmp.mul_assign(pow2)
    tmp.mul_assign(x)
    return tmp


def _matrix_mul_naive(state, matrix, field):
    """dst_i = sum_j state_j * coeff_ij, from zero, by mul_and_accumulate_into (poseidon2.rs:247-255)."""
    out = []
    for row in matrix:
        tmp = field.zero()
        for src, coeff in zip(state, row):
            tmp.mul_and_accumulate_into(src, field.constant(coeff))
        out.append(tmp)
    return out


class Poseidon2FlattenedGate(Evaluator):
    """Poseidon2RoundFunctionFlattenedEvaluator<F, 8, 12, 4> over Goldilocks (poseidon2.rs:166-403):
    the permutation of variables 0..11 equals variables 12..23, every S-box layer "reset" by committed
    cells.  118 terms of degree 7 in push order: 3 x 12 resets of the first half, 22 of the partial
    rounds, 4 x 12 of the second half, 12 output terms.  S-box output cell s (0..105) reads witness
    column s while s < num_witness_columns_used and variable column 24 + s - num_witness_columns_used
    after that (:225-236).  The matrices are applied naively with constant coefficients, as the
    reference does, so the capture is its IR -- which passes every cap of a launch; the gate is a
    native kind and compile_gate_set does not capture it."""
    name = "poseidon2_flattened"
    native_kind = KIND_POSEIDON2
    num_quotient_terms = 118
    max_constraint_degree = 7
    STATE_WIDTH, HALF_NUM_FULL_ROUNDS, NUM_PARTIAL_ROUNDS = 12, 4, 22
    TOTAL_NUM_VARIABLES = 130   # total_num_variables (:430-437)

    def __init__(self, num_copiable_columns_used, num_witness_columns_used):
        self.num_copiable_columns_used = int(num_copiable_columns_used)
        self.num_witness_columns_used = int(num_witness_columns_used)
        if not 0 <= self.num_witness_columns_used <= self.TOTAL_NUM_VARIABLES - 2 * self.STATE_WIDTH:
            raise ValueError("at most 106 cells of the gate can be witness columns")
        if self.num_copiable_columns_used + self.num_witness_columns_used < self.TOTAL_NUM_VARIABLES:
            raise ValueError("the gate needs 130 cells (:231, :309, :361)")
        self.principal_width = (self.num_copiable_columns_used, self.num_witness_columns_used, 0)

    def num_repetitions_in_geometry(self, geometry):
        """The min of the copiable and the witness limit (:84-104)."""
        reps = geometry.num_columns_under_copy_permutation // self.num_copiable_columns_used
        if self.num_witness_columns_used:
            reps = min(reps, geometry.num_witness_columns // self.num_witness_columns_used)
        return reps

    def num_required_constants_in_geometry(self, geometry):
        return 0

    @classmethod
    def compute_strategy(cls, geometry):
        """Poseidon2FlattenedGate::compute_strategy (:502-528): (instances, (copiable, witness
        columns per instance))."""
        num_copiable, num_witnesses = geometry.num_columns_under_copy_permutation, geometry.num_witness_columns
        max_instances = min(num_copiable // (2 * cls.STATE_WIDTH),
                            (num_copiable + num_witnesses) // cls.TOTAL_NUM_VARIABLES)
        if max_instances <= 0:
            raise ValueError("can not allocate a gate, need at least %d copiable vars and %d vars + witnesses in total"
                             % (2 * cls.STATE_WIDTH, cls.TOTAL_NUM_VARIABLES))
        in_witness_per_copy = num_witnesses // max_instances
        return max_instances, (cls.TOTAL_NUM_VARIABLES - in_witness_per_copy, in_witness_per_copy)

    def evaluate_once(self, src, dst, shared):
        sw, half = self.STATE_WIDTH, self.HALF_NUM_FULL_ROUNDS
        field, rc = src.field(), poseidon2_round_constants()
        external, inner = poseidon2_external_matrix(), poseidon2_inner_matrix()
        full_round_constants = rc[:half] + rc[half + self.NUM_PARTIAL_ROUNDS:]
        partial_round_constants = [rc[half + r][0] for r in range(self.NUM_PARTIAL_ROUNDS)]
        state = [src.get_variable_value(i) for i in range(sw)]
        output = [src.get_variable_value(sw + i) for i in range(sw)]   # the output is placed early
        offsets = {"witness": 0, "copiable": 2 * sw}

        def sbox_out_var():   # witness columns first, then copiable ones (:225-236)
            if offsets["witness"] < self.num_witness_columns_used:
                offsets["witness"] += 1
                return src.get_witness_value(offsets["witness"] - 1)
            offsets["copiable"] += 1
            return src.get_variable_value(offsets["copiable"] - 1)

        def reset(state):
            cells = []
            for value in state:
                cell = sbox_out_var()
                contribution = value.copy()
                contribution.sub_assign(cell)
                dst.push_evaluation_result(contribution)
                cells.append(cell)
            return cells

        def full_round(state, round):
            for i in range(sw):
                state[i].add_assign(field.constant(full_round_constants[round][i]))
                state[i] = _small_pow_7(state[i])
            return _matrix_mul_naive(state, external, field)

        for round in range(half):
            state = reset(state) if round else _matrix_mul_naive(state, external, field)
            state = full_round(state, round)
        for round in range(self.NUM_PARTIAL_ROUNDS):
            state[0].add_assign(field.constant(partial_round_constants[round]))
            cell = sbox_out_var()
            contribution = state[0].copy()
            contribution.sub_assign(cell)
            dst.push_evaluation_result(contribution)
            state[0] = _small_pow_7(cell)
            state = _matrix_mul_naive(state, inner, field)
        for round in range(half):
            state = full_round(reset(state), half + round)
        for value, out in zip(state, output):
            contribution = out.copy()
            contribution.sub_assign(value)
            dst.push_evaluation_result(contribution)


def library():
    """The evaluators of the library in a fixed order: eight gates, ZeroCheck in both placements."""
    return [FmaGateInBaseFieldWithoutConstant(), BooleanConstraintGate(), ConstantsAllocatorGate(), ReductionGate(4),
            SelectionGate(), ZeroCheckGate(False), ZeroCheckGate(True), DotProductGate(4), ConditionalSwapGate(1)]
