// Quotient gate terms: an evaluator of captured relation programs over LDE columns that stay on
// the device (the loop prover.rs:560-1085 drives on the CPU).
//
// The circuit's evaluators stay the caller's.  What arrives here is what gpu_synthesizer/mod.rs
// captures from an evaluator's evaluate_once: a straight-line program of Relation::{Add, Double,
// Sub, Negate, Mul, Square} over Index::{VariablePoly, WitnessPoly, ConstantPoly, TemporaryValue,
// ConstantValue} and the list of pushed terms, with its placement (repetitions, PerChunkOffset,
// selector path, constants offset).  For every point L = coset * n + row of the first q cosets
//   acc(L) += sum_gates selector_g(L) sum_rep sum_term alpha[k] term(L),
// k running on across repetitions and gates: push_evaluation_result / proceed_to_next_gate /
// advance (buffering_source.rs:157-221, 303-377), evaluate_over_general_purpose_columns
// (cs/traits/evaluator.rs:376-397), compute_selector_subpath (prover.rs:2775-2916) and the
// specialized-columns form, which has no selector (prover.rs:651-801).
//
// Structure.  Three frames, one per launch (gate_terms_kernel, gate_check_kernel, gate_value_kernel),
// each instantiated per program kind, whose walk hands the terms of one repetition of one gate to a
// sink.  Placement, the selector product and the three sinks are written once for all of them.  One
// point per lane, 256 lanes per workgroup, one launch for all gates of a segment.
//
// Kind 0, the Interpreter.  The program is wave-uniform: every word of it is fetched through a
// uniform address of the uploaded image and forced into scalar registers (readfirstlane), so the
// decode (field extracts, the operand-kind and opcode branches, the column-address arithmetic) is
// scalar work and no lane takes a branch another does not.  A temporary lives in an LDS slot laid
// out [slot][lane], 8 bytes per lane, so a wave's access is 512 contiguous bytes: conflict free by
// construction, private to the lane, and no barrier is needed.  The host allocates slots by
// liveness (boojum_amd/gates.py), so GT_SLOTS bounds the values live at once, not the program's
// length.  The selector constants of a point (columns 0 .. depth - 1) are loaded once into
// registers and every gate multiplies its own path from them.
//
// Image (u64 words, built by the caller, checked by check_image below, uploaded once):
//   [0] GT_MAGIC  [1] number of segments S  [2 .. 2 + S) word offset of each segment
//   segment: [0] gates G  [1] instructions I  [2] writes W  [3] immediates M  [4] alpha base
//            [5] terms (sum over gates of repetitions * writes)  [6] selector columns read
//            [7] kind: 0 interpreted, 1 native Poseidon2 flattened gate (gates_poseidon2.hpp),
//            3 library gates (gates_library.hpp); 2 is no kind
//            G descriptors of 8 words, I instructions, W writes, M immediates
//   descriptor: [0] instr begin | end << 32   [1] write begin | end << 32
//               [2] repetitions | path length << 32   [3] path bit mask (bit i set: take column i,
//               clear: 1 - column i)   [4] variables base | per repetition << 32
//               [5] witnesses base | per repetition << 32   [6] constants base | per repetition << 32
//               [7] 0; in a native segment num_witness_columns_used
//   instruction: opcode | slot << 8 | a << 16 | b << 40;  operand (24 bits): kind << 21 | index
//   kinds: 0 VariablePoly, 1 WitnessPoly, 2 ConstantPoly, 3 slot, 4 immediate (index into M)
//   opcodes: Relation's order -- 0 Add, 1 Double, 2 Sub, 3 Negate, 4 Mul, 5 Square; 6 Inverse is
//   refused.  No evaluator in cs/gates records it: the three textual hits
//   (fma_gate_without_constant.rs:353, fma_gate_in_extension_without_constant.rs:451,
//   zero_check.rs:539) are all inside witness-resolution closures, not evaluate_once.
//
// A native segment holds one gate of a kind whose walk is written out (kind 1, p2g::Program, no LDS):
// G = 1, I = W = M = 0, the descriptor's [0] is 0 and its [1] is 0 | terms per repetition << 32 with
// no writes behind it, [2] .. [6] keep their meaning.
//
// A library segment (kind 3, lib::Program, no LDS) holds 1 .. GT_GATES gates the library has generated
// straight-line code for (tools/gen_gate_library.py -> gates_library.hpp, from the captures of
// boojum_amd.gates.library()): I = W = M = 0, a descriptor's [0] is the library id, its [1] is
// 0 | terms per repetition << 32, [2] .. [6] keep their meaning and [7] is 0.  The two entry points
// pick the frame's instantiation by the kind.
//
// One call launches one segment.  A gate set over the caps is split into segments by the caller,
// which is exact because the call adds to the accumulator and a segment carries its alpha base.
//
// The same image also answers where a witness fails its gates (check_if_satisfied,
// cs/implementations/satisfiability_test.rs:15-353): gate_check_kernel walks the same programs over
// trace rows and reports the count and the first failing (row, term) in a status record.
#include <hip/hip_runtime.h>
#include <cstring>
#include <new>
#include "ext2.hpp"
#include "gl.hpp"
#include "stage_host.hpp"

namespace bj {

namespace {

constexpr uint64_t GT_MAGIC = 0x3153455441474A42ULL;  // "BJGATES1"
constexpr uint32_t GT_THREADS = 256;
constexpr uint32_t GT_SLOTS = BJ_GATE_MAX_SLOTS;        // 16 slots of 2 KB: 32 KB, five workgroups per CU
constexpr uint32_t GT_SEL = BJ_GATE_MAX_SELECTOR_DEPTH;
constexpr uint32_t GT_INSTRS = BJ_GATE_MAX_INSTRUCTIONS;
constexpr uint32_t GT_GATES = BJ_GATE_MAX_GATES;
constexpr uint32_t GT_HDR = 8, GT_DESC = 8;
constexpr uint32_t K_VAR = 0, K_WIT = 1, K_CONST = 2, K_SLOT = 3, K_IMM = 4;
constexpr uint32_t OP_ADD = 0, OP_DOUBLE = 1, OP_SUB = 2, OP_NEGATE = 3, OP_MUL = 4, OP_SQUARE = 5;
static_assert(OP_ADD == 0 && OP_SUB == 2 && OP_MUL == 4, "Relation's order (gpu_synthesizer/mod.rs:125-133)");
constexpr uint32_t IDX_BITS = 21, IDX_MASK = (1u << IDX_BITS) - 1;

struct Cols {
    const uint64_t* p[3];  // variables, witnesses, constants: coset 0 of column 0
    size_t stride[3];
};

// a uniform word of the image, in scalar registers
__device__ __forceinline__ uint64_t uword(const uint64_t* __restrict__ p) {
    const uint64_t v = *p;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

// Where a gate sits: words [2] .. [7] of its descriptor, decoded once into scalar registers.
struct Placement {
    uint32_t reps, depth, base[3], per[3], word7;
    uint64_t mask;

    __device__ __forceinline__ explicit Placement(const uint64_t* __restrict__ d) {
        const uint64_t d2 = uword(d + 2);
        reps = (uint32_t)d2, depth = (uint32_t)(d2 >> 32), mask = uword(d + 3);
#pragma unroll
        for (uint32_t k = 0; k < 3; k++) {
            const uint64_t w = uword(d + 4 + k);
            base[k] = (uint32_t)w, per[k] = (uint32_t)(w >> 32);
        }
        word7 = (uint32_t)uword(d + 7);
    }
};

// The path product over constant columns 0 .. depth - 1: column i, or 1 - column i where the mask's
// bit i is clear; 1 for an empty path.  The program kind gives the column values and says how far to unroll.
template <class Program>
__device__ __forceinline__ uint64_t selector(const Placement& pl, const Program& prog) {
    uint64_t sel = 1;
#pragma unroll Program::SELECTOR_UNROLL
    for (uint32_t i = 0; i < GT_SEL && i < pl.depth; i++) {
        const uint64_t c = prog.selector_column(i);
        const uint64_t f = (pl.mask >> i) & 1 ? c : gl::sub(1, c);
        sel = i == 0 ? f : gl::mul(sel, f);
    }
    return sel;
}

// ------------------------------------------------------------------ what happens to a term
// A walk hands every term to sink.emit(v) in push order; the frame around it sets what changes per gate
// and stops walking once the sink is done().

// g += alpha[k] term, two base products, k running on from the segment's alpha base
struct AccumulatorSink {
    const uint64_t* __restrict__ alpha;
    uint64_t g0, g1;
    __device__ __forceinline__ void emit(uint64_t v) {
        g0 = gl::add(g0, gl::mul(v, uword(alpha)));
        g1 = gl::add(g1, gl::mul(v, uword(alpha + 1)));
        alpha += 2;
    }
    __device__ __forceinline__ bool done() const { return false; }
};

// the lane's failing terms (selector * term != 0): their number and the first k, the smallest as k only grows
struct CheckSink {
    uint64_t sel, count;
    uint32_t k, first;
    bool selected, in;
    __device__ __forceinline__ void emit(uint64_t v) {
        const bool fail = in && gl::canon(selected ? gl::mul(v, sel) : v) != 0;
        first = fail && count == 0 ? k : first;
        count += fail;
        k++;
    }
    __device__ __forceinline__ bool done() const { return false; }
};

// the canonical value of term `target` to the record (wave-uniform: every lane walks the same row)
struct ValueSink {
    unsigned long long* __restrict__ status;
    uint32_t k, target;
    __device__ __forceinline__ void emit(uint64_t v) {
        if (k == target && threadIdx.x == 0) status[2] = gl::canon(v);
        k++;
    }
    __device__ __forceinline__ bool done() const { return k > target; }
};

// ------------------------------------------------------------------ the program kinds
// A kind says how many LDS slots a lane needs (SLOTS) and is made per lane for (segment, columns,
// point L, the lane's slots).  It gives the frames gate(d) at each descriptor, walk(placement, off,
// sink) for one repetition of that gate at L and the repetition's three column offsets, and the point's
// selector columns (read_selector_columns() once where a frame forms selectors, then selector_column(i)).
#include "gates_poseidon2.hpp"
#include "gates_library.hpp"

// Kind 0: the relation programs of the image, temporaries in this lane's column of the LDS slots.
struct Interpreter {
    static constexpr uint32_t SELECTOR_UNROLL = GT_SEL;  // the columns are registers: static indices
    static constexpr uint32_t GATES = 0;                 // as many as the segment says
    static constexpr uint32_t SLOTS = GT_SLOTS;
    const Cols& cols;
    const size_t L;
    uint64_t* slots;
    const uint64_t* __restrict__ instr;
    const uint64_t* __restrict__ writes;
    const uint64_t* __restrict__ imm;
    uint32_t i0, i1, w0, w1;  // the current gate's instruction and write ranges
    uint32_t sel_cols;        // selector columns the segment reads
    uint64_t selc[GT_SEL];    // their values at the point, loaded once for all gates

    __device__ __forceinline__ Interpreter(const uint64_t* __restrict__ seg, const Cols& cols, size_t L, uint64_t* slots)
        : cols(cols), L(L), slots(slots) {
        instr = seg + GT_HDR + (size_t)(uint32_t)uword(seg + 0) * GT_DESC;
        writes = instr + (uint32_t)uword(seg + 1);
        imm = writes + (uint32_t)uword(seg + 2);
        sel_cols = (uint32_t)uword(seg + 6);
    }
    __device__ __forceinline__ void read_selector_columns() {
#pragma unroll
        for (uint32_t i = 0; i < GT_SEL; i++) selc[i] = i < sel_cols ? cols.p[2][(size_t)i * cols.stride[2] + L] : 0;
    }
    __device__ __forceinline__ void gate(const uint64_t* __restrict__ d) {
        const uint64_t d0 = uword(d), d1 = uword(d + 1);
        i0 = (uint32_t)d0, i1 = (uint32_t)(d0 >> 32), w0 = (uint32_t)d1, w1 = (uint32_t)(d1 >> 32);
    }
    __device__ __forceinline__ uint64_t selector_column(uint32_t i) const { return selc[i]; }

    __device__ __forceinline__ uint64_t fetch(uint32_t operand, const uint32_t (&off)[3]) const {
        const uint32_t kind = operand >> IDX_BITS, idx = operand & IDX_MASK;
        if (kind == K_SLOT) return slots[idx * GT_THREADS];
        if (kind == K_IMM) return uword(imm + idx);
        if (kind == K_VAR) return cols.p[0][(size_t)(idx + off[0]) * cols.stride[0] + L];
        if (kind == K_WIT) return cols.p[1][(size_t)(idx + off[1]) * cols.stride[1] + L];
        return cols.p[2][(size_t)(idx + off[2]) * cols.stride[2] + L];
    }
    template <class Sink>
    __device__ __forceinline__ void walk(const Placement&, const uint32_t (&off)[3], Sink& sink) const {
        for (uint32_t pc = i0; pc < i1; pc++) {
            const uint64_t w = uword(instr + pc);
            const uint32_t op = (uint32_t)w & 0xff, slot = (uint32_t)(w >> 8) & 0xff;
            const uint64_t a = fetch((uint32_t)(w >> 16) & 0xffffff, off);
            uint64_t r;
            if (op == OP_DOUBLE) {
                r = gl::add(a, a);
            } else if (op == OP_NEGATE) {
                r = gl::sub(0, a);
            } else if (op == OP_SQUARE) {
                r = gl::mul(a, a);
            } else {
                const uint64_t b = fetch((uint32_t)(w >> 40) & 0xffffff, off);
                r = op == OP_MUL ? gl::mul(a, b) : op == OP_ADD ? gl::add(a, b) : gl::sub(a, b);
            }
            slots[slot * GT_THREADS] = r;
        }
        for (uint32_t t = w0; t < w1; t++) sink.emit(fetch((uint32_t)uword(writes + t) & 0xffffff, off));
    }
};

// ------------------------------------------------------------------ the frames
// A frame owns the LDS slots, the lane's point and its guard, the gate loop, what the sink needs per
// gate, and what leaves the kernel.

// This lane's column of the [slot][lane] LDS slots, if the kind asks for any.
template <class Program>
__device__ __forceinline__ uint64_t* lane_slots() {
    if constexpr (Program::SLOTS != 0) {
        __shared__ uint64_t lds[Program::SLOTS * GT_THREADS];
        return lds + threadIdx.x;
    }
    return nullptr;
}

// The repetitions of one gate, the column offsets running on by the placement's per-repetition steps.
template <class Program, class Sink>
__device__ __forceinline__ void repetitions(const Program& prog, const Placement& pl, Sink& sink) {
    uint32_t off[3] = {pl.base[0], pl.base[1], pl.base[2]};
    for (uint32_t rep = 0; rep < pl.reps && !sink.done(); rep++) {
        prog.walk(pl, off, sink);
#pragma unroll
        for (uint32_t k = 0; k < 3; k++) off[k] += pl.per[k];
    }
}

// The gates of a segment: word [0], or what the kind fixes (the validator holds a native segment to it).
template <class Program>
__device__ __forceinline__ uint32_t gates_of(const uint64_t* __restrict__ seg) {
    return Program::GATES ? Program::GATES : (uint32_t)uword(seg + 0);
}

// Lane l of a launch over `count` points from `first`.  A lane past the end walks the first point, so
// its loads stay in bounds, and (`in` false) writes and counts nothing.
__device__ __forceinline__ size_t lane_point(uint64_t first, uint64_t count, bool& in) {
    const size_t l = blockIdx.x * (size_t)GT_THREADS + threadIdx.x;
    in = l < count;
    return (size_t)first + (in ? l : 0);
}

// bj_quotient_gate_terms_d: acc(L) += sum_gates selector_g(L) sum_rep sum_term alpha[k] term(L); the
// selector multiplies a gate's sum once, the accumulator is read once and written once.
template <class Program>
__global__ __launch_bounds__(GT_THREADS) void gate_terms_kernel(const uint64_t* __restrict__ seg, Cols cols,
                                                                const uint64_t* __restrict__ alphas, size_t total,
                                                                uint64_t* __restrict__ dst0,
                                                                uint64_t* __restrict__ dst1) {
    bool in;
    const size_t L = lane_point(0, total, in);
    Program prog(seg, cols, L, lane_slots<Program>());
    prog.read_selector_columns();
    AccumulatorSink sink{alphas + 2 * uword(seg + 4), 0, 0};
    uint64_t acc0 = 0, acc1 = 0;
    const uint32_t n_gates = gates_of<Program>(seg);
    for (uint32_t g = 0; g < n_gates; g++) {
        const uint64_t* __restrict__ d = seg + GT_HDR + (size_t)g * GT_DESC;
        const Placement pl(d);
        prog.gate(d);
        sink.g0 = sink.g1 = 0;
        repetitions(prog, pl, sink);
        if (pl.depth) {
            const uint64_t sel = selector(pl, prog);
            sink.g0 = gl::mul(sink.g0, sel);
            sink.g1 = gl::mul(sink.g1, sel);
        }
        acc0 = gl::add(acc0, sink.g0);
        acc1 = gl::add(acc1, sink.g1);
    }
    if (in) {
        dst0[L] = gl::canon(gl::add(acc0, dst0[L]));
        dst1[L] = gl::canon(gl::add(acc1, dst1[L]));
    }
}

// ------------------------------------------------------------------ satisfiability check
// The same walk over trace columns (no LDE, no challenges, no accumulator): term k of row r fails
// iff selector_g(r) * term_k(r) != 0, k being the running term index the alphas use (the segment's
// alpha base carries it on).  One row of the window per lane.  A lane keeps its number of failures
// and the first failing k (CheckSink); a wave reduces both with shuffles and, only if it saw a
// failure, issues one 64-bit add and one 64-bit min on the status record: [0] += count,
// [1] = min(row << 32 | k).
//
// gate_value_kernel is the second, one-wave launch of the call: every lane walks the row of the
// record's key and lane 0 writes the canonical value of term k to [2] -- only when k lies in this
// segment and the row in this window, so the value follows the key across the calls of a set.
constexpr uint64_t GC_NONE = ~0ULL;
constexpr uint32_t GC_WAVE = 64;

__global__ void gate_check_begin_kernel(unsigned long long* __restrict__ status) {
    if (threadIdx.x < 4) status[threadIdx.x] = threadIdx.x == 1 ? GC_NONE : 0;
}

// A lane's failures (their number and the first k, on row L) into the record: one add and one min
// per wave that saw a failure.
__device__ __forceinline__ void check_combine(uint64_t count, uint32_t first, size_t L,
                                              unsigned long long* __restrict__ status) {
    unsigned long long key = count ? ((unsigned long long)L << 32) | first : GC_NONE;
    unsigned long long sum = count;
#pragma unroll
    for (uint32_t o = GC_WAVE / 2; o; o >>= 1) {
        sum += __shfl_down(sum, o, GC_WAVE);
        const unsigned long long other = __shfl_down(key, o, GC_WAVE);
        key = other < key ? other : key;
    }
    if ((threadIdx.x & (GC_WAVE - 1)) == 0 && sum) {
        atomicAdd(&status[0], sum);
        atomicMin(&status[1], key);
    }
}

template <class Program>
__global__ __launch_bounds__(GT_THREADS) void gate_check_kernel(const uint64_t* __restrict__ seg, Cols cols,
                                                                uint64_t row_begin, uint64_t n_rows,
                                                                unsigned long long* __restrict__ status) {
    bool in;
    const size_t L = lane_point(row_begin, n_rows, in);
    Program prog(seg, cols, L, lane_slots<Program>());
    prog.read_selector_columns();
    CheckSink sink{1, 0, (uint32_t)uword(seg + 4), 0, false, in};
    const uint32_t n_gates = gates_of<Program>(seg);
    for (uint32_t g = 0; g < n_gates; g++) {
        const uint64_t* __restrict__ d = seg + GT_HDR + (size_t)g * GT_DESC;
        const Placement pl(d);
        prog.gate(d);
        sink.selected = pl.depth != 0;  // the gate's selector is formed before its repetitions
        sink.sel = selector(pl, prog);
        repetitions(prog, pl, sink);
    }
    check_combine(sink.count, sink.first, L, status);
}

template <class Program>
__global__ __launch_bounds__(GT_THREADS) void gate_value_kernel(const uint64_t* __restrict__ seg, Cols cols,
                                                                uint64_t row_begin, uint64_t n_rows,
                                                                unsigned long long* __restrict__ status) {
    const uint32_t k = (uint32_t)uword(seg + 4);
    const uint64_t key = uword(reinterpret_cast<const uint64_t*>(status) + 1);
    const uint64_t row = key >> 32;
    const uint32_t target = (uint32_t)key;
    if (key == GC_NONE || target < k || target - k >= uword(seg + 5)) return;
    if (row < row_begin || row - row_begin >= n_rows) return;
    Program prog(seg, cols, (size_t)row, lane_slots<Program>());  // no selector is formed: its columns stay unread
    ValueSink sink{status, k, target};
    const uint32_t n_gates = gates_of<Program>(seg);
    for (uint32_t g = 0; g < n_gates && !sink.done(); g++) {  // the walk ends with the repetition of the target
        const uint64_t* __restrict__ d = seg + GT_HDR + (size_t)g * GT_DESC;
        const Placement pl(d);
        prog.gate(d);
        repetitions(prog, pl, sink);
    }
}

// ------------------------------------------------------------------ host side: the image's checks
struct Need {
    uint64_t cols[3];  // columns the largest repetition reaches, per kind
    uint64_t alphas;   // challenges the whole image consumes
    uint64_t segments;
};

struct GateSet {
    uint64_t magic;
    uint64_t* image_d;
    Need need;
    uint64_t n_segments;
    uint64_t seg_offset[BJ_GATE_MAX_SEGMENTS];
    uint64_t seg_kind[BJ_GATE_MAX_SEGMENTS];
};

int bad(const char* why) {
    char msg[256];
    snprintf(msg, sizeof msg, "gate program: %s", why);
    return set_error(BJ_EINVAL, msg);
}

// An operand's claim on its space; false when it is outside.  written: the slots written so far.
bool operand_ok(uint32_t operand, uint64_t n_imm, uint32_t written, const uint64_t (&last)[3], Need& need) {
    const uint32_t kind = operand >> IDX_BITS, idx = operand & IDX_MASK;
    if (kind == K_SLOT) return idx < GT_SLOTS && ((written >> idx) & 1);
    if (kind == K_IMM) return idx < n_imm;
    if (kind > K_IMM) return false;
    const uint64_t reach = last[kind] + idx + 1;  // columns needed at the largest repetition
    if (reach > ((uint64_t)1 << 31)) return false;
    if (reach > need.cols[kind]) need.cols[kind] = reach;
    return true;
}

// A descriptor's placement, the same words for both kinds of gate, checked in two steps because a
// native gate's own checks fire between them.  First [2] and [3]: the repetitions and the selector
// path with its mask.
int check_path(const uint64_t* d, uint64_t& reps, uint64_t& depth) {
    reps = d[2] & 0xffffffff, depth = d[2] >> 32;
    if (reps == 0 || reps > (1u << 20)) return bad("num_repetitions outside 1..2^20");
    if (depth > GT_SEL || (d[3] >> depth)) return bad("malformed selector path");
    return BJ_OK;
}

// Then [4] .. [6]: the three base | per << 32 column offsets.  width: the columns one repetition must
// hold, per kind (a native gate's cells; nothing for a program, whose operands are checked one by one).
// last: the offset at the largest repetition, at most 2^20 + 2^10 (2^20 - 1), well inside 2^31.
int check_offsets(const uint64_t* d, uint64_t reps, const uint64_t (&width)[3], uint64_t (&last)[3]) {
    for (int k = 0; k < 3; k++) {
        const uint64_t b = d[4 + k] & 0xffffffff, per = d[4 + k] >> 32;
        if (b > (1u << 20) || per > (1u << 10)) return bad("a column offset is out of range");
        if (per < width[k]) return bad("a repetition of the native gate is narrower than its cells");
        last[k] = b + per * (reps - 1);
    }
    return BJ_OK;
}

// A native segment (kind != 0): one gate, no program, the kind's own term count and cell split.
int check_native(const uint64_t* seg, Need& need) {
    const uint64_t G = seg[0], I = seg[1], W = seg[2], M = seg[3], terms = seg[5], sel = seg[6], kind = seg[7];
    if (kind != p2g::KIND) return bad("unknown native segment kind");
    if (G != 1) return bad("a native segment holds exactly one gate");
    if (I || W || M) return bad("a native segment carries no instructions, writes or immediates");
    const uint64_t* d = seg + GT_HDR;
    const uint64_t nw = d[7];
    uint64_t reps, depth, last[3];
    if (d[0] != 0 || d[1] != (uint64_t)p2g::TERMS << 32) return bad("a native gate's instruction or write range is malformed");
    if (const int rc = check_path(d, reps, depth)) return rc;
    if (terms != p2g::TERMS * reps) return bad("a native segment's term count is not 118 per repetition");
    if (sel != depth) return bad("a segment's selector columns are not its deepest path");
    if (nw > p2g::MAX_WITNESS_CELLS) return bad("num_witness_columns_used exceeds the gate's 106 S-box output cells");
    const uint64_t width[3] = {p2g::CELLS - nw, nw, 0};
    if (const int rc = check_offsets(d, reps, width, last)) return rc;
    for (int k = 0; k < 2; k++)  // columns needed at the largest repetition
        if (width[k] && last[k] + width[k] > need.cols[k]) need.cols[k] = last[k] + width[k];
    return BJ_OK;
}

// A library segment (kind 3): every gate's placement first, as for the other kinds, then what is the
// kind's own -- no program area, a known id with its term count, word [7] clear, the sums of the head.
// need: what the largest repetition reaches, as the operands of the interpreted program would claim it.
namespace refusal {  // the kind's own refusals by name; tests/test_gate_library_cpu.py holds an image for each
constexpr const char* PROGRAM_AREA = "a library segment carries no instructions, writes or immediates";
constexpr const char* UNKNOWN_ID = "unknown library gate id";
constexpr const char* GATE_TERMS = "a library gate's term count is not its entry's";
constexpr const char* WORD7 = "word [7] of a library gate is not 0";
}  // namespace refusal

int check_library(const uint64_t* seg, Need& need) {
    const uint64_t G = seg[0], I = seg[1], W = seg[2], M = seg[3], terms = seg[5], sel = seg[6];
    const uint64_t* desc = seg + GT_HDR;
    uint64_t count = 0, deepest = 0;
    uint64_t reps[GT_GATES], last[GT_GATES][3];  // G <= GT_GATES: check_image
    for (uint64_t g = 0; g < G; g++) {
        uint64_t depth;
        if (const int rc = check_path(desc + g * GT_DESC, reps[g], depth)) return rc;
        if (const int rc = check_offsets(desc + g * GT_DESC, reps[g], {0, 0, 0}, last[g])) return rc;
        if (depth > deepest) deepest = depth;
    }
    if (I || W || M) return bad(refusal::PROGRAM_AREA);
    for (uint64_t g = 0; g < G; g++) {
        const uint64_t* d = desc + g * GT_DESC;
        if (d[0] == 0 || d[0] > lib::ENTRIES) return bad(refusal::UNKNOWN_ID);
        const lib::Entry& e = lib::TABLE[d[0] - 1];
        if (d[1] != (uint64_t)e.terms << 32) return bad(refusal::GATE_TERMS);
        if (d[7] != 0) return bad(refusal::WORD7);
        for (int k = 0; k < 3; k++)  // columns needed at the largest repetition
            if (e.columns[k] && last[g][k] + e.columns[k] > need.cols[k]) need.cols[k] = last[g][k] + e.columns[k];
        count += reps[g] * e.terms;
    }
    if (count != terms) return bad("a segment's term count is not the sum over its gates");
    if (sel != deepest) return bad("a segment's selector columns are not its deepest path");
    return BJ_OK;
}

// An interpreted segment: every gate's ranges and placement, every instruction and write.
int check_interpreted(const uint64_t* seg, Need& need) {
    const uint64_t G = seg[0], I = seg[1], W = seg[2], M = seg[3], terms = seg[5], sel = seg[6];
    const uint64_t* desc = seg + GT_HDR;
    const uint64_t* instr = desc + G * GT_DESC;
    const uint64_t* writes = instr + I;
    uint64_t count = 0, deepest = 0;
    for (uint64_t g = 0; g < G; g++) {
        const uint64_t* d = desc + g * GT_DESC;
        const uint64_t i0 = d[0] & 0xffffffff, i1 = d[0] >> 32, w0 = d[1] & 0xffffffff, w1 = d[1] >> 32;
        uint64_t reps, depth, last[3];
        if (i0 > i1 || i1 > I || w0 >= w1 || w1 > W) return bad("a gate's instruction or write range is malformed or has no terms");
        if (const int rc = check_path(d, reps, depth)) return rc;
        if (d[7] != 0) return bad("malformed selector path");
        if (depth > deepest) deepest = depth;
        if (const int rc = check_offsets(d, reps, {0, 0, 0}, last)) return rc;
        uint32_t written = 0;
        for (uint64_t pc = i0; pc < i1; pc++) {
            const uint64_t w = instr[pc];
            const uint32_t op = (uint32_t)(w & 0xff), slot = (uint32_t)((w >> 8) & 0xff);
            if (op == 6) return bad("Relation::Inverse is not evaluated (no evaluator in cs/gates records it)");
            if (op > 6) return bad("unknown opcode");
            if (slot >= GT_SLOTS) return bad("more temporaries live at once than BJ_GATE_MAX_SLOTS");
            const bool unary = op == OP_DOUBLE || op == OP_NEGATE || op == OP_SQUARE;
            if (!operand_ok((uint32_t)((w >> 16) & 0xffffff), M, written, last, need) ||
                (!unary && !operand_ok((uint32_t)((w >> 40) & 0xffffff), M, written, last, need)))
                return bad("an operand is outside its space, or a temporary is read before it is written");
            if (unary && (w >> 40)) return bad("a unary relation carries a second operand");
            written |= 1u << slot;
        }
        for (uint64_t t = w0; t < w1; t++) {
            if (writes[t] >> 24 || !operand_ok((uint32_t)writes[t], M, written, last, need))
                return bad("a written operand is outside its space, or a temporary that was never written");
        }
        count += reps * (w1 - w0);
    }
    if (count != terms) return bad("a segment's term count is not the sum over its gates");
    if (sel != deepest) return bad("a segment's selector columns are not its deepest path");
    return BJ_OK;
}

int check_image(const uint64_t* image, size_t words, Need& need, uint64_t* seg_offset, uint64_t* seg_kind) {
    need = Need{{0, 0, 0}, 0, 0};
    if (!image) return bad("null image");
    if (words < 2 || image[0] != GT_MAGIC) return bad("not a gate-set image");
    const uint64_t n_seg = image[1];
    if (n_seg == 0 || n_seg > BJ_GATE_MAX_SEGMENTS) return bad("segment count outside 1..BJ_GATE_MAX_SEGMENTS");
    if (words < 2 + n_seg) return bad("truncated segment table");
    need.segments = n_seg;
    for (uint64_t s = 0; s < n_seg; s++) {
        const uint64_t at = image[2 + s];
        if (at < 2 + n_seg || at > words || words - at < GT_HDR) return bad("segment offset outside the image");
        const uint64_t* seg = image + at;
        const uint64_t G = seg[0], I = seg[1], W = seg[2], M = seg[3], base = seg[4], terms = seg[5], sel = seg[6];
        if (G == 0 || G > GT_GATES) return bad("gates of a segment outside 1..BJ_GATE_MAX_GATES");
        if (I > GT_INSTRS) return bad("a segment exceeds BJ_GATE_MAX_INSTRUCTIONS");
        if (W > GT_INSTRS || M > GT_INSTRS) return bad("a segment's writes or immediates exceed BJ_GATE_MAX_INSTRUCTIONS");
        if (words - at < GT_HDR + G * GT_DESC + I + W + M) return bad("truncated segment");
        if (sel > GT_SEL) return bad("selector depth exceeds BJ_GATE_MAX_SELECTOR_DEPTH");
        if (base != need.alphas) return bad("a segment's alpha base is not the sum of the terms before it");
        if (seg_kind) seg_kind[s] = seg[7];
        const int rc = seg[7] == lib::KIND ? check_library(seg, need)
                       : seg[7]           ? check_native(seg, need)
                                          : check_interpreted(seg, need);
        if (rc) return rc;
        if (sel > need.cols[K_CONST]) need.cols[K_CONST] = sel;
        need.alphas += terms;
        if (seg_offset) seg_offset[s] = at;
    }
    return BJ_OK;
}

// The three column kinds of a call as the kernels take them.  A kind the set names must be there,
// wide enough and with a stride of at least `extent` (`below` in the entry point's message); a kind
// no operand names is never read and points at `unused`, so no lane forms a null address.
int bind_columns(const Need& need, const uint64_t* const (&p)[3], const size_t (&stride)[3], const uint32_t (&have)[3],
                 uint64_t extent, const uint64_t* unused, const char* entry, const char* below, Cols& cols) {
    static const char* const name[3] = {"variables", "witnesses", "constants"};
    for (int k = 0; k < 3; k++) {
        char msg[160];
        if (need.cols[k] > have[k]) {
            snprintf(msg, sizeof msg, "gate program: an operand reaches %s column %llu of %u", name[k],
                     (unsigned long long)(need.cols[k] - 1), have[k]);
            return set_error(BJ_EINVAL, msg);
        }
        if (need.cols[k] && (!p[k] || stride[k] < extent)) {
            snprintf(msg, sizeof msg, "%s: %s are null or their stride is below %s", entry, name[k], below);
            return set_error(BJ_EINVAL, msg);
        }
        cols.p[k] = need.cols[k] ? p[k] : unused;
        cols.stride[k] = need.cols[k] ? stride[k] : 0;
    }
    return BJ_OK;
}

}  // namespace

}  // namespace bj

extern "C" {

int bj_gate_set_check_h(const uint64_t* image, size_t words, uint64_t* need) {
    bj::Need n;
    if (const int rc = bj::check_image(image, words, n, nullptr, nullptr)) return rc;
    if (need) {
        need[0] = n.cols[0], need[1] = n.cols[1], need[2] = n.cols[2];
        need[3] = n.alphas, need[4] = n.segments;
    }
    return BJ_OK;
}

int bj_gate_native_info_h(uint32_t kind, uint64_t* out) {
    if (kind != bj::p2g::KIND) return bj::set_error(BJ_EINVAL, "bj_gate_native_info_h: unknown native gate kind");
    if (!out) return bj::set_error(BJ_EINVAL, "bj_gate_native_info_h: null out");
    out[0] = bj::p2g::CELLS, out[1] = bj::p2g::TERMS, out[2] = bj::p2g::DEGREE, out[3] = bj::p2g::MAX_WITNESS_CELLS;
    return BJ_OK;
}

int bj_gate_library_find_h(const char* name, uint64_t* out) {
    if (!name) return bj::set_error(BJ_EINVAL, "bj_gate_library_find_h: null name");
    if (!out) return bj::set_error(BJ_EINVAL, "bj_gate_library_find_h: null out");
    for (const bj::lib::Entry& e : bj::lib::TABLE) {
        if (strcmp(name, e.name) != 0) continue;
        out[0] = e.id, out[1] = e.terms, out[2] = e.columns[0], out[3] = e.columns[1], out[4] = e.columns[2];
        out[5] = e.digest;
        return BJ_OK;
    }
    return bj::set_error(BJ_EINVAL, "bj_gate_library_find_h: no library gate of that name");
}

int bj_gate_set_upload_d(const uint64_t* image, size_t words, void** set) {
    if (!set) return bj::set_error(BJ_EINVAL, "bj_gate_set_upload_d: null set");
    *set = nullptr;
    bj::GateSet* s = new (std::nothrow) bj::GateSet;
    if (!s) return bj::set_error(BJ_EINVAL, "bj_gate_set_upload_d: out of host memory");
    if (const int rc = bj::check_image(image, words, s->need, s->seg_offset, s->seg_kind)) {
        delete s;
        return rc;
    }
    s->magic = bj::GT_MAGIC;
    s->n_segments = s->need.segments;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&s->image_d), words * sizeof(uint64_t));
    if (e == hipSuccess) {
        e = hipMemcpy(s->image_d, image, words * sizeof(uint64_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) (void)hipFree(s->image_d);
    }
    if (e != hipSuccess) {
        delete s;
        return bj::hip_fail(e, "gate set upload");
    }
    *set = s;
    return BJ_OK;
}

int bj_gate_set_release(void* set) {
    bj::GateSet* s = static_cast<bj::GateSet*>(set);
    if (!s) return BJ_OK;
    if (s->magic != bj::GT_MAGIC) return bj::set_error(BJ_EINVAL, "bj_gate_set_release: not a gate set");
    s->magic = 0;
    const hipError_t e = hipFree(s->image_d);
    delete s;
    return bj::ok_or(e, "gate set release");
}

int bj_quotient_gate_terms_d(const void* set, uint32_t segment, const uint64_t* vars, size_t vars_stride,
                             uint32_t n_vars, const uint64_t* wits, size_t wits_stride, uint32_t n_wits,
                             const uint64_t* consts, size_t consts_stride, uint32_t n_consts, const uint64_t* alphas,
                             uint32_t n_alphas, uint32_t log_n, uint32_t log_q, uint64_t* dst0, uint64_t* dst1,
                             void* stream) {
    const bj::GateSet* s = static_cast<const bj::GateSet*>(set);
    if (!s || s->magic != bj::GT_MAGIC) return bj::set_error(BJ_EINVAL, "bj_quotient_gate_terms_d: not a gate set");
    if (const char* why = bj::bad_domain(log_n, log_q)) return bj::set_error(BJ_EINVAL, why);
    if (segment >= s->n_segments) return bj::set_error(BJ_EINVAL, "bj_quotient_gate_terms_d: no such segment");
    if (!alphas || !dst0 || !dst1) return bj::set_error(BJ_EINVAL, "bj_quotient_gate_terms_d: null pointer");
    const size_t total = (size_t)1 << (log_n + log_q);
    bj::Cols cols;  // an unused kind points at the accumulator
    if (const int rc = bj::bind_columns(s->need, {vars, wits, consts}, {vars_stride, wits_stride, consts_stride},
                                        {n_vars, n_wits, n_consts}, total, dst0, "bj_quotient_gate_terms_d",
                                        "2^(log_n + log_q)", cols))
        return rc;
    if (s->need.alphas > n_alphas) return bj::set_error(BJ_EINVAL, "gate program: fewer challenges than terms");
    const size_t blocks = (total + bj::GT_THREADS - 1) / bj::GT_THREADS;
    const uint64_t kind = s->seg_kind[segment];
    hipLaunchKernelGGL(kind == bj::lib::KIND   ? bj::gate_terms_kernel<bj::lib::Program>
                       : kind == bj::p2g::KIND ? bj::gate_terms_kernel<bj::p2g::Program>
                                               : bj::gate_terms_kernel<bj::Interpreter>,
                       dim3((unsigned)blocks), dim3(bj::GT_THREADS), 0, bj::S(stream),
                       s->image_d + s->seg_offset[segment], cols, alphas, total, dst0, dst1);
    return bj::ok_or(hipGetLastError(), "quotient gate terms");
}

int bj_gate_set_satisfied_d(const void* set, uint32_t segment, const uint64_t* vars, size_t vars_stride,
                            uint32_t n_vars, const uint64_t* wits, size_t wits_stride, uint32_t n_wits,
                            const uint64_t* consts, size_t consts_stride, uint32_t n_consts, uint64_t row_begin,
                            uint64_t n_rows, uint64_t* status_d, void* stream) {
    const bj::GateSet* s = static_cast<const bj::GateSet*>(set);
    if (!s || s->magic != bj::GT_MAGIC) return bj::set_error(BJ_EINVAL, "bj_gate_set_satisfied_d: not a gate set");
    const bool begin = segment & BJ_GATE_CHECK_BEGIN;
    segment &= ~BJ_GATE_CHECK_BEGIN;
    if (segment >= s->n_segments) return bj::set_error(BJ_EINVAL, "bj_gate_set_satisfied_d: no such segment");
    if (!status_d) return bj::set_error(BJ_EINVAL, "bj_gate_set_satisfied_d: null status");
    const uint64_t rows_cap = (uint64_t)1 << 32;
    if (n_rows == 0 || row_begin > rows_cap || n_rows > rows_cap - row_begin)
        return bj::set_error(BJ_EINVAL, "bj_gate_set_satisfied_d: the row window is empty or ends past 2^32");
    if (s->need.alphas >= rows_cap)  // the key holds k in 32 bits, all ones being "none"
        return bj::set_error(BJ_EINVAL, "bj_gate_set_satisfied_d: the set has 2^32 terms or more");
    bj::Cols cols;  // an unused kind points at the record
    if (const int rc = bj::bind_columns(s->need, {vars, wits, consts}, {vars_stride, wits_stride, consts_stride},
                                        {n_vars, n_wits, n_consts}, row_begin + n_rows, status_d,
                                        "bj_gate_set_satisfied_d", "row_begin + n_rows", cols))
        return rc;
    hipStream_t st = bj::S(stream);
    unsigned long long* status = reinterpret_cast<unsigned long long*>(status_d);
    const uint64_t* seg = s->image_d + s->seg_offset[segment];
    if (begin) hipLaunchKernelGGL(bj::gate_check_begin_kernel, dim3(1), dim3(bj::GC_WAVE), 0, st, status);
    const size_t blocks = (size_t)((n_rows + bj::GT_THREADS - 1) / bj::GT_THREADS);
    const uint64_t kind = s->seg_kind[segment];
    hipLaunchKernelGGL(kind == bj::lib::KIND   ? bj::gate_check_kernel<bj::lib::Program>
                       : kind == bj::p2g::KIND ? bj::gate_check_kernel<bj::p2g::Program>
                                               : bj::gate_check_kernel<bj::Interpreter>,
                       dim3((unsigned)blocks), dim3(bj::GT_THREADS), 0, st, seg, cols, row_begin, n_rows, status);
    hipLaunchKernelGGL(kind == bj::lib::KIND   ? bj::gate_value_kernel<bj::lib::Program>
                       : kind == bj::p2g::KIND ? bj::gate_value_kernel<bj::p2g::Program>
                                               : bj::gate_value_kernel<bj::Interpreter>,
                       dim3(1), dim3(bj::GC_WAVE), 0, st, seg, cols, row_begin, n_rows, status);
    return bj::ok_or(hipGetLastError(), "gate set satisfiability check");
}

}  // extern "C"
