// Native gate-set segment, kind 1: the Poseidon2 flattened gate over Goldilocks
// (Poseidon2RoundFunctionFlattenedEvaluator<F, 8, 12, 4>, cs/gates/poseidon2.rs:166-403).
//
// Captured as the reference writes it the gate is about 31 matrix layers of 144
// mul_and_accumulate_into each: several thousand relations and more than 16 live temporaries, so it
// passes neither BJ_GATE_MAX_INSTRUCTIONS nor BJ_GATE_MAX_SLOTS and the interpreter of gates.hip
// cannot run it.  Its structure is fixed, so it is written out here instead: one walk over an
// instance, layer by layer -- load the layer's cells, form the expected state from the 12 registers
// of the layer before, hand `expected - cell` to a sink, replace the state by the cells.  A lane
// holds 12 state words and the sink's own; no LDS, no barrier, no scratch.
//
// Cells of one repetition (130): variables 0..11 the input, 12..23 the output, then the 106
// "S-box output" cells in the order they are met (3 x 12 first half, 22 partial, 4 x 12 second
// half): cell s reads witness column s while s < nw (num_witness_columns_used, descriptor word [7])
// and variable column 24 + s - nw after that.  Terms in push order (118): the 36 + 22 + 48 resets,
// then output - state.  Which column a cell reads is wave-uniform, so the split costs scalar work.
//
// The external matrix is circ(2 M4, M4, M4) with adds and doublings, the inner matrix the sum plus
// the element shifted by SH; every constant is the reference's (poseidon2/params.rs).  Values are
// u64 representatives, any on input; what a sink keeps is canonicalised where it leaves the kernel.
//
// This file holds the gate's own: constants, matrices, S-boxes, the walk and the program kind that hands
// it to the frames.  Placement, selector, sinks and the three kernels are gates.hip's, which includes this
// inside namespace bj's unnamed namespace, after Cols and Placement; it needs gl.hpp and ext2.hpp.
#pragma once

namespace p2g {

constexpr uint32_t KIND = 1;
constexpr uint32_t SW = 12, HALF_FULL = 4, PARTIAL = 22;
constexpr uint32_t CELLS = 130, TERMS = 118, DEGREE = 7, MAX_WITNESS_CELLS = 106, FIXED_VARS = 2 * SW;
static_assert(MAX_WITNESS_CELLS == (HALF_FULL - 1) * SW + PARTIAL + HALF_FULL * SW, "the S-box output cells");
static_assert(CELLS == FIXED_VARS + MAX_WITNESS_CELLS && TERMS == MAX_WITNESS_CELLS + SW, "poseidon2.rs:422-437");

// ROUND_CONSTANTS_ALIGNED_PER_ROUND: rounds 0..3 and 26..29 are FULL_ROUND_CONSTANTS, element 0 of
// rounds 4..25 PARTIAL_ROUND_CONSTANTS (params.rs:107-136).  Read with a uniform index.
__constant__ const uint64_t RC[2 * HALF_FULL + PARTIAL][SW] = {
#include "poseidon2_rc.inc"
};
// INNER_ROUNDS_MATRIX_DIAGONAL_ELEMENTS_MINUS_ONE_SHIFTS (params.rs:35-36)
__device__ __forceinline__ constexpr int shift_of(uint32_t i) {
    constexpr int SH[SW] = {4, 14, 11, 8, 0, 5, 2, 9, 13, 6, 3, 12};
    return SH[i];
}

__device__ __forceinline__ uint64_t dbl(uint64_t a) { return gl::add(a, a); }

// x <- M4 x, M4 = [[5,7,1,3],[4,6,1,1],[1,3,5,7],[1,1,4,6]] (EXTERNAL_MDS_MATRIX_BLOCK): 8 adds, 6 doublings
__device__ __forceinline__ void m4(uint64_t* x) {
    const uint64_t t0 = gl::add(x[0], x[1]), t1 = gl::add(x[2], x[3]);
    const uint64_t t2 = gl::add(dbl(x[1]), t1), t3 = gl::add(dbl(x[3]), t0);
    const uint64_t t4 = gl::add(dbl(dbl(t1)), t3), t5 = gl::add(dbl(dbl(t0)), t2);
    x[0] = gl::add(t3, t5);
    x[1] = t5;
    x[2] = gl::add(t2, t4);
    x[3] = t4;
}

// x <- circ(2 M4, M4, M4) x (EXTERNAL_MDS_MATRIX, params.rs:63-94)
__device__ __forceinline__ void external_matrix(uint64_t (&x)[SW]) {
    m4(x), m4(x + 4), m4(x + 8);
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        const uint64_t s = gl::add(gl::add(x[j], x[4 + j]), x[8 + j]);
        x[j] = gl::add(x[j], s), x[4 + j] = gl::add(x[4 + j], s), x[8 + j] = gl::add(x[8 + j], s);
    }
}

// x <- (1 + diag(2^SH)) x (INNER_ROUNDS_MATRIX, params.rs:96-105)
__device__ __forceinline__ void inner_matrix(uint64_t (&x)[SW]) {
    uint64_t s = gl::add(x[0], x[1]);
#pragma unroll
    for (uint32_t i = 2; i < SW; i++) s = gl::add(s, x[i]);
#pragma unroll
    for (uint32_t i = 0; i < SW; i++) x[i] = gl::add(gl::mul_pow2_small(x[i], shift_of(i)), s);
}

// z[j] = a[j] b[j], four independent products in the 14-instruction form
__device__ __forceinline__ void mul4(const uint64_t* a, const uint64_t* b, uint64_t* z) {
    using namespace ext2;
    uint32_t zl[4], zh[4];
    glasm::mul_x4(lo32(a[0]), hi32(a[0]), lo32(b[0]), hi32(b[0]), zl[0], zh[0], lo32(a[1]), hi32(a[1]), lo32(b[1]),
                  hi32(b[1]), zl[1], zh[1], lo32(a[2]), hi32(a[2]), lo32(b[2]), hi32(b[2]), zl[2], zh[2], lo32(a[3]),
                  hi32(a[3]), lo32(b[3]), hi32(b[3]), zl[3], zh[3]);
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) z[j] = u64_of(zl[j], zh[j]);
}

// small_pow(7) as field_like.rs:92-101 forms it: x^2, x^4, x^6, x^7 -- 4 products
__device__ __forceinline__ uint64_t sbox(uint64_t x) {
    const uint64_t x2 = gl::mul(x, x);
    return gl::mul(gl::mul(gl::mul(x2, x2), x2), x);
}

// x[i] <- (x[i] + RC[round][i])^7 for the whole state, four elements to a batch of products
__device__ __forceinline__ void full_sboxes(uint64_t (&x)[SW], uint32_t round) {
#pragma unroll
    for (uint32_t b = 0; b < SW; b += 4) {
        uint64_t v[4], v2[4], v4[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) v[j] = gl::add(x[b + j], RC[round][b + j]);
        mul4(v, v, v2);
        mul4(v2, v2, v4);
        mul4(v4, v2, v4);
        mul4(v4, v, x + b);
    }
}

// Where the cells of one repetition are: the variable and witness columns at the repetition's
// offsets (coset 0 / row 0 of each) with their strides, and the split.  All wave-uniform.
struct Instance {
    const uint64_t* __restrict__ var;
    const uint64_t* __restrict__ wit;
    size_t var_stride, wit_stride;
    uint32_t nw;

    __device__ __forceinline__ uint64_t variable(uint32_t i, size_t L) const { return var[(size_t)i * var_stride + L]; }
    // S-box output cell s: witness column s while s < nw, variable column 24 + s - nw after that
    __device__ __forceinline__ uint64_t cell(uint32_t s, size_t L) const {
        const uint64_t* __restrict__ p =
            s < nw ? wit + (size_t)s * wit_stride : var + (size_t)(FIXED_VARS + s - nw) * var_stride;
        return p[L];
    }
};

// "reset" of the whole state (poseidon2.rs:224-244, 354-374): 12 terms, the state becomes the cells
template <class Sink>
__device__ __forceinline__ void reset(uint64_t (&x)[SW], const Instance& at, uint32_t& s, size_t L, Sink& sink) {
    uint64_t c[SW];
#pragma unroll
    for (uint32_t i = 0; i < SW; i++) c[i] = at.cell(s + i, L);
#pragma unroll
    for (uint32_t i = 0; i < SW; i++) {
        sink.emit(gl::sub(x[i], c[i]));
        x[i] = c[i];
    }
    s += SW;
}

// One instance at point (or row) L: 118 terms to the sink in push order.
template <class Sink>
__device__ __forceinline__ void walk(const Instance& at, size_t L, Sink& sink) {
    uint64_t x[SW];
#pragma unroll
    for (uint32_t i = 0; i < SW; i++) x[i] = at.variable(i, L);
    external_matrix(x);
    uint32_t s = 0;
#pragma unroll 1
    for (uint32_t round = 0; round < HALF_FULL; round++) {
        if (round) reset(x, at, s, L, sink);
        full_sboxes(x, round);
        external_matrix(x);
    }
#pragma unroll 1
    for (uint32_t round = 0; round < PARTIAL; round++, s++) {
        const uint64_t c = at.cell(s, L);
        sink.emit(gl::sub(gl::add(x[0], RC[HALF_FULL + round][0]), c));
        x[0] = sbox(c);
        inner_matrix(x);
    }
#pragma unroll 1
    for (uint32_t round = 0; round < HALF_FULL; round++) {
        reset(x, at, s, L, sink);
        full_sboxes(x, HALF_FULL + PARTIAL + round);
        external_matrix(x);
    }
#pragma unroll
    for (uint32_t i = 0; i < SW; i++) sink.emit(gl::sub(at.variable(SW + i, L), x[i]));
}

// The program kind the frames of gates.hip are instantiated with: one descriptor, nothing per gate,
// the selector columns loaded as they are met (a rolled loop), word [7] of the placement the split.
struct Program {
    static constexpr uint32_t SELECTOR_UNROLL = 1;
    static constexpr uint32_t GATES = 1;
    static constexpr uint32_t SLOTS = 0;
    const Cols& cols;
    const size_t L;

    __device__ __forceinline__ Program(const uint64_t* __restrict__, const Cols& cols, size_t L, uint64_t*)
        : cols(cols), L(L) {}
    __device__ __forceinline__ void gate(const uint64_t* __restrict__) {}
    __device__ __forceinline__ void read_selector_columns() {}
    __device__ __forceinline__ uint64_t selector_column(uint32_t i) const {
        return cols.p[2][(size_t)i * cols.stride[2] + L];
    }
    template <class Sink>
    __device__ __forceinline__ void walk(const Placement& pl, const uint32_t (&off)[3], Sink& sink) const {
        p2g::walk(Instance{cols.p[0] + (size_t)off[0] * cols.stride[0], cols.p[1] + (size_t)off[1] * cols.stride[1],
                           cols.stride[0], cols.stride[1], pl.word7},
                  L, sink);
    }
};

}  // namespace p2g
