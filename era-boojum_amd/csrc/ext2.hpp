// GoldilocksExt2 = F[u] / (u^2 - 7) (field/goldilocks/extension.rs:14-40) on top of gl.hpp: what
// fri.hip, deep.hip, stage2.hip and quotient.hip share.  Values are (c0, c1) pairs of u64
// representatives, not necessarily canonical; a kernel canonicalises what it writes.
#pragma once
#include "gl.hpp"
#if defined(__HIPCC__)
#include "gl_asm.hpp"
#endif

namespace bj {
namespace ext2 {

constexpr uint64_t EXT2_NON_RESIDUE = 7;  // GoldilocksExt2::NON_RESIDUE (extension.rs:14-16)
static_assert(EXT2_NON_RESIDUE == (1u << 3) - 1, "times7 multiplies by the non-residue as 2^3 v - v");

GL_FN uint64_t times7(uint64_t v) { return gl::sub(gl::mul_pow2_small(v, 3), v); }
GL_FN uint64_t neg(uint64_t v) { return gl::sub(0, v); }

struct E2 {
    uint64_t c0, c1;
};
// an element from two words of the C ABI, which need not be canonical
GL_FN E2 canon2(uint64_t c0, uint64_t c1) { return {gl::canon(c0), gl::canon(c1)}; }
// (a0 + a1 u)(b0 + b1 u) (field/traits/field.rs:407-424)
GL_FN E2 mul(E2 a, E2 b) {
    return {gl::add(gl::mul(a.c0, b.c0), times7(gl::mul(a.c1, b.c1))), gl::add(gl::mul(a.c0, b.c1), gl::mul(a.c1, b.c0))};
}
// norm(a) = a0^2 - 7 a1^2 in the base field; 1 / a = conj(a) / norm(a)
GL_FN uint64_t norm(E2 a) { return gl::sub(gl::mul(a.c0, a.c0), times7(gl::mul(a.c1, a.c1))); }
GL_FN bool is_zero(E2 a) { return (gl::canon(a.c0) | gl::canon(a.c1)) == 0; }

#if defined(__HIPCC__)
__device__ __forceinline__ uint32_t lo32(uint64_t v) { return (uint32_t)v; }
__device__ __forceinline__ uint32_t hi32(uint64_t v) { return (uint32_t)(v >> 32); }
__device__ __forceinline__ uint64_t u64_of(uint32_t lo, uint32_t hi) { return ((uint64_t)hi << 32) | lo; }

// a * b with the four products as one batch of the 14-instruction form (gl_asm.hpp): the product
// of a walk over columns (stage2.hip, quotient.hip)
__device__ __forceinline__ E2 mul_x4(E2 a, E2 b) {
    uint32_t zl[4], zh[4];
    glasm::mul_x4(lo32(a.c0), hi32(a.c0), lo32(b.c0), hi32(b.c0), zl[0], zh[0], lo32(a.c1), hi32(a.c1), lo32(b.c1),
                  hi32(b.c1), zl[1], zh[1], lo32(a.c0), hi32(a.c0), lo32(b.c1), hi32(b.c1), zl[2], zh[2], lo32(a.c1),
                  hi32(a.c1), lo32(b.c0), hi32(b.c0), zl[3], zh[3]);
    return {gl::add(u64_of(zl[0], zh[0]), times7(u64_of(zl[1], zh[1]))),
            gl::add(u64_of(zl[2], zh[2]), u64_of(zl[3], zh[3]))};
}

// a^(p - 2), p - 2 = (2^31 - 1) 2^33 + (2^32 - 1): 64 squarings and 10 products
__device__ __forceinline__ uint64_t sqn(uint64_t a, int k) {
    for (int i = 0; i < k; i++) a = gl::mul(a, a);
    return a;
}
static __device__ uint64_t inv_chain(uint64_t a) {
    const uint64_t t2 = gl::mul(sqn(a, 1), a);       // a^(2^2 - 1)
    const uint64_t t4 = gl::mul(sqn(t2, 2), t2);     // a^(2^4 - 1)
    const uint64_t t8 = gl::mul(sqn(t4, 4), t4);
    const uint64_t t16 = gl::mul(sqn(t8, 8), t8);
    const uint64_t t24 = gl::mul(sqn(t16, 8), t8);
    const uint64_t t28 = gl::mul(sqn(t24, 4), t4);
    const uint64_t t30 = gl::mul(sqn(t28, 2), t2);
    const uint64_t t31 = gl::mul(sqn(t30, 1), a);    // a^(2^31 - 1)
    const uint64_t t32 = gl::mul(sqn(t31, 1), a);    // a^(2^32 - 1)
    return gl::mul(sqn(t31, 33), t32);
}
#endif

}  // namespace ext2
}  // namespace bj
