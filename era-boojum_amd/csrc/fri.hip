// FRI folding by 2 of a GoldilocksExt2 codeword held as two base columns (c0, c1).
//
// fold_multiple (cs/implementations/fri/mod.rs:362-474), as used by
// interpolate_independent_cosets (:476-585) and interpolate_flattened_cosets (:587-682):
// the codeword is bit-reversed, so f(x) and f(-x) are neighbours (2i, 2i + 1), and
//   out_i = f(x) + f(-x) + alpha * (f(x) - f(-x)) * roots[i] * coset_inverse,
// with alpha = (ch0, ch1) in GoldilocksExt2 (u^2 = 7, field/goldilocks/extension.rs:14-40,
// product as field/traits/field.rs:407-424) and roots the INVERSED bit-reversed twiddles of the
// full domain (precompute_twiddles_for_fft::<true>, fri/mod.rs:191-192). Over several cosets
// stored one after another the root index is the flat pair index, which is what both
// reference loops use. Outputs are canonical.
//
// bj_fri_fold_multi_d folds by 2^r (r = 1..3, the range do_fri allows, fri/mod.rs:204-205) in one
// launch: the r by-2 steps of one reduction run on registers (fri_fold_multi_kernel).
#include <hip/hip_runtime.h>
#include "gl.hpp"
#include "gl_asm.hpp"
#include "ext2.hpp"
#include "stage_host.hpp"

namespace bj {

namespace {

// the non-residue 7, times7 and the halves lo32, hi32, u64_of
using namespace ext2;

// beta = alpha * coset_inverse (an Ext2 times a base element, folded on the host) and
// bsum = beta0 + beta1, so each output costs six products: (d0, d1) * roots[i] (2), the Karatsuba
// Ext2 product by beta (3) and the non-residue multiple (1), as interleaved gfx950 asm products
// (glasm, 14 instructions each).  Pairs (x, -x) are one 16-byte load per column when both
// columns are 16-byte aligned (V16), two 8-byte loads otherwise.
template <bool V16>
__device__ __forceinline__ ulonglong2 load_pair(const uint64_t* __restrict__ c, size_t i) {
    if constexpr (V16) return reinterpret_cast<const ulonglong2*>(c)[i];
    return make_ulonglong2(c[2 * i], c[2 * i + 1]);
}

// One fold_multiple step on one pair of each column: (f(x), f(-x)) = (x0, y0) + (x1, y1) u and the
// root r of the pair, beta and bsum in halves.  Canonical outputs.
struct Beta {
    uint32_t b0l, b0h, b1l, b1h, bsl, bsh;
};
__device__ __forceinline__ Beta beta_halves(uint64_t beta0, uint64_t beta1, uint64_t bsum) {
    return {lo32(beta0), hi32(beta0), lo32(beta1), hi32(beta1), lo32(bsum), hi32(bsum)};
}
__device__ __forceinline__ void fold_pair(uint64_t x0, uint64_t y0, uint64_t x1, uint64_t y1, uint64_t r,
                                          const Beta& b, uint64_t& o0, uint64_t& o1) {
    const uint64_t s0 = gl::sub(x0, y0), s1 = gl::sub(x1, y1);
    const uint32_t s0l = lo32(s0), s0h = hi32(s0), s1l = lo32(s1), s1h = hi32(s1), rl = lo32(r), rh = hi32(r);
    uint32_t a0l, a0h, a1l, a1h;
    glasm::mul_x2(s0l, s0h, rl, rh, a0l, a0h, s1l, s1h, rl, rh, a1l, a1h);
    const uint64_t sa = gl::add(u64_of(a0l, a0h), u64_of(a1l, a1h));
    const uint32_t sal = lo32(sa), sah = hi32(sa);
    // (a0 + a1 u) (beta0 + beta1 u), u^2 = 7 (field/traits/field.rs:407-424)
    uint32_t v0l, v0h, v1l, v1h, ml, mh;
    glasm::mul_x3(a0l, a0h, b.b0l, b.b0h, v0l, v0h, a1l, a1h, b.b1l, b.b1h, v1l, v1h, sal, sah, b.bsl, b.bsh, ml,
                  mh);
    const uint64_t v0 = u64_of(v0l, v0h), v1 = u64_of(v1l, v1h);
    const uint64_t e1 = gl::sub(gl::sub(u64_of(ml, mh), v0), v1);
    const uint64_t e0 = gl::add(v0, times7(v1));
    o0 = gl::canon(gl::add(gl::add(e0, x0), y0));
    o1 = gl::canon(gl::add(gl::add(e1, x1), y1));
}

template <bool V16>
__global__ __launch_bounds__(256) void fri_fold_kernel(const uint64_t* __restrict__ c0,
                                                       const uint64_t* __restrict__ c1, size_t n_out,
                                                       const uint64_t* __restrict__ roots, uint64_t beta0,
                                                       uint64_t beta1, uint64_t bsum, uint64_t* __restrict__ d0,
                                                       uint64_t* __restrict__ d1) {
    const Beta b = beta_halves(beta0, beta1, bsum);
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n_out; i += (size_t)gridDim.x * blockDim.x) {
        const ulonglong2 p0 = load_pair<V16>(c0, i), p1 = load_pair<V16>(c1, i);  // (f(x), f(-x))
        uint64_t o0, o1;
        fold_pair(p0.x, p0.y, p1.x, p1.y, roots[i], b, o0, o1);
        d0[i] = o0;
        d1[i] = o1;
    }
}

// Fold by 2^R in one pass: lane j holds the 2^R consecutive values [2^R j, 2^R (j + 1)) of each
// column in registers and folds them R times.  Step s folds the 2^(R-1-s) pairs at flat index
// i = 2^(R-1-s) j + t with roots[i] and beta_s = alpha^(2^s) coset_inverse^(2^s): exactly what R
// by-2 passes compute (each step's outputs canonical, as the by-2 kernel stores them), without
// the R - 1 round trips of the intermediate vectors.  Per output the pass moves 2 * 2^R values
// in, 2^R - 1 roots in and 2 values out.  V16: both columns and the root table are 16-byte
// aligned, so a lane's 2^R values (16, 32 or 64 bytes) and its root runs load as 16-byte words;
// otherwise everything is 8-byte loads.
struct FoldBetas {
    uint64_t beta0[3], beta1[3], bsum[3];
};

template <int N, bool V16>
__device__ __forceinline__ void load_run(const uint64_t* __restrict__ p, size_t first, uint64_t (&v)[8]) {
    if constexpr (V16 && N >= 2) {
        const ulonglong2* q = reinterpret_cast<const ulonglong2*>(p + first);  // first is a multiple of N
#pragma unroll
        for (int k = 0; k < N / 2; k++) {
            const ulonglong2 w = q[k];
            v[2 * k] = w.x;
            v[2 * k + 1] = w.y;
        }
    } else {
#pragma unroll
        for (int k = 0; k < N; k++) v[k] = p[first + k];
    }
}

template <int R, bool V16>
__global__ __launch_bounds__(256) void fri_fold_multi_kernel(const uint64_t* __restrict__ c0,
                                                             const uint64_t* __restrict__ c1, size_t n_out,
                                                             const uint64_t* __restrict__ roots, FoldBetas fb,
                                                             uint64_t* __restrict__ d0,
                                                             uint64_t* __restrict__ d1) {
    static_assert(R >= 2 && R <= 3, "fold by 4 or 8");
    const size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (j >= n_out) return;
    constexpr int W = 1 << R;
    uint64_t v0[8], v1[8], rt[3][8];
    load_run<W, V16>(c0, j * W, v0);
    load_run<W, V16>(c1, j * W, v1);
    // the 2^R - 1 roots: the runs roots[2^(R-1) j ...], roots[2^(R-2) j ...], roots[j]
    load_run<(W >> 1), V16>(roots, j * (W >> 1), rt[0]);
    load_run<(W >> 2), V16>(roots, j * (W >> 2), rt[1]);
    if constexpr (R == 3) load_run<1, V16>(roots, j, rt[2]);
#pragma unroll
    for (int s = 0; s < R; s++) {
        const Beta b = beta_halves(fb.beta0[s], fb.beta1[s], fb.bsum[s]);
#pragma unroll
        for (int t = 0; t < (W >> (s + 1)); t++) {
            uint64_t o0, o1;
            fold_pair(v0[2 * t], v0[2 * t + 1], v1[2 * t], v1[2 * t + 1], rt[s][t], b, o0, o1);
            v0[t] = o0;
            v1[t] = o1;
        }
    }
    d0[j] = v0[0];
    d1[j] = v1[0];
}

}  // namespace

hipError_t launch_fri_fold(const uint64_t* c0, const uint64_t* c1, size_t n_out, const uint64_t* roots,
                           uint64_t coset_inverse, uint64_t ch0, uint64_t ch1, uint64_t* d0, uint64_t* d1,
                           hipStream_t st) {
    if (n_out == 0) return hipSuccess;
    if (((uintptr_t)c0 | (uintptr_t)c1) % 8) return hipErrorInvalidValue;  // u64 elements
    size_t blocks = (n_out + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    const uint64_t beta0 = gl::canon(gl::mul(ch0, coset_inverse)), beta1 = gl::canon(gl::mul(ch1, coset_inverse));
    const uint64_t bsum = gl::canon(gl::add(beta0, beta1));
    if (((uintptr_t)c0 | (uintptr_t)c1) % 16 == 0)
        hipLaunchKernelGGL(fri_fold_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, c0, c1, n_out, roots,
                           beta0, beta1, bsum, d0, d1);
    else
        hipLaunchKernelGGL(fri_fold_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, c0, c1, n_out, roots,
                           beta0, beta1, bsum, d0, d1);
    return hipGetLastError();
}

namespace {

// Step s of a fold by 2^r takes alpha^(2^s) (the challenge squared per step, fri/mod.rs:218-224)
// and coset_inverse^(2^s) (squared after every fold, :554, :651); their product and its halves'
// sum are folded here, on the host, as launch_fri_fold does for one step.
FoldBetas fold_betas(uint64_t coset_inverse, uint64_t ch0, uint64_t ch1, uint32_t log_fold) {
    FoldBetas fb = {};
    uint64_t a0 = gl::canon(ch0), a1 = gl::canon(ch1), ci = gl::canon(coset_inverse);
    for (uint32_t s = 0; s < log_fold; s++) {
        fb.beta0[s] = gl::canon(gl::mul(a0, ci));
        fb.beta1[s] = gl::canon(gl::mul(a1, ci));
        fb.bsum[s] = gl::canon(gl::add(fb.beta0[s], fb.beta1[s]));
        // (a0 + a1 u)^2 = a0^2 + 7 a1^2 + 2 a0 a1 u (field/traits/field.rs:427-440)
        const uint64_t sq0 = gl::add(gl::mul(a0, a0), gl::mul(EXT2_NON_RESIDUE, gl::mul(a1, a1)));
        const uint64_t sq1 = gl::mul(2, gl::mul(a0, a1));
        a0 = gl::canon(sq0);
        a1 = gl::canon(sq1);
        ci = gl::canon(gl::mul(ci, ci));
    }
    return fb;
}

template <int R>
hipError_t launch_fold_multi(const uint64_t* c0, const uint64_t* c1, size_t n_out, const uint64_t* roots,
                             const FoldBetas& fb, uint64_t* d0, uint64_t* d1, hipStream_t st) {
    const size_t blocks = (n_out + 255) / 256;  // one output per lane, no stride loop
    if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
    if (((uintptr_t)c0 | (uintptr_t)c1 | (uintptr_t)roots) % 16 == 0)
        hipLaunchKernelGGL((fri_fold_multi_kernel<R, true>), dim3((unsigned)blocks), dim3(256), 0, st, c0, c1, n_out,
                           roots, fb, d0, d1);
    else
        hipLaunchKernelGGL((fri_fold_multi_kernel<R, false>), dim3((unsigned)blocks), dim3(256), 0, st, c0, c1, n_out,
                           roots, fb, d0, d1);
    return hipGetLastError();
}

}  // namespace

}  // namespace bj

extern "C" {

int bj_fri_fold_multi_d(const uint64_t* c0, const uint64_t* c1, size_t n_src, const uint64_t* roots,
                        uint64_t coset_inverse, uint64_t ch0, uint64_t ch1, uint32_t log_fold, uint64_t* dst_c0,
                        uint64_t* dst_c1, void* stream) {
    if (log_fold < 1 || log_fold > 3) return bj::set_error(BJ_EINVAL, "bj_fri_fold_multi_d: log_fold outside 1..3");
    if (n_src & (((size_t)1 << log_fold) - 1))
        return bj::set_error(BJ_EINVAL, "bj_fri_fold_multi_d: n_src is no multiple of 2^log_fold");
    if (n_src == 0) return BJ_OK;
    if (!c0 || !c1 || !roots || !dst_c0 || !dst_c1) return bj::set_error(BJ_EINVAL, "bj_fri_fold_multi_d: null pointer");
    if (((uintptr_t)c0 | (uintptr_t)c1 | (uintptr_t)roots | (uintptr_t)dst_c0 | (uintptr_t)dst_c1) % 8)
        return bj::set_error(BJ_EINVAL, "bj_fri_fold_multi_d: a pointer is not 8-byte aligned");
    const hipStream_t st = bj::S(stream);
    const size_t n_out = n_src >> log_fold;
    hipError_t e;
    if (log_fold == 1) {
        e = bj::launch_fri_fold(c0, c1, n_out, roots, coset_inverse, ch0, ch1, dst_c0, dst_c1, st);
    } else {
        const bj::FoldBetas fb = bj::fold_betas(coset_inverse, ch0, ch1, log_fold);
        e = log_fold == 2 ? bj::launch_fold_multi<2>(c0, c1, n_out, roots, fb, dst_c0, dst_c1, st)
                          : bj::launch_fold_multi<3>(c0, c1, n_out, roots, fb, dst_c0, dst_c1, st);
    }
    if (e == hipSuccess) return BJ_OK;
    char what[32];
    snprintf(what, sizeof what, "fri fold by 2^%u", log_fold);
    return bj::hip_fail(e, what);
}

}  // extern "C"
