// DEEP: evaluations at the out-of-domain point and the quotening pass that builds the FRI codeword.
//
// * bj_barycentric_weights_d: precompute_for_barycentric_evaluation_in_extension
//   (cs/implementations/utils.rs:907-1021), the Lagrange weights of coset * <w_n> at an Ext2 point.
// * bj_evaluate_at_d: barycentric_evaluate_base_at_extension_for_bitreversed_parallel
//   (utils.rs:1085-1158) for many columns at once, the sums of prover.rs:1501-1780.
// * bj_deep_quotient_d: one opening point of quotening_operation_in_extension
//   (prover.rs:2523-2706, driven by :1823-2050) over a row window of the flat bit-reversed domain.
// * bj_deep_codeword_d: every opening point over several column groups in one launch, with one
//   shared x and one base-field inversion per row pair.
//
// GoldilocksExt2 is (c0, c1) with u^2 = 7 (field/goldilocks/extension.rs:14-40).  The kernels see
// base columns only: the caller folds every source of an opening point, base or Ext2, into one
// Ext2 coefficient per base column and one Ext2 constant, so
//   sum_j ch_j (f_j(x) - v_j) = sum_c gamma_c col_c(x) - K.
// Field arithmetic is exact, so any order of operations gives the reference's bits once the
// outputs are canonical.
#include <hip/hip_runtime.h>
#include "gl.hpp"
#include "gl_asm.hpp"
#include "ext2.hpp"
#include "stage_host.hpp"

namespace bj {

namespace {

// the non-residue 7, times7, neg and the inversion chain inv_chain
using namespace ext2;

// Powers of one root w by 8-bit digits of the exponent: tab[256 k + b] = w^(b 2^(8k)), k < 4, and
// the digit-0 entries carry `scale` as well, so scale * w^e is three products for any e < 2^32.
constexpr uint32_t POW_TAB_WORDS = 1024;
__global__ __launch_bounds__(256) void pow_table_kernel(uint64_t* __restrict__ tab, uint64_t w, uint64_t scale) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    const uint32_t k = t >> 8, b = t & 255;
    uint64_t v = gl::pow(w, (uint64_t)b << (8 * k));
    if (k == 0) v = gl::mul(v, scale);
    tab[t] = gl::canon(v);
}
__device__ __forceinline__ uint64_t scaled_pow(const uint64_t* __restrict__ tab, uint32_t e) {
    const uint64_t lo = gl::mul(tab[e & 255], tab[256 + ((e >> 8) & 255)]);
    const uint64_t hi = gl::mul(tab[512 + ((e >> 16) & 255)], tab[768 + (e >> 24)]);
    return gl::mul(lo, hi);
}

// ------------------------------------------------------------------ barycentric weights
// w[bitrev_n(i)] = C' y / (at - y), y = coset w_n^i (tab), C' = (at^n - coset^n) / (n coset^n);
// the Ext2 inverse is conj / norm with one base inverse per element.  s7 = 7 at1^2.
__global__ __launch_bounds__(256) void weights_kernel(const uint64_t* __restrict__ tab, uint32_t log_n, uint64_t c0,
                                                      uint64_t c1, uint64_t at0, uint64_t at1, uint64_t s7,
                                                      uint64_t* __restrict__ w0, uint64_t* __restrict__ w1) {
    const size_t n = (size_t)1 << log_n;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const uint64_t y = scaled_pow(tab, (uint32_t)i);
        const uint64_t d0 = gl::sub(at0, y);
        const uint64_t ninv = inv_chain(gl::sub(gl::mul(d0, d0), s7));
        const uint64_t i0 = gl::mul(d0, ninv), i1 = gl::mul(neg(at1), ninv);  // 1 / (at - y)
        const uint64_t t0 = gl::mul(c0, y), t1 = gl::mul(c1, y);
        const size_t r = gl::bitrev32((uint32_t)i, log_n);
        w0[r] = gl::canon(gl::add(gl::mul(t0, i0), times7(gl::mul(t1, i1))));
        w1[r] = gl::canon(gl::add(gl::mul(t0, i1), gl::mul(t1, i0)));
    }
}
__global__ void weights_one_kernel(uint64_t* __restrict__ w0, uint64_t* __restrict__ w1) {
    w0[0] = 1;
    w1[0] = 0;
}

// ------------------------------------------------------------------ evaluate at z
// The sum over the four waves of a 256-thread block, in every thread.  Every thread of the block calls it.
__device__ __forceinline__ uint64_t block_sum(uint64_t v, uint64_t* ws) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v = gl::add(v, (uint64_t)__shfl_down((unsigned long long)v, d, 64));
    __syncthreads();  // the previous sum's readers are done with ws
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
    __syncthreads();
    return gl::add(gl::add(ws[0], ws[1]), gl::add(ws[2], ws[3]));
}

// Block (x = column tile, y = row range) sums rows [y rpb, (y + 1) rpb) of EVAL_TC columns: a thread
// keeps the weights of its row in registers across the tile's columns (two products per element)
// and its partial sums in registers across its rows; one block sum per column at the end.  Column
// tiles of one row range are neighbours in the grid, so the weights they share come from cache.
// partial: [row range][column][2], not canonical.
constexpr uint32_t EVAL_TC = 8;
constexpr size_t EVAL_MIN_ROWS = 1024;  // rows per block: at least four per thread
__global__ __launch_bounds__(256) void evaluate_partial_kernel(const uint64_t* __restrict__ cols, uint32_t n_cols,
                                                               size_t col_stride, size_t n, size_t rpb,
                                                               const uint64_t* __restrict__ w0,
                                                               const uint64_t* __restrict__ w1,
                                                               uint64_t* __restrict__ partial) {
    __shared__ uint64_t ws[4];
    const uint32_t c0 = blockIdx.x * EVAL_TC;
    const uint32_t nc = n_cols - c0 < EVAL_TC ? n_cols - c0 : EVAL_TC;
    const size_t start = (size_t)blockIdx.y * rpb;
    const size_t end = start + rpb < n ? start + rpb : n;
    const uint64_t* base = cols + (size_t)c0 * col_stride;
    uint64_t s0[EVAL_TC], s1[EVAL_TC];
#pragma unroll
    for (uint32_t j = 0; j < EVAL_TC; j++) s0[j] = s1[j] = 0;
    for (size_t r = start + threadIdx.x; r < end; r += 256) {
        const uint64_t a = w0[r], b = w1[r];
        const uint32_t al = (uint32_t)a, ah = (uint32_t)(a >> 32), bl = (uint32_t)b, bh = (uint32_t)(b >> 32);
        uint64_t f[EVAL_TC];
#pragma unroll
        for (uint32_t j = 0; j < EVAL_TC; j++) f[j] = j < nc ? base[(size_t)j * col_stride + r] : 0;
#pragma unroll
        for (uint32_t j = 0; j < EVAL_TC; j += 2) {
            const uint32_t fl = (uint32_t)f[j], fh = (uint32_t)(f[j] >> 32);
            const uint32_t gl_ = (uint32_t)f[j + 1], gh = (uint32_t)(f[j + 1] >> 32);
            uint32_t zl[4], zh[4];
            glasm::mul_x4(fl, fh, al, ah, zl[0], zh[0], fl, fh, bl, bh, zl[1], zh[1],
                          gl_, gh, al, ah, zl[2], zh[2], gl_, gh, bl, bh, zl[3], zh[3]);
            s0[j] = gl::add(s0[j], ((uint64_t)zh[0] << 32) | zl[0]);
            s1[j] = gl::add(s1[j], ((uint64_t)zh[1] << 32) | zl[1]);
            s0[j + 1] = gl::add(s0[j + 1], ((uint64_t)zh[2] << 32) | zl[2]);
            s1[j + 1] = gl::add(s1[j + 1], ((uint64_t)zh[3] << 32) | zl[3]);
        }
    }
    uint64_t* out = partial + ((size_t)blockIdx.y * n_cols + c0) * 2;
#pragma unroll
    for (uint32_t j = 0; j < EVAL_TC; j++) {
        if (j < nc) {  // block-uniform
            const uint64_t t0 = block_sum(s0[j], ws), t1 = block_sum(s1[j], ws);
            if (threadIdx.x == 0) {
                out[2 * j] = t0;
                out[2 * j + 1] = t1;
            }
        }
    }
}

// One block per column: the sum over the row ranges in a fixed order, canonical.
__global__ __launch_bounds__(256) void evaluate_finish_kernel(const uint64_t* __restrict__ partial, uint32_t n_cols,
                                                              uint32_t n_ranges, uint64_t* __restrict__ out) {
    __shared__ uint64_t ws[4];
    const uint32_t c = blockIdx.x;
    uint64_t a0 = 0, a1 = 0;
    for (uint32_t b = threadIdx.x; b < n_ranges; b += 256) {
        a0 = gl::add(a0, partial[((size_t)b * n_cols + c) * 2]);
        a1 = gl::add(a1, partial[((size_t)b * n_cols + c) * 2 + 1]);
    }
    const uint64_t t0 = block_sum(a0, ws), t1 = block_sum(a1, ws);
    if (threadIdx.x == 0) {
        out[2 * (size_t)c] = gl::canon(t0);
        out[2 * (size_t)c + 1] = gl::canon(t1);
    }
}

// ------------------------------------------------------------------ quotening
// acc += f * (g0, g1) for the two rows of a pair; the coefficient is wave-uniform (SGPRs)
__device__ __forceinline__ void fma_pair(uint64_t fe, uint64_t fo, uint64_t g0, uint64_t g1, uint64_t (&acc)[4]) {
    uint32_t zl[4], zh[4];
    const uint32_t el = (uint32_t)fe, eh = (uint32_t)(fe >> 32), ol = (uint32_t)fo, oh = (uint32_t)(fo >> 32);
    const uint32_t g0l = (uint32_t)g0, g0h = (uint32_t)(g0 >> 32), g1l = (uint32_t)g1, g1h = (uint32_t)(g1 >> 32);
    glasm::mul_sb_x4(el, eh, g0l, g0h, zl[0], zh[0], el, eh, g1l, g1h, zl[1], zh[1],
                     ol, oh, g0l, g0h, zl[2], zh[2], ol, oh, g1l, g1h, zl[3], zh[3]);
#pragma unroll
    for (int i = 0; i < 4; i++) acc[i] = gl::add(acc[i], ((uint64_t)zh[i] << 32) | zl[i]);
}

// A thread owns the rows (2i, 2i + 1) of global pair i: in the bit-reversed domain they are the
// points (x, -x), x = 7 w_N^(bitrev_{log N - 1}(i)) (tab), so the two Ext2 inverses 1 / (+-x - at) share
// one base inverse: norms (x - at0)^2 - 7 at1^2 and (x + at0)^2 - 7 at1^2, one inversion of their
// product.  Lanes are consecutive pairs, so a column's load is contiguous over the wave; the
// columns are looped with the coefficient table read through a uniform index.  V16: the window
// starts and ends on a pair and every column is 16-byte aligned, so a pair is one 16-byte load and
// store; otherwise 8-byte accesses, each row checked against the window.
constexpr uint32_t DQ_UNROLL = 8;
template <bool V16>
__global__ __launch_bounds__(256) void deep_quotient_kernel(
    const uint64_t* __restrict__ cols, uint32_t n_cols, size_t col_stride, const uint64_t* __restrict__ gammas,
    uint64_t k0, uint64_t k1, uint64_t at0, uint64_t at1, uint64_t s7, const uint64_t* __restrict__ tab,
    uint32_t pair_bits, size_t row0, size_t n_rows, size_t n_pairs, uint64_t* __restrict__ dst0,
    uint64_t* __restrict__ dst1, int accumulate) {
    const size_t t = blockIdx.x * (size_t)256 + threadIdx.x;
    if (t >= n_pairs) return;
    const size_t pair = (row0 >> 1) + t;
    // window-relative index of the pair's even row (-1 when the window starts on an odd row)
    const ptrdiff_t rel = (ptrdiff_t)(2 * pair) - (ptrdiff_t)row0;
    const bool in_e = V16 || (rel >= 0 && (size_t)rel < n_rows);
    const bool in_o = V16 || (size_t)(rel + 1) < n_rows;
    auto load = [&](const uint64_t* col, uint64_t& fe, uint64_t& fo) {
        if constexpr (V16) {
            const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(col + rel);
            fe = v.x;
            fo = v.y;
        } else {
            fe = in_e ? col[rel] : 0;
            fo = in_o ? col[rel + 1] : 0;
        }
    };
    uint64_t acc[4] = {0, 0, 0, 0};  // even row (c0, c1), odd row (c0, c1)
    uint32_t c = 0;
    for (; c + DQ_UNROLL <= n_cols; c += DQ_UNROLL) {  // DQ_UNROLL columns' loads in flight per lane
        uint64_t fe[DQ_UNROLL], fo[DQ_UNROLL];
#pragma unroll
        for (uint32_t j = 0; j < DQ_UNROLL; j++) load(cols + (size_t)(c + j) * col_stride, fe[j], fo[j]);
#pragma unroll
        for (uint32_t j = 0; j < DQ_UNROLL; j++) fma_pair(fe[j], fo[j], gammas[2 * (c + j)], gammas[2 * (c + j) + 1], acc);
    }
    for (; c < n_cols; c++) {
        uint64_t fe, fo;
        load(cols + (size_t)c * col_stride, fe, fo);
        fma_pair(fe, fo, gammas[2 * c], gammas[2 * c + 1], acc);
    }
    const uint64_t x = scaled_pow(tab, gl::bitrev32((uint32_t)pair, pair_bits));
    const uint64_t de = gl::sub(x, at0), xa = gl::add(x, at0);  // the odd row's c0 is -xa
    uint64_t ne = gl::sub(gl::mul(de, de), s7), no = gl::sub(gl::mul(xa, xa), s7);
    if (!in_e) ne = 1;  // a row outside the window (or the domain) must not enter the shared inverse
    if (!in_o) no = 1;
    const uint64_t inv = inv_chain(gl::mul(ne, no));
    const uint64_t ie = gl::mul(inv, no), io = gl::mul(inv, ne);
    // 1 / (d0 - at1 u) = (d0 + at1 u) / norm
    const uint64_t e0 = gl::mul(de, ie), e1 = gl::mul(at1, ie);
    const uint64_t o0 = gl::mul(neg(xa), io), o1 = gl::mul(at1, io);
    const uint64_t me0 = gl::sub(acc[0], k0), me1 = gl::sub(acc[1], k1);
    const uint64_t mo0 = gl::sub(acc[2], k0), mo1 = gl::sub(acc[3], k1);
    uint64_t qe0 = gl::add(gl::mul(me0, e0), times7(gl::mul(me1, e1)));
    uint64_t qe1 = gl::add(gl::mul(me0, e1), gl::mul(me1, e0));
    uint64_t qo0 = gl::add(gl::mul(mo0, o0), times7(gl::mul(mo1, o1)));
    uint64_t qo1 = gl::add(gl::mul(mo0, o1), gl::mul(mo1, o0));
    if constexpr (V16) {
        ulonglong2* p0 = reinterpret_cast<ulonglong2*>(dst0 + rel);
        ulonglong2* p1 = reinterpret_cast<ulonglong2*>(dst1 + rel);
        if (accumulate) {
            const ulonglong2 a = *p0, b = *p1;
            qe0 = gl::add(qe0, a.x);
            qo0 = gl::add(qo0, a.y);
            qe1 = gl::add(qe1, b.x);
            qo1 = gl::add(qo1, b.y);
        }
        *p0 = make_ulonglong2(gl::canon(qe0), gl::canon(qo0));
        *p1 = make_ulonglong2(gl::canon(qe1), gl::canon(qo1));
    } else {
        if (in_e) {
            if (accumulate) {
                qe0 = gl::add(qe0, dst0[rel]);
                qe1 = gl::add(qe1, dst1[rel]);
            }
            dst0[rel] = gl::canon(qe0);
            dst1[rel] = gl::canon(qe1);
        }
        if (in_o) {
            if (accumulate) {
                qo0 = gl::add(qo0, dst0[rel + 1]);
                qo1 = gl::add(qo1, dst1[rel + 1]);
            }
            dst0[rel + 1] = gl::canon(qo0);
            dst1[rel + 1] = gl::canon(qo1);
        }
    }
}

// ------------------------------------------------------------------ the codeword in one launch
// Every opening point of bj_deep_codeword_d.  The arguments travel by value: a term is a column
// range of one group with its coefficients, the terms of point p are [term_end[p - 1], term_end[p]).
constexpr uint32_t CW_POINTS = BJ_DEEP_MAX_POINTS;
constexpr uint32_t CW_TERMS = BJ_DEEP_MAX_TERMS;
struct CwTerm {
    const uint64_t* base;    // the range's first column, window-relative
    size_t stride;
    const uint64_t* gammas;  // n_cols x 2
    uint32_t n_cols, pad;
};
struct CwPoint {
    uint64_t at0, at1, s7, k0, k1;  // canonical; s7 = 7 at1^2
};
struct CwArgs {
    CwTerm term[CW_TERMS];
    CwPoint point[CW_POINTS];
    uint32_t term_end[CW_POINTS];
    uint64_t wpow[32];  // w_{2^log_domain}^(2^b)
    uint32_t n_points, pair_bits;
};
static_assert(sizeof(CwArgs) <= 3600, "the kernel arguments hold 4096 bytes");
static_assert(sizeof(bj_deep_codeword_t) == 904, "the descriptor of the C ABI");

// deep_quotient_kernel's thread (the row pair (x, -x), the same loads, the same column walk), with
// x computed once from the powers in the arguments and shared by the points, and one inversion for
// all of them: phase 1 takes the product of the norms of x - at_p and -x - at_p for every p, inverts
// the product of those and unwinds it into one inverse per point (Montgomery's trick, unrolled over
// the cap so the arrays stay in registers); phase 2 walks the points, each term's columns as the
// one-point kernel does, splits the point's inverse between its two rows with the norms computed
// again, multiplies and adds into one Ext2 sum per row, written once.
template <bool V16>
__global__ __launch_bounds__(256) void deep_codeword_kernel(CwArgs a, size_t row0, size_t n_rows, size_t n_pairs,
                                                            uint64_t* __restrict__ dst0, uint64_t* __restrict__ dst1,
                                                            int accumulate) {
    const size_t t = blockIdx.x * (size_t)256 + threadIdx.x;
    if (t >= n_pairs) return;
    const size_t pair = (row0 >> 1) + t;
    const ptrdiff_t rel = (ptrdiff_t)(2 * pair) - (ptrdiff_t)row0;
    const bool in_e = V16 || (rel >= 0 && (size_t)rel < n_rows);
    const bool in_o = V16 || (size_t)(rel + 1) < n_rows;
    auto load = [&](const uint64_t* col, uint64_t& fe, uint64_t& fo) {
        if constexpr (V16) {
            const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(col + rel);
            fe = v.x;
            fo = v.y;
        } else {
            fe = in_e ? col[rel] : 0;
            fo = in_o ? col[rel + 1] : 0;
        }
    };
    // x = 7 w^(bitrev(pair))
    uint64_t x = gl::GENERATOR;
    {
        const uint32_t e = gl::bitrev32((uint32_t)pair, a.pair_bits);
        for (uint32_t b = 0; b < a.pair_bits; b++) x = gl::mul(x, (e >> b) & 1 ? a.wpow[b] : 1);
    }
    // phase 1: ip[p] = 1 / (norm(x - at_p) norm(-x - at_p)), a row outside the window counting as norm 1
    auto norms = [&](uint32_t p, uint64_t& de, uint64_t& xa, uint64_t& ne, uint64_t& no) {
        de = gl::sub(x, a.point[p].at0);
        xa = gl::add(x, a.point[p].at0);  // the odd row's c0 is -xa
        ne = in_e ? gl::sub(gl::mul(de, de), a.point[p].s7) : 1;
        no = in_o ? gl::sub(gl::mul(xa, xa), a.point[p].s7) : 1;
    };
    uint64_t ip[CW_POINTS];
    {
        uint64_t nn[CW_POINTS];
        uint64_t run = 1;
#pragma unroll
        for (uint32_t p = 0; p < CW_POINTS; p++) {
            ip[p] = nn[p] = 1;
            if (p < a.n_points) {  // wave-uniform
                uint64_t de, xa, ne, no;
                norms(p, de, xa, ne, no);
                nn[p] = gl::mul(ne, no);
                ip[p] = run;  // the product of the points before p, for now
                run = gl::mul(run, nn[p]);
            }
        }
        uint64_t inv = inv_chain(run);
#pragma unroll
        for (int p = CW_POINTS - 1; p >= 0; p--) {
            if ((uint32_t)p < a.n_points) {
                ip[p] = gl::mul(inv, ip[p]);
                inv = gl::mul(inv, nn[p]);
            }
        }
    }
    // phase 2
    uint64_t q[4] = {0, 0, 0, 0};  // even row (c0, c1), odd row (c0, c1)
    uint32_t ti = 0;
    for (uint32_t p = 0; p < a.n_points; p++) {
        uint64_t acc[4] = {0, 0, 0, 0};
        const uint32_t te = a.term_end[p];
        for (; ti < te; ti++) {
            const uint64_t* __restrict__ cols = a.term[ti].base;
            const uint64_t* __restrict__ gammas = a.term[ti].gammas;
            const size_t col_stride = a.term[ti].stride;
            const uint32_t n_cols = a.term[ti].n_cols;
            uint32_t c = 0;
            for (; c + DQ_UNROLL <= n_cols; c += DQ_UNROLL) {
                uint64_t fe[DQ_UNROLL], fo[DQ_UNROLL];
#pragma unroll
                for (uint32_t j = 0; j < DQ_UNROLL; j++) load(cols + (size_t)(c + j) * col_stride, fe[j], fo[j]);
#pragma unroll
                for (uint32_t j = 0; j < DQ_UNROLL; j++)
                    fma_pair(fe[j], fo[j], gammas[2 * (c + j)], gammas[2 * (c + j) + 1], acc);
            }
            for (; c < n_cols; c++) {
                uint64_t fe, fo;
                load(cols + (size_t)c * col_stride, fe, fo);
                fma_pair(fe, fo, gammas[2 * c], gammas[2 * c + 1], acc);
            }
        }
        // the point's inverse: a select chain on the wave-uniform p, so ip stays in registers
        uint64_t ipp = ip[0];
#pragma unroll
        for (uint32_t k = 1; k < CW_POINTS; k++) ipp = p == k ? ip[k] : ipp;
        uint64_t de, xa, ne, no;
        norms(p, de, xa, ne, no);
        const uint64_t iep = gl::mul(ipp, no), iop = gl::mul(ipp, ne), at1 = a.point[p].at1;
        // 1 / (d0 - at1 u) = (d0 + at1 u) / norm
        const E2 inv_e = {gl::mul(de, iep), gl::mul(at1, iep)};
        const E2 inv_o = {gl::mul(neg(xa), iop), gl::mul(at1, iop)};
        const E2 me = {gl::sub(acc[0], a.point[p].k0), gl::sub(acc[1], a.point[p].k1)};
        const E2 mo = {gl::sub(acc[2], a.point[p].k0), gl::sub(acc[3], a.point[p].k1)};
        const E2 re = mul_x4(me, inv_e), ro = mul_x4(mo, inv_o);
        q[0] = gl::add(q[0], re.c0);
        q[1] = gl::add(q[1], re.c1);
        q[2] = gl::add(q[2], ro.c0);
        q[3] = gl::add(q[3], ro.c1);
    }
    if constexpr (V16) {
        ulonglong2* p0 = reinterpret_cast<ulonglong2*>(dst0 + rel);
        ulonglong2* p1 = reinterpret_cast<ulonglong2*>(dst1 + rel);
        if (accumulate) {
            const ulonglong2 u = *p0, v = *p1;
            q[0] = gl::add(q[0], u.x);
            q[2] = gl::add(q[2], u.y);
            q[1] = gl::add(q[1], v.x);
            q[3] = gl::add(q[3], v.y);
        }
        *p0 = make_ulonglong2(gl::canon(q[0]), gl::canon(q[2]));
        *p1 = make_ulonglong2(gl::canon(q[1]), gl::canon(q[3]));
    } else {
        if (in_e) {
            if (accumulate) {
                q[0] = gl::add(q[0], dst0[rel]);
                q[1] = gl::add(q[1], dst1[rel]);
            }
            dst0[rel] = gl::canon(q[0]);
            dst1[rel] = gl::canon(q[1]);
        }
        if (in_o) {
            if (accumulate) {
                q[2] = gl::add(q[2], dst0[rel + 1]);
                q[3] = gl::add(q[3], dst1[rel + 1]);
            }
            dst0[rel + 1] = gl::canon(q[2]);
            dst1[rel + 1] = gl::canon(q[3]);
        }
    }
}

// ------------------------------------------------------------------ launchers
hipError_t launch_pow_table(uint64_t* tab, uint64_t w, uint64_t scale, hipStream_t st) {
    hipLaunchKernelGGL(pow_table_kernel, dim3(POW_TAB_WORDS / 256), dim3(256), 0, st, tab, w, scale);
    return hipGetLastError();
}

hipError_t launch_weights(uint32_t log_n, uint64_t coset, uint64_t at0, uint64_t at1, uint64_t* w0, uint64_t* w1,
                          hipStream_t st) {
    if (log_n == 0) {  // n == 1: (1, 0) (utils.rs:919-927)
        hipLaunchKernelGGL(weights_one_kernel, dim3(1), dim3(1), 0, st, w0, w1);
        return hipGetLastError();
    }
    const size_t n = (size_t)1 << log_n;
    // C' = (at^n - coset^n) / (n coset^n) (utils.rs:933-945 without the factor coset, which the kernel's y carries)
    coset = gl::canon(coset);
    E2 an = canon2(at0, at1);
    uint64_t cn = coset;
    for (uint32_t i = 0; i < log_n; i++) {
        an = mul(an, an);
        cn = gl::mul(cn, cn);
    }
    const uint64_t k = gl::inv(gl::mul(cn, gl::canon((uint64_t)n)));
    const uint64_t c0 = gl::canon(gl::mul(gl::sub(an.c0, cn), k)), c1 = gl::canon(gl::mul(an.c1, k));
    const uint64_t s7 = gl::canon(times7(gl::mul(at1, at1)));
    Workspace ws(st);
    uint64_t* tab = nullptr;
    if (hipError_t e = ws.alloc(&tab, POW_TAB_WORDS)) return e;
    if (hipError_t e = launch_pow_table(tab, gl::domain_generator(log_n), coset, st)) return e;
    size_t blocks = (n + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(weights_kernel, dim3((unsigned)blocks), dim3(256), 0, st, tab, log_n, c0, c1, gl::canon(at0),
                       gl::canon(at1), s7, w0, w1);
    return hipGetLastError();
}

hipError_t launch_evaluate_at(const uint64_t* cols, uint32_t n_cols, size_t col_stride, uint32_t log_n,
                              const uint64_t* w0, const uint64_t* w1, uint64_t* out, hipStream_t st) {
    if (n_cols == 0) return hipSuccess;
    const size_t n = (size_t)1 << log_n;
    const uint32_t tiles = (n_cols + EVAL_TC - 1) / EVAL_TC;
    // about 4096 blocks, at most 1024 row ranges (a power of two, so the ranges are equal)
    size_t max_ranges = 1;
    while (max_ranges < 1024 && max_ranges * 2 * tiles <= 4096) max_ranges *= 2;
    size_t rpb = n / max_ranges;
    if (rpb < EVAL_MIN_ROWS) rpb = EVAL_MIN_ROWS;
    const size_t ranges = (n + rpb - 1) / rpb;
    Workspace ws(st);
    uint64_t* partial = nullptr;
    if (hipError_t e = ws.alloc(&partial, ranges * n_cols * 2)) return e;
    hipLaunchKernelGGL(evaluate_partial_kernel, dim3(tiles, (unsigned)ranges), dim3(256), 0, st, cols, n_cols,
                       col_stride, n, rpb, w0, w1, partial);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(evaluate_finish_kernel, dim3(n_cols), dim3(256), 0, st, partial, n_cols, (uint32_t)ranges, out);
    return hipGetLastError();
}

hipError_t launch_deep_quotient(const uint64_t* cols, uint32_t n_cols, size_t col_stride, const uint64_t* gammas,
                                uint64_t k0, uint64_t k1, uint64_t at0, uint64_t at1, uint32_t log_domain, size_t row0,
                                size_t n_rows, uint64_t* dst0, uint64_t* dst1, int accumulate, hipStream_t st) {
    if (n_rows == 0) return hipSuccess;
    at0 = gl::canon(at0);
    at1 = gl::canon(at1);
    const uint64_t s7 = gl::canon(times7(gl::mul(at1, at1)));
    Workspace ws(st);
    uint64_t* tab = nullptr;
    if (hipError_t e = ws.alloc(&tab, POW_TAB_WORDS)) return e;
    if (hipError_t e = launch_pow_table(tab, gl::domain_generator(log_domain), gl::GENERATOR, st)) return e;
    const uint32_t pair_bits = log_domain ? log_domain - 1 : 0;
    const size_t n_pairs = ((row0 + n_rows + 1) >> 1) - (row0 >> 1);
    const size_t blocks = (n_pairs + 255) / 256;  // at most 2^23
    uintptr_t align = (uintptr_t)dst0 | (uintptr_t)dst1;
    if (n_cols) align |= (uintptr_t)cols;
    const bool v16 = (row0 & 1) == 0 && (n_rows & 1) == 0 && align % 16 == 0 && (n_cols <= 1 || (col_stride & 1) == 0);
    auto kernel = v16 ? deep_quotient_kernel<true> : deep_quotient_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, st, cols, n_cols, col_stride, gammas,
                       gl::canon(k0), gl::canon(k1), at0, at1, s7, tab, pair_bits, row0, n_rows, n_pairs, dst0, dst1,
                       accumulate);
    return hipGetLastError();
}

// NULL when the descriptor's shape is sound (what can be said without looking at n_rows)
const char* bad_codeword(const bj_deep_codeword_t& d) {
    if (d.n_groups > BJ_DEEP_MAX_GROUPS) return "bj_deep_codeword_d: more than BJ_DEEP_MAX_GROUPS groups";
    if (d.n_points > BJ_DEEP_MAX_POINTS) return "bj_deep_codeword_d: more than BJ_DEEP_MAX_POINTS points";
    if (d.n_terms > BJ_DEEP_MAX_TERMS) return "bj_deep_codeword_d: more than BJ_DEEP_MAX_TERMS terms";
    if (d.log_domain > 32) return "log_domain exceeds the 2-adicity (32) of the field";
    const size_t domain = (size_t)1 << d.log_domain;
    if (d.n_rows > domain || d.row0 > domain - d.n_rows) return "bj_deep_codeword_d: row0 + n_rows exceeds 2^log_domain";
    for (uint32_t t = 0; t < d.n_terms; t++) {
        const bj_deep_term_t& m = d.terms[t];
        if (m.group >= d.n_groups) return "bj_deep_codeword_d: a term names a missing group";
        if (m.point >= d.n_points) return "bj_deep_codeword_d: a term names a missing point";
        const uint32_t gc = d.groups[m.group].n_cols;
        if (m.first_col > gc || m.n_cols > gc - m.first_col) return "bj_deep_codeword_d: a term's columns lie outside its group";
        if (m.gamma_offset > d.n_gammas || m.n_cols > d.n_gammas - m.gamma_offset)
            return "bj_deep_codeword_d: a term's coefficients lie outside gammas";
        if (t && m.point < d.terms[t - 1].point) return "bj_deep_codeword_d: terms are not sorted by point";
    }
    return nullptr;
}
const char* bad_codeword_pointers(const bj_deep_codeword_t& d) {
    if (!d.dst0 || !d.dst1) return "bj_deep_codeword_d: null dst";
    if (d.n_gammas && !d.gammas) return "bj_deep_codeword_d: null gammas";
    for (uint32_t g = 0; g < d.n_groups; g++) {
        if (d.groups[g].n_cols && !d.groups[g].cols) return "bj_deep_codeword_d: null cols";
        if (d.groups[g].n_cols && d.groups[g].col_stride < d.n_rows) return "bj_deep_codeword_d: col_stride < n_rows";
    }
    return nullptr;
}

// d has passed both checks and n_rows > 0
hipError_t launch_deep_codeword(const bj_deep_codeword_t& d, hipStream_t st) {
    CwArgs a = {};
    uintptr_t align = (uintptr_t)d.dst0 | (uintptr_t)d.dst1;
    bool even_strides = true;
    uint32_t t = 0;
    for (uint32_t p = 0; p < d.n_points; p++) {
        const uint64_t at1 = gl::canon(d.points[p].at1);
        a.point[p] = {gl::canon(d.points[p].at0), at1, gl::canon(times7(gl::mul(at1, at1))), gl::canon(d.points[p].k0),
                      gl::canon(d.points[p].k1)};
        for (; t < d.n_terms && d.terms[t].point == p; t++) {
            const bj_deep_term_t& m = d.terms[t];
            const bj_deep_group_t& g = d.groups[m.group];
            a.term[t] = {m.n_cols ? g.cols + (size_t)m.first_col * g.col_stride : nullptr, g.col_stride,
                         m.n_cols ? d.gammas + 2 * (size_t)m.gamma_offset : nullptr, m.n_cols, 0};
            if (m.n_cols) align |= (uintptr_t)a.term[t].base;
            if (m.n_cols > 1 && (g.col_stride & 1)) even_strides = false;
        }
        a.term_end[p] = t;
    }
    a.n_points = d.n_points;
    a.pair_bits = d.log_domain ? d.log_domain - 1 : 0;
    fill_wpow(a.wpow, d.log_domain);
    const size_t n_pairs = ((d.row0 + d.n_rows + 1) >> 1) - (d.row0 >> 1);
    const size_t blocks = (n_pairs + 255) / 256;  // at most 2^23
    const bool v16 = (d.row0 & 1) == 0 && (d.n_rows & 1) == 0 && align % 16 == 0 && even_strides;
    auto kernel = v16 ? deep_codeword_kernel<true> : deep_codeword_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, st, a, d.row0, d.n_rows, n_pairs, d.dst0, d.dst1,
                       (int)d.accumulate);
    return hipGetLastError();
}

}  // namespace

}  // namespace bj

extern "C" {

int bj_barycentric_weights_d(uint32_t log_n, uint64_t coset, uint64_t at0, uint64_t at1, uint64_t* w0, uint64_t* w1,
                             void* stream) {
    if (const char* why = bj::bad_log_n(log_n)) return bj::set_error(BJ_EINVAL, why);
    if (!w0 || !w1) return bj::set_error(BJ_EINVAL, "bj_barycentric_weights_d: null output");
    if (gl::canon(coset) == 0) return bj::set_error(BJ_EINVAL, "bj_barycentric_weights_d: coset must be non-zero");
    const hipError_t e = bj::launch_weights(log_n, coset, at0, at1, w0, w1, bj::S(stream));
    return bj::ok_or(e, "barycentric weights");
}

int bj_evaluate_at_d(const uint64_t* cols, uint32_t n_cols, size_t col_stride, uint32_t log_n, const uint64_t* w0,
                     const uint64_t* w1, uint64_t* out, void* stream) {
    if (const char* why = bj::bad_log_n(log_n)) return bj::set_error(BJ_EINVAL, why);
    if (n_cols == 0) return BJ_OK;
    if (!cols || !w0 || !w1 || !out) return bj::set_error(BJ_EINVAL, "bj_evaluate_at_d: null pointer");
    if (col_stride < ((size_t)1 << log_n)) return bj::set_error(BJ_EINVAL, "bj_evaluate_at_d: col_stride < 2^log_n");
    const hipError_t e = bj::launch_evaluate_at(cols, n_cols, col_stride, log_n, w0, w1, out, bj::S(stream));
    return bj::ok_or(e, "evaluate at");
}

int bj_deep_quotient_d(const uint64_t* cols, uint32_t n_cols, size_t col_stride, const uint64_t* gammas, uint64_t k0,
                       uint64_t k1, uint64_t at0, uint64_t at1, uint32_t log_domain, size_t row0, size_t n_rows,
                       uint64_t* dst0, uint64_t* dst1, int accumulate, void* stream) {
    if (log_domain > 32) return bj::set_error(BJ_EINVAL, "log_domain exceeds the 2-adicity (32) of the field");
    const size_t domain = (size_t)1 << log_domain;
    if (n_rows > domain || row0 > domain - n_rows)
        return bj::set_error(BJ_EINVAL, "bj_deep_quotient_d: row0 + n_rows exceeds 2^log_domain");
    if (n_rows == 0) return BJ_OK;
    if (!dst0 || !dst1) return bj::set_error(BJ_EINVAL, "bj_deep_quotient_d: null dst");
    if (n_cols && (!cols || !gammas)) return bj::set_error(BJ_EINVAL, "bj_deep_quotient_d: null cols or gammas");
    if (n_cols && col_stride < n_rows) return bj::set_error(BJ_EINVAL, "bj_deep_quotient_d: col_stride < n_rows");
    const hipError_t e = bj::launch_deep_quotient(cols, n_cols, col_stride, gammas, k0, k1, at0, at1, log_domain, row0,
                                                  n_rows, dst0, dst1, accumulate, bj::S(stream));
    return bj::ok_or(e, "deep quotient");
}

int bj_deep_codeword_d(const bj_deep_codeword_t* desc, void* stream) {
    if (!desc) return bj::set_error(BJ_EINVAL, "bj_deep_codeword_d: null descriptor");
    if (const char* why = bj::bad_codeword(*desc)) return bj::set_error(BJ_EINVAL, why);
    if (desc->n_rows == 0) return BJ_OK;
    if (const char* why = bj::bad_codeword_pointers(*desc)) return bj::set_error(BJ_EINVAL, why);
    return bj::ok_or(bj::launch_deep_codeword(*desc, bj::S(stream)), "deep codeword");
}

}  // extern "C"
