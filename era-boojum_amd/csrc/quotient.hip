// Quotient: the copy-permutation and lookup terms over the LDE domain, the division by the
// vanishing polynomial, on columns that stay on the device (prover.rs:1111-1467 without the gate
// terms, which depend on the circuit and enter as the accumulator's initial contents).
//
// * bj_quotient_copy_permutation_d: the (z(x) - 1) L_1(x) term (prover.rs:1148-1227 over
//   unnormalized_l1_inverse, utils.rs:1585-1665) and compute_quotient_terms_in_extension
//   (cs/implementations/copy_permutation.rs:1000-1249), all relations in one pass over the rows.
// * bj_quotient_lookup_term_d: dst += alpha (E (beta + sum_t g_t src_t) - f), the one operation
//   behind both loops of compute_quotient_terms_for_lookup_specialized
//   (lookup_argument_in_ext.rs:949-1310).
// * bj_quotient_divide_vanishing_d: divide_by_vanishing_for_bitreversed_coset_enumeration
//   (utils.rs:770-817); bj_vanishing_inverses_h: its q per-coset constants, host only.
//
// The domain is the library's (deep.hip): leaf order L = coset * n + row over the first q cosets of
// bj_lde_d's output, x_L = 7 w_{nq}^(bitrev_{log nq}(L)).  A source column's value at point L is
// column[L]: the first q cosets of a D-LDE, D >= q, are the q-LDE (subset_for_degree,
// lde.rs:298-308).
//
// Copy permutation.  A thread owns QP_ROWS points, QP_THREADS apart, so every load is contiguous
// over the wave.  It walks the relations j = 0 .. m - 1 with the running pair
//   D = lhs_j prod_c (w_c + beta sigma_c + gamma),   N = rhs_j prod_c (w_c + beta k_c x + gamma)
// and adds alpha_{j+1} (D - N) to an accumulator in registers; p_j is loaded once, as lhs of
// relation j and rhs of relation j + 1, beta x is computed once per row, and dst is read and
// written once.  lhs_{m-1} = z(w x) is read in place at row bitrev(bitrev(row) + 1 mod n) of the
// same coset (the reference clones the column: shift_by_omega_assuming_bitreversed,
// utils.rs:1245-1271).  1 / (x - 1) of the L_1 term: one base inversion of the product over the
// thread's rows.  The non-residues, the alphas, the powers of w_{nq} and the per-coset x^n - 1
// travel by value in the kernel arguments, QP_KCAP columns and QP_RCAP relations per launch; a
// wider trace takes several launches that meet on chunk boundaries, and only the first adds the
// L_1 term.
//
// Field arithmetic is exact, so any order of operations gives the reference's bits once the
// outputs are canonical.
#include <hip/hip_runtime.h>
#include "gl.hpp"
#include "gl_asm.hpp"
#include "ext2.hpp"
#include "stage_host.hpp"

namespace bj {

namespace {

using namespace ext2;

constexpr uint32_t QP_ROWS = 2;      // points of a thread, sharing one inversion
constexpr uint32_t QP_THREADS = 256;
constexpr uint32_t QP_TILE = QP_ROWS * QP_THREADS;
constexpr uint32_t QP_KCAP = 128;    // columns of one launch
constexpr uint32_t QP_RCAP = 64;     // relations of one launch
constexpr uint32_t Q_MAX = BJ_QUOTIENT_MAX_DEGREE;
constexpr uint32_t LT_THREADS = 256;
static_assert(Q_MAX <= QP_KCAP, "a launch holds at least one whole chunk");

struct QpConsts {
    uint64_t k[QP_KCAP];       // non-residues of the launch's columns, canonical
    E2 alpha[QP_RCAP + 1];     // [0]: the L_1 term's (first launch); [1 + r]: relation j0 + r
    uint64_t wpow[32];         // w_{nq}^(2^b)
    uint64_t xn1[Q_MAX];       // x^n - 1 on coset i: 7^n w_q^(bitrev(i)) - 1
};
static_assert(sizeof(QpConsts) <= 3600, "the kernel arguments hold 4096 bytes");

// 7 w_{nq}^(bitrev(L))
__device__ __forceinline__ uint64_t point(const uint64_t (&wpow)[32], uint32_t L, uint32_t log_d) {
    const uint32_t e = gl::bitrev32(L, log_d);
    uint64_t x = gl::GENERATOR;
    for (uint32_t b = 0; b < log_d; b++) x = gl::mul(x, (e >> b) & 1 ? wpow[b] : 1);
    return x;
}

// ------------------------------------------------------------------ copy permutation
// Relations [j0, j1) of m; s2 is bj_copy_permutation_d's output after its LDE: pair t = columns
// 2 t, 2 t + 1, pair 0 = z, pair t = p_{t-1}, so rhs_j is pair j and lhs_j pair j + 1 (z shifted
// for j = m - 1).
__global__ __launch_bounds__(QP_THREADS) void quotient_cp_kernel(
    const uint64_t* __restrict__ vars, size_t vars_stride, const uint64_t* __restrict__ sigmas, size_t sigmas_stride,
    const uint64_t* __restrict__ s2, size_t s2_stride, uint32_t n_cols, uint32_t m, uint32_t j0, uint32_t j1,
    uint32_t log_n, uint32_t log_q, E2 beta, E2 gamma, QpConsts k, uint64_t* __restrict__ dst0,
    uint64_t* __restrict__ dst1) {
    const uint32_t log_d = log_n + log_q;
    const size_t total = (size_t)1 << log_d;
    const size_t base = blockIdx.x * (size_t)QP_TILE + threadIdx.x;
    size_t L[QP_ROWS];
    bool in[QP_ROWS];
    E2 bx[QP_ROWS], acc[QP_ROWS], prev[QP_ROWS];
    uint64_t x[QP_ROWS];
#pragma unroll
    for (uint32_t r = 0; r < QP_ROWS; r++) {
        const size_t l = base + r * QP_THREADS;
        in[r] = l < total;
        L[r] = in[r] ? l : 0;  // a lane past the end reads point 0 and writes nothing
        x[r] = point(k.wpow, (uint32_t)L[r], log_d);
        bx[r] = {gl::mul(beta.c0, x[r]), gl::mul(beta.c1, x[r])};
        prev[r] = {s2[(size_t)(2 * j0) * s2_stride + L[r]], s2[(size_t)(2 * j0 + 1) * s2_stride + L[r]]};
        acc[r] = {0, 0};
    }
    if (j0 == 0) {  // alpha_0 (z - 1) (x^n - 1) / (x - 1); x != 1 on the coset 7 <w>
        uint64_t d[QP_ROWS];
#pragma unroll
        for (uint32_t r = 0; r < QP_ROWS; r++) d[r] = in[r] ? gl::sub(x[r], 1) : 1;
        static_assert(QP_ROWS == 2, "the shared inversion is written for two rows");
        const uint64_t inv = inv_chain(gl::mul(d[0], d[1]));
#pragma unroll
        for (uint32_t r = 0; r < QP_ROWS; r++) {
            const uint64_t l1 = gl::mul(k.xn1[L[r] >> log_n], gl::mul(inv, d[1 - r]));
            const E2 t = {gl::mul(gl::sub(prev[r].c0, 1), l1), gl::mul(prev[r].c1, l1)};
            acc[r] = mul(k.alpha[0], t);
        }
    }
    const size_t n_mask = ((size_t)1 << log_n) - 1;
    for (uint32_t j = j0; j < j1; j++) {
        E2 lhs[QP_ROWS], dp[QP_ROWS], np[QP_ROWS];
#pragma unroll
        for (uint32_t r = 0; r < QP_ROWS; r++) {
            if (j + 1 < m) {
                lhs[r] = {s2[(size_t)(2 * j + 2) * s2_stride + L[r]], s2[(size_t)(2 * j + 3) * s2_stride + L[r]]};
            } else {  // z(w x): the next row in natural order, same coset
                const uint32_t row = (uint32_t)(L[r] & n_mask);
                const uint32_t next = gl::bitrev32((gl::bitrev32(row, log_n) + 1) & (uint32_t)n_mask, log_n);
                const size_t ls = (L[r] & ~n_mask) | next;
                lhs[r] = {s2[ls], s2[s2_stride + ls]};
            }
            dp[r] = lhs[r];
            np[r] = prev[r];
        }
        const uint32_t first = j << log_q;
        const uint32_t stop = (j + 1) << log_q;
        const uint32_t end = stop < n_cols ? stop : n_cols;
        for (uint32_t c = first; c < end; c++) {
            const uint64_t kc = k.k[c - (j0 << log_q)];
#pragma unroll
            for (uint32_t r = 0; r < QP_ROWS; r++) {
                const uint64_t w = vars[(size_t)c * vars_stride + L[r]];
                const uint64_t s = sigmas[(size_t)c * sigmas_stride + L[r]];
                const uint64_t wg = gl::add(w, gamma.c0);
                // k_c (beta x) and beta sigma: the multipliers k_c and beta are wave-uniform
                uint32_t zl[4], zh[4];
                glasm::mul_sb_x4(lo32(bx[r].c0), hi32(bx[r].c0), lo32(kc), hi32(kc), zl[0], zh[0], lo32(bx[r].c1),
                                 hi32(bx[r].c1), lo32(kc), hi32(kc), zl[1], zh[1], lo32(s), hi32(s), lo32(beta.c0),
                                 hi32(beta.c0), zl[2], zh[2], lo32(s), hi32(s), lo32(beta.c1), hi32(beta.c1), zl[3],
                                 zh[3]);
                const E2 num = {gl::add(wg, u64_of(zl[0], zh[0])), gl::add(gamma.c1, u64_of(zl[1], zh[1]))};
                const E2 den = {gl::add(wg, u64_of(zl[2], zh[2])), gl::add(gamma.c1, u64_of(zl[3], zh[3]))};
                np[r] = mul_x4(np[r], num);
                dp[r] = mul_x4(dp[r], den);
            }
        }
        const E2 a = k.alpha[1 + j - j0];
#pragma unroll
        for (uint32_t r = 0; r < QP_ROWS; r++) {
            const E2 t = mul(a, E2{gl::sub(dp[r].c0, np[r].c0), gl::sub(dp[r].c1, np[r].c1)});
            acc[r] = {gl::add(acc[r].c0, t.c0), gl::add(acc[r].c1, t.c1)};
            prev[r] = lhs[r];
        }
    }
#pragma unroll
    for (uint32_t r = 0; r < QP_ROWS; r++) {
        if (in[r]) {
            dst0[L[r]] = gl::canon(gl::add(acc[r].c0, dst0[L[r]]));
            dst1[L[r]] = gl::canon(gl::add(acc[r].c1, dst1[L[r]]));
        }
    }
}

// ------------------------------------------------------------------ lookup term
struct LtConsts : LookupSources {};  // a type of this file's, so the kernel keeps its name

// One point per thread: dst += alpha (E (beta + sum_t g_t src_t) - f), f = 1 when NULL.
__global__ __launch_bounds__(LT_THREADS) void quotient_lookup_kernel(LtConsts k, uint32_t n_src, E2 beta,
                                                                     const uint64_t* __restrict__ e0,
                                                                     const uint64_t* __restrict__ e1,
                                                                     const uint64_t* __restrict__ f, E2 alpha,
                                                                     size_t total, uint64_t* __restrict__ dst0,
                                                                     uint64_t* __restrict__ dst1) {
    const size_t i = blockIdx.x * (size_t)LT_THREADS + threadIdx.x;
    if (i >= total) return;
    E2 d = beta;
    for (uint32_t t = 0; t < n_src; t++) {
        const uint64_t v = k.src[t][i];
        d = {gl::add(d.c0, gl::mul(v, k.g[2 * t])), gl::add(d.c1, gl::mul(v, k.g[2 * t + 1]))};
    }
    E2 v = mul(E2{e0[i], e1[i]}, d);
    v.c0 = gl::sub(v.c0, f ? f[i] : 1);
    v = mul(alpha, v);
    dst0[i] = gl::canon(gl::add(v.c0, dst0[i]));
    dst1[i] = gl::canon(gl::add(v.c1, dst1[i]));
}

// ------------------------------------------------------------------ division by the vanishing polynomial
struct DvConsts {
    uint64_t inv[Q_MAX];  // 1 / (x^n - 1) on coset i, canonical
};

__global__ __launch_bounds__(256) void quotient_divide_kernel(DvConsts k, uint32_t log_n, size_t total,
                                                              uint64_t* __restrict__ dst0,
                                                              uint64_t* __restrict__ dst1) {
    const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
    if (i >= total) return;
    const uint64_t v = k.inv[i >> log_n];
    dst0[i] = gl::canon(gl::mul(dst0[i], v));
    dst1[i] = gl::canon(gl::mul(dst1[i], v));
}

// ------------------------------------------------------------------ host constants and launchers
// x^n - 1 on coset i of the q-LDE: 7^n w_{nq}^(n bitrev_{log q}(i)) - 1, canonical
void vanishing_on_cosets(uint32_t log_n, uint32_t log_q, uint64_t* out) {
    uint64_t g = gl::GENERATOR;
    for (uint32_t b = 0; b < log_n; b++) g = gl::mul(g, g);
    const uint64_t wq = gl::domain_generator(log_q);  // w_{nq}^n
    const size_t q = (size_t)1 << log_q;
    for (size_t i = 0; i < q; i++)
        out[i] = gl::canon(gl::sub(gl::mul(g, gl::pow(wq, gl::bitrev32((uint32_t)i, log_q))), 1));
}

hipError_t launch_quotient_cp(const uint64_t* vars, size_t vars_stride, const uint64_t* sigmas, size_t sigmas_stride,
                              const uint64_t* s2, size_t s2_stride, uint32_t n_cols, uint32_t log_n, uint32_t log_q,
                              const uint64_t* non_residues, E2 beta, E2 gamma, const uint64_t* alphas, uint64_t* dst0,
                              uint64_t* dst1, hipStream_t st) {
    const uint32_t log_d = log_n + log_q;
    const size_t total = (size_t)1 << log_d;
    const uint32_t m = (uint32_t)(((uint64_t)n_cols + ((uint64_t)1 << log_q) - 1) >> log_q);
    QpConsts k;
    fill_wpow(k.wpow, log_d);
    for (uint32_t i = 0; i < Q_MAX; i++) k.xn1[i] = 0;
    vanishing_on_cosets(log_n, log_q, k.xn1);
    k.alpha[0] = canon2(alphas[0], alphas[1]);
    // whole chunks per launch: at most QP_KCAP columns and QP_RCAP relations
    uint32_t per = QP_KCAP >> log_q;
    if (per > QP_RCAP) per = QP_RCAP;
    const size_t blocks = (total + QP_TILE - 1) / QP_TILE;
    for (uint32_t j0 = 0; j0 < m; j0 += per) {
        const uint32_t j1 = m - j0 < per ? m : j0 + per;
        const uint32_t c0 = j0 << log_q;
        for (uint32_t c = 0; c < QP_KCAP; c++) k.k[c] = c0 + c < n_cols ? gl::canon(non_residues[c0 + c]) : 0;
        for (uint32_t r = 0; r < QP_RCAP; r++) {
            const uint32_t j = j0 + r;
            k.alpha[1 + r] = j < j1 ? canon2(alphas[2 * (j + 1)], alphas[2 * (j + 1) + 1]) : E2{0, 0};
        }
        hipLaunchKernelGGL(quotient_cp_kernel, dim3((unsigned)blocks), dim3(QP_THREADS), 0, st, vars, vars_stride,
                           sigmas, sigmas_stride, s2, s2_stride, n_cols, m, j0, j1, log_n, log_q, beta, gamma, k, dst0,
                           dst1);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

// the checks every device entry point of the quotient shares; NULL when the sizes are fine
const char* bad_quotient_domain(uint32_t log_n, uint32_t log_q) {
    if (const char* why = bad_domain(log_n, log_q)) return why;
    if (((uint64_t)1 << log_q) > Q_MAX) return "the quotient degree exceeds BJ_QUOTIENT_MAX_DEGREE";
    return nullptr;
}

}  // namespace

}  // namespace bj

extern "C" {

int bj_quotient_copy_permutation_d(const uint64_t* vars, size_t vars_stride, const uint64_t* sigmas,
                                   size_t sigmas_stride, const uint64_t* stage2, size_t stage2_stride, uint32_t n_cols,
                                   uint32_t log_n, uint32_t log_q, const uint64_t* non_residues, uint64_t beta0,
                                   uint64_t beta1, uint64_t gamma0, uint64_t gamma1, const uint64_t* alphas,
                                   uint64_t* dst0, uint64_t* dst1, void* stream) {
    if (const char* why = bj::bad_quotient_domain(log_n, log_q)) return bj::set_error(BJ_EINVAL, why);
    if (n_cols == 0) return bj::set_error(BJ_EINVAL, "bj_quotient_copy_permutation_d: n_cols must be positive");
    if (!vars || !sigmas || !stage2 || !non_residues || !alphas || !dst0 || !dst1)
        return bj::set_error(BJ_EINVAL, "bj_quotient_copy_permutation_d: null pointer");
    const size_t total = (size_t)1 << (log_n + log_q);
    if (vars_stride < total || sigmas_stride < total || stage2_stride < total)
        return bj::set_error(BJ_EINVAL, "bj_quotient_copy_permutation_d: a column stride is below 2^(log_n + log_q)");
    const hipError_t e = bj::launch_quotient_cp(vars, vars_stride, sigmas, sigmas_stride, stage2, stage2_stride, n_cols,
                                                log_n, log_q, non_residues, bj::ext2::canon2(beta0, beta1),
                                                bj::ext2::canon2(gamma0, gamma1), alphas, dst0, dst1,
                                                bj::S(stream));
    return bj::ok_or(e, "quotient copy permutation");
}

int bj_quotient_lookup_term_d(const uint64_t* const* srcs, uint32_t n_src, const uint64_t* g, uint64_t beta0,
                              uint64_t beta1, const uint64_t* e_c0, const uint64_t* e_c1, const uint64_t* f,
                              uint64_t alpha0, uint64_t alpha1, uint32_t log_n, uint32_t log_q, uint64_t* dst0,
                              uint64_t* dst1, void* stream) {
    if (const char* why = bj::bad_quotient_domain(log_n, log_q)) return bj::set_error(BJ_EINVAL, why);
    if (n_src == 0 || n_src > bj::LOOKUP_MAX_SRC)
        return bj::set_error(BJ_EINVAL, "bj_quotient_lookup_term_d: n_src must be 1..16");
    if (!srcs || !g || !e_c0 || !e_c1 || !dst0 || !dst1)
        return bj::set_error(BJ_EINVAL, "bj_quotient_lookup_term_d: null pointer");
    bj::LtConsts k;
    if (!bj::fill_lookup_sources(k, srcs, n_src, g))
        return bj::set_error(BJ_EINVAL, "bj_quotient_lookup_term_d: null source column");
    const size_t total = (size_t)1 << (log_n + log_q);
    hipLaunchKernelGGL(bj::quotient_lookup_kernel, dim3((unsigned)((total + bj::LT_THREADS - 1) / bj::LT_THREADS)),
                       dim3(bj::LT_THREADS), 0, bj::S(stream), k, n_src, bj::ext2::canon2(beta0, beta1), e_c0,
                       e_c1, f, bj::ext2::canon2(alpha0, alpha1), total, dst0, dst1);
    return bj::ok_or(hipGetLastError(), "quotient lookup term");
}

int bj_vanishing_inverses_h(uint32_t log_n, uint32_t log_q, uint64_t* out) {
    if (const char* why = bj::bad_domain(log_n, log_q)) return bj::set_error(BJ_EINVAL, why);
    if (!out) return bj::set_error(BJ_EINVAL, "bj_vanishing_inverses_h: null out");
    // 7 generates the whole multiplicative group and nq < p - 1, so 7^n w_q^k is never 1
    const uint64_t wq = gl::domain_generator(log_q);
    uint64_t g = gl::GENERATOR;
    for (uint32_t b = 0; b < log_n; b++) g = gl::mul(g, g);
    const uint64_t q = (uint64_t)1 << log_q;
    for (uint64_t i = 0; i < q; i++)
        out[i] = gl::canon(gl::inv(gl::sub(gl::mul(g, gl::pow(wq, gl::bitrev32((uint32_t)i, log_q))), 1)));
    return BJ_OK;
}

int bj_quotient_divide_vanishing_d(uint64_t* dst0, uint64_t* dst1, uint32_t log_n, uint32_t log_q, void* stream) {
    if (const char* why = bj::bad_quotient_domain(log_n, log_q)) return bj::set_error(BJ_EINVAL, why);
    if (!dst0 || !dst1) return bj::set_error(BJ_EINVAL, "bj_quotient_divide_vanishing_d: null pointer");
    bj::DvConsts k;
    for (uint32_t i = 0; i < bj::Q_MAX; i++) k.inv[i] = 0;
    if (const int rc = bj_vanishing_inverses_h(log_n, log_q, k.inv)) return rc;
    const size_t total = (size_t)1 << (log_n + log_q);
    hipLaunchKernelGGL(bj::quotient_divide_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       bj::S(stream), k, log_n, total, dst0, dst1);
    return bj::ok_or(hipGetLastError(), "quotient divide by vanishing");
}

}  // extern "C"
