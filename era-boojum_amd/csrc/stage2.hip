// Stage 2: the copy-permutation grand product z(x) with its partial products, and the lookup
// argument's encoding polynomials, on columns that stay on the device.
//
// * bj_copy_permutation_d: compute_partial_products_in_extension
//   (cs/implementations/copy_permutation.rs:649-774; pointwise_rational_in_extension :114-248,
//   pointwise_product_in_extension :298-365, shifted_grand_product_in_extension :425-510), called
//   at prover.rs:360-392, over the main domain in natural order: x_i = w_n^i (utils.rs:690-721).
// * bj_lookup_encoding_d: out = f / (beta + sum_t g_t src_t), the one operation behind both
//   families of compute_lookup_poly_pairs_specialized (lookup_argument_in_ext.rs:320-700).
// * bj_non_residues_h: non_residues_for_copy_permutation (copy_permutation.rs:512-522) over
//   make_non_residues (utils.rs:636-688), host only.
//
// Copy permutation, three kernels on one stream and nothing but kernel boundaries between them:
//   1. rational: a thread owns a row and walks the columns.  With N_j, D_j the numerator and
//      denominator products of chunk j it keeps the prefix products PN_j = N_0..N_j and
//      PD_j = D_0..D_j, and what it needs is the prefix rational R_j = PN_j / PD_j: the
//      intermediate p_j is z R_j and the row's factor a is R_{m-1}.  One base-field inversion
//      (norm of PD, conj / norm) serves a group of up to CP_MP chunks: 1 / PD_j = (1 / PD_last) D_last..D_{j+1},
//      walked backwards with the D_j in LDS and PN_j parked in the output slot R_j goes to.
//      Its last launch also scans a over the block's CP_TILE rows: the z slot receives the
//      exclusive prefix within the tile, and the tile's first row (whose prefix is 1) the tile total.
//   2. totals: one workgroup turns the tile totals into their exclusive prefix in place, which is
//      z at each tile's first row, and writes the product over all rows to the status record.
//   3. apply: z = (tile prefix) (prefix within the tile), p_j = z R_j in place, canonical.
// The outputs are the working set; there is no scratch.  The non-residues travel by value in the
// kernel arguments, CP_KCAP columns per launch; a wider trace takes several rational launches
// that carry the running prefix rational in the z slot.
//
// Field arithmetic is exact, so any order of operations gives the reference's bits once the
// outputs are canonical.
#include <hip/hip_runtime.h>
#include <vector>
#include "gl.hpp"
#include "gl_asm.hpp"
#include "ext2.hpp"
#include "stage_host.hpp"

namespace bj {

namespace {

using namespace ext2;

constexpr uint32_t CP_TILE = 128;   // rows of one block of the rational pass: the scan's tile
constexpr uint32_t CP_KCAP = 256;   // columns of one rational launch
constexpr uint32_t CP_MP = 16;      // chunks that share one inversion, at most (16 bytes of LDS per row each)
constexpr uint32_t TOTALS_THREADS = 256;
constexpr uint32_t LK_ROWS = 4;     // rows of a thread, sharing one inversion
constexpr uint32_t LK_THREADS = 256;
constexpr uint32_t LK_TILE = LK_ROWS * LK_THREADS;

constexpr E2 ONE = {1, 0};

struct CpConsts {
    uint64_t k[CP_KCAP];  // non-residues of the launch's columns, canonical
    uint64_t wpow[32];    // w_n^(2^b)
};

// lo32, hi32, u64_of and the column walk's product mul_x4 are ext2.hpp's

__device__ __forceinline__ E2 shfl_up(E2 v, int d) {
    return {(uint64_t)__shfl_up((unsigned long long)v.c0, d, 64), (uint64_t)__shfl_up((unsigned long long)v.c1, d, 64)};
}

// Exclusive prefix product of v over the block's threads (WAVES waves of 64) and the block's
// product.  Every thread of the block calls it; ws holds WAVES elements.
template <uint32_t WAVES>
__device__ __forceinline__ E2 block_exclusive_product(E2 v, E2* ws, E2& total) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const E2 t = shfl_up(v, d);
        if (lane >= (uint32_t)d) v = mul(t, v);
    }
    if (lane == 63) ws[wave] = v;
    E2 ex = shfl_up(v, 1);
    if (lane == 0) ex = ONE;
    __syncthreads();
    E2 before = ONE;
    total = ONE;
#pragma unroll
    for (uint32_t w = 0; w < WAVES; w++) {
        if (w == wave) before = total;
        total = mul(total, ws[w]);
    }
    return mul(before, ex);
}

// ------------------------------------------------------------------ 1. rational
// Columns [c0, c1) of the trace, c1 - c0 <= CP_KCAP.  `first`: the running prefix rational
// starts at 1, otherwise at what the previous launch left in the z slot.  `last`: the tile scan.
// A chunk whose denominator product is zero counts once into status[2] and contributes the
// factor 0 (numerator 0 over denominator 1), so the shared inversion never sees a zero.
__global__ __launch_bounds__(CP_TILE) void cp_rational_kernel(
    const uint64_t* __restrict__ vars, size_t vars_stride, const uint64_t* __restrict__ sigmas, size_t sigmas_stride,
    uint32_t c0, uint32_t c1, uint32_t n_cols, uint32_t log_q, uint32_t group, uint32_t log_n, E2 beta, E2 gamma,
    CpConsts k, uint64_t* __restrict__ out, size_t out_stride, int first, int last,
    unsigned long long* __restrict__ status) {
    __shared__ E2 ws[CP_TILE / 64];
    extern __shared__ E2 den[];  // [group][CP_TILE]: the denominators of the group's pieces
    const size_t n = (size_t)1 << log_n;
    const size_t i = blockIdx.x * (size_t)CP_TILE + threadIdx.x;
    const bool active = i < n;
    const size_t row = active ? i : 0;  // a lane past the end reads row 0 and writes nothing
    uint64_t x = 1;
    for (uint32_t b = 0; b < log_n; b++) x = gl::mul(x, (row >> b) & 1 ? k.wpow[b] : 1);
    const uint64_t bx0 = gl::mul(beta.c0, x), bx1 = gl::mul(beta.c1, x);
    uint64_t* z0 = out;
    uint64_t* z1 = out + out_stride;
    const uint32_t q = 1u << log_q;
    E2 run = ONE;  // the prefix rational through every column before c
    if (!first) run = {z0[row], z1[row]};
    uint32_t zeros = 0;
    uint32_t c = c0;
    while (c < c1) {
        const uint32_t chunk0 = c >> log_q;  // piece t of this group ends with chunk chunk0 + t (or at c1)
        E2 pn = run, pd = ONE;
        uint32_t pieces = 0;
        for (uint32_t t = 0; t < group && c < c1; t++) {
            {
                const uint32_t stop = (chunk0 + t + 1) << log_q;
                const uint32_t end = stop < c1 ? stop : c1;
                E2 nj = ONE, dj = ONE;
                for (; c < end; c++) {
                    const uint64_t w = vars[(size_t)c * vars_stride + row];
                    const uint64_t s = sigmas[(size_t)c * sigmas_stride + row];
                    const uint64_t kc = k.k[c - c0];
                    const uint64_t wg = gl::add(w, gamma.c0);
                    // k_c (beta x) and beta sigma: the multipliers k_c and beta are wave-uniform
                    uint32_t zl[4], zh[4];
                    glasm::mul_sb_x4(lo32(bx0), hi32(bx0), lo32(kc), hi32(kc), zl[0], zh[0], lo32(bx1), hi32(bx1),
                                     lo32(kc), hi32(kc), zl[1], zh[1], lo32(s), hi32(s), lo32(beta.c0), hi32(beta.c0),
                                     zl[2], zh[2], lo32(s), hi32(s), lo32(beta.c1), hi32(beta.c1), zl[3], zh[3]);
                    const E2 num = {gl::add(wg, u64_of(zl[0], zh[0])), gl::add(gamma.c1, u64_of(zl[1], zh[1]))};
                    const E2 dn = {gl::add(wg, u64_of(zl[2], zh[2])), gl::add(gamma.c1, u64_of(zl[3], zh[3]))};
                    nj = mul_x4(nj, num);
                    dj = mul_x4(dj, dn);
                }
                if (is_zero(dj)) {
                    zeros += active;
                    nj = {0, 0};
                    dj = ONE;
                }
                den[t * CP_TILE + threadIdx.x] = dj;
                pn = mul(pn, nj);
                pd = mul(pd, dj);
                // a piece that more columns follow ends a chunk j <= m - 2: park PN_j in slot j
                if (end < n_cols && (end & (q - 1)) == 0 && active) {
                    uint64_t* slot = out + (size_t)(2 * (chunk0 + t + 1)) * out_stride;
                    slot[row] = pn.c0;
                    slot[out_stride + row] = pn.c1;
                }
                pieces = t + 1;
            }
        }
        const uint64_t ninv = inv_chain(norm(pd));
        E2 s = {gl::mul(pd.c0, ninv), gl::mul(neg(pd.c1), ninv)};  // 1 / PD of the group's last piece
        for (uint32_t tt = pieces; tt-- > 0;) {
            {
                const uint32_t stop = (chunk0 + tt + 1) << log_q;
                const uint32_t end = stop < c1 ? stop : c1;
                const bool slotted = end < n_cols && (end & (q - 1)) == 0;
                uint64_t* slot = out + (size_t)(2 * (chunk0 + tt + 1)) * out_stride;
                E2 r;
                if (tt + 1 == pieces) {
                    r = mul(pn, s);
                    run = r;
                } else {  // not the group's last piece, so it ended a chunk and PN_j is in its slot
                    r = mul(E2{slot[row], slot[out_stride + row]}, s);
                }
                if (slotted && active) {
                    slot[row] = r.c0;
                    slot[out_stride + row] = r.c1;
                }
                s = mul(s, den[tt * CP_TILE + threadIdx.x]);
            }
        }
    }
    if (zeros) atomicAdd(&status[2], (unsigned long long)zeros);
    if (!last) {
        if (active) {
            z0[i] = run.c0;
            z1[i] = run.c1;
        }
        return;
    }
    E2 total;
    const E2 ex = block_exclusive_product<CP_TILE / 64>(active ? run : ONE, ws, total);
    if (active) {
        const E2 v = threadIdx.x == 0 ? total : ex;
        z0[i] = v.c0;
        z1[i] = v.c1;
    }
}

// ------------------------------------------------------------------ 2. tile totals
// One workgroup.  Tile b's total sits at row b * CP_TILE of the z slot and is replaced by the
// product of the totals before it: a thread multiplies its run of per consecutive tiles, the
// block scans the runs' products, and the thread walks its run again.
__global__ __launch_bounds__(TOTALS_THREADS) void cp_totals_kernel(uint64_t* __restrict__ z0, uint64_t* __restrict__ z1,
                                                                   size_t n_tiles, size_t per,
                                                                   unsigned long long* __restrict__ status) {
    __shared__ E2 ws[TOTALS_THREADS / 64];
    const size_t b0 = threadIdx.x * per < n_tiles ? threadIdx.x * per : n_tiles;
    const size_t b1 = b0 + per < n_tiles ? b0 + per : n_tiles;
    E2 p = ONE;
    for (size_t b = b0; b < b1; b++) p = mul(p, E2{z0[b * CP_TILE], z1[b * CP_TILE]});
    E2 total;
    E2 e = block_exclusive_product<TOTALS_THREADS / 64>(p, ws, total);
    for (size_t b = b0; b < b1; b++) {
        const E2 t = {z0[b * CP_TILE], z1[b * CP_TILE]};
        z0[b * CP_TILE] = gl::canon(e.c0);
        z1[b * CP_TILE] = gl::canon(e.c1);
        e = mul(e, t);
    }
    if (threadIdx.x == 0) {
        status[0] = gl::canon(total.c0);
        status[1] = gl::canon(total.c1);
    }
}

// ------------------------------------------------------------------ 3. apply
// z_i = z[tile's first row] * (prefix within the tile); the tile's first row is final already and
// nobody writes it here, so its readers race with no one.  Then p_j = z_i R_j for j < m - 1.
__global__ __launch_bounds__(256) void cp_apply_kernel(uint64_t* __restrict__ out, size_t out_stride, uint32_t m,
                                                       size_t n) {
    const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
    if (i >= n) return;
    uint64_t* z0 = out;
    uint64_t* z1 = out + out_stride;
    const size_t head = i & ~(size_t)(CP_TILE - 1);
    E2 z = {z0[head], z1[head]};
    if (i != head) {
        z = mul(z, E2{z0[i], z1[i]});
        z0[i] = gl::canon(z.c0);
        z1[i] = gl::canon(z.c1);
    }
    for (uint32_t j = 0; j + 1 < m; j++) {
        uint64_t* s0 = out + (size_t)(2 * j + 2) * out_stride;
        uint64_t* s1 = s0 + out_stride;
        const E2 p = mul(z, E2{s0[i], s1[i]});
        s0[i] = gl::canon(p.c0);
        s1[i] = gl::canon(p.c1);
    }
}

// ------------------------------------------------------------------ lookup encodings
struct LkConsts : LookupSources {};  // a type of this file's, so the kernel keeps its name

// A thread owns rows base + r * LK_THREADS, r < LK_ROWS, so every load and store is contiguous over
// the wave; the rows' Ext2 inverses share one base inversion of the product of their norms.  A
// zero denominator counts into status[2] and gives 0; a row past the end enters as norm 1.
__global__ __launch_bounds__(LK_THREADS) void lookup_encoding_kernel(LkConsts k, uint32_t n_src, E2 beta,
                                                                     const uint64_t* __restrict__ f, size_t n,
                                                                     uint64_t* __restrict__ o0, uint64_t* __restrict__ o1,
                                                                     unsigned long long* __restrict__ status) {
    const size_t base = blockIdx.x * (size_t)LK_TILE + threadIdx.x;
    E2 d[LK_ROWS];
#pragma unroll
    for (uint32_t r = 0; r < LK_ROWS; r++) d[r] = beta;
    for (uint32_t t = 0; t < n_src; t++) {
        const uint64_t* __restrict__ src = k.src[t];
        const uint64_t g0 = k.g[2 * t], g1 = k.g[2 * t + 1];
#pragma unroll
        for (uint32_t r = 0; r < LK_ROWS; r++) {
            const size_t i = base + r * LK_THREADS;
            const uint64_t v = i < n ? src[i] : 0;
            d[r] = {gl::add(d[r].c0, gl::mul(v, g0)), gl::add(d[r].c1, gl::mul(v, g1))};
        }
    }
    uint64_t nr[LK_ROWS], pre[LK_ROWS];
    uint32_t zeros = 0;
#pragma unroll
    for (uint32_t r = 0; r < LK_ROWS; r++) {
        const bool in = base + r * LK_THREADS < n;
        nr[r] = gl::canon(norm(d[r]));
        if (nr[r] == 0 || !in) {  // the norm is zero only for d = 0: 7 is no square
            zeros += in;
            nr[r] = 1;
            d[r] = {0, 0};
        }
        pre[r] = r ? gl::mul(pre[r - 1], nr[r]) : nr[r];
    }
    uint64_t inv = inv_chain(pre[LK_ROWS - 1]);
#pragma unroll
    for (uint32_t r = LK_ROWS; r-- > 0;) {
        const size_t i = base + r * LK_THREADS;
        const uint64_t ir = r ? gl::mul(inv, pre[r - 1]) : inv;  // 1 / norm of row r
        inv = gl::mul(inv, nr[r]);
        if (i < n) {
            uint64_t e0 = gl::mul(d[r].c0, ir), e1 = gl::mul(neg(d[r].c1), ir);
            if (f) {
                const uint64_t fv = f[i];
                e0 = gl::mul(e0, fv);
                e1 = gl::mul(e1, fv);
            }
            o0[i] = gl::canon(e0);
            o1[i] = gl::canon(e1);
        }
    }
    if (zeros) atomicAdd(&status[2], (unsigned long long)zeros);
}

// ------------------------------------------------------------------ launchers
hipError_t launch_copy_permutation(const uint64_t* vars, size_t vars_stride, const uint64_t* sigmas,
                                   size_t sigmas_stride, uint32_t n_cols, uint32_t log_n, const uint64_t* non_residues,
                                   E2 beta, E2 gamma, uint32_t log_q, uint64_t* out, size_t out_stride,
                                   uint64_t* status, hipStream_t st) {
    const size_t n = (size_t)1 << log_n;
    const size_t n_tiles = (n + CP_TILE - 1) / CP_TILE;
    const uint32_t m = (uint32_t)((((uint64_t)n_cols + ((uint64_t)1 << log_q) - 1)) >> log_q);
    unsigned long long* status_ = reinterpret_cast<unsigned long long*>(status);
    if (hipError_t e = hipMemsetAsync(status, 0, 4 * sizeof(uint64_t), st)) return e;
    // groups of equal size, as few as CP_MP allows (17 chunks: 9 + 8)
    const uint32_t n_groups = (m + CP_MP - 1) / CP_MP;
    const uint32_t group = (m + n_groups - 1) / n_groups;
    CpConsts k;
    fill_wpow(k.wpow, log_n);
    for (uint32_t c0 = 0; c0 < n_cols; c0 += CP_KCAP) {
        const uint32_t c1 = n_cols - c0 < CP_KCAP ? n_cols : c0 + CP_KCAP;
        for (uint32_t c = 0; c < CP_KCAP; c++) k.k[c] = c0 + c < c1 ? gl::canon(non_residues[c0 + c]) : 0;
        hipLaunchKernelGGL(cp_rational_kernel, dim3((unsigned)n_tiles), dim3(CP_TILE),
                           group * CP_TILE * sizeof(E2), st, vars, vars_stride, sigmas, sigmas_stride, c0, c1, n_cols,
                           log_q, group, log_n, beta, gamma, k, out, out_stride, c0 == 0 ? 1 : 0,
                           c1 == n_cols ? 1 : 0, status_);
        if (hipError_t e = hipGetLastError()) return e;
    }
    const size_t per = (n_tiles + TOTALS_THREADS - 1) / TOTALS_THREADS;
    hipLaunchKernelGGL(cp_totals_kernel, dim3(1), dim3(TOTALS_THREADS), 0, st, out, out + out_stride, n_tiles, per,
                       status_);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(cp_apply_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, out, out_stride, m, n);
    return hipGetLastError();
}

}  // namespace

}  // namespace bj

extern "C" {

int bj_copy_permutation_d(const uint64_t* vars, size_t vars_stride, const uint64_t* sigmas, size_t sigmas_stride,
                          uint32_t n_cols, uint32_t log_n, const uint64_t* non_residues, uint64_t beta0, uint64_t beta1,
                          uint64_t gamma0, uint64_t gamma1, uint32_t chunk, uint64_t* out, size_t out_stride,
                          uint64_t* status_d, void* stream) {
    if (const char* why = bj::bad_log_n(log_n)) return bj::set_error(BJ_EINVAL, why);
    if (n_cols == 0) return bj::set_error(BJ_EINVAL, "bj_copy_permutation_d: n_cols must be positive");
    if (chunk == 0 || (chunk & (chunk - 1)))
        return bj::set_error(BJ_EINVAL, "bj_copy_permutation_d: chunk must be a power of two");
    if (!vars || !sigmas || !non_residues || !out || !status_d)
        return bj::set_error(BJ_EINVAL, "bj_copy_permutation_d: null pointer");
    const size_t n = (size_t)1 << log_n;
    if (vars_stride < n || sigmas_stride < n || out_stride < n)
        return bj::set_error(BJ_EINVAL, "bj_copy_permutation_d: a column stride is below 2^log_n");
    const uint32_t log_q = (uint32_t)__builtin_ctz(chunk);
    const hipError_t e = bj::launch_copy_permutation(vars, vars_stride, sigmas, sigmas_stride, n_cols, log_n,
                                                     non_residues, bj::ext2::canon2(beta0, beta1),
                                                     bj::ext2::canon2(gamma0, gamma1), log_q, out, out_stride, status_d,
                                                     bj::S(stream));
    return bj::ok_or(e, "copy permutation");
}

int bj_lookup_encoding_d(const uint64_t* const* srcs, uint32_t n_src, const uint64_t* g, uint64_t beta0, uint64_t beta1,
                         const uint64_t* f, uint32_t log_n, uint64_t* out_c0, uint64_t* out_c1, uint64_t* status_d,
                         void* stream) {
    if (const char* why = bj::bad_log_n(log_n)) return bj::set_error(BJ_EINVAL, why);
    if (n_src == 0 || n_src > bj::LOOKUP_MAX_SRC)
        return bj::set_error(BJ_EINVAL, "bj_lookup_encoding_d: n_src must be 1..16");
    if (!srcs || !g || !out_c0 || !out_c1 || !status_d)
        return bj::set_error(BJ_EINVAL, "bj_lookup_encoding_d: null pointer");
    bj::LkConsts k;
    if (!bj::fill_lookup_sources(k, srcs, n_src, g))
        return bj::set_error(BJ_EINVAL, "bj_lookup_encoding_d: null source column");
    const size_t n = (size_t)1 << log_n;
    hipStream_t st = bj::S(stream);
    hipError_t e = hipMemsetAsync(status_d, 0, 4 * sizeof(uint64_t), st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(bj::lookup_encoding_kernel, dim3((unsigned)((n + bj::LK_TILE - 1) / bj::LK_TILE)),
                           dim3(bj::LK_THREADS), 0, st, k, n_src, bj::ext2::canon2(beta0, beta1), f, n, out_c0, out_c1,
                           reinterpret_cast<unsigned long long*>(status_d));
        e = hipGetLastError();
    }
    return bj::ok_or(e, "lookup encoding");
}

int bj_non_residues_h(uint32_t num, uint32_t log_n, uint64_t* out) {
    if (const char* why = bj::bad_log_n(log_n)) return bj::set_error(BJ_EINVAL, why);
    if (num == 0 || !out) return bj::set_error(BJ_EINVAL, "bj_non_residues_h: num must be positive and out non-null");
    // x^n by log_n squarings
    auto pow_n = [log_n](uint64_t x) {
        for (uint32_t i = 0; i < log_n; i++) x = gl::mul(x, x);
        return gl::canon(x);
    };
    out[0] = 1;
    std::vector<uint64_t> seen;  // k^n of the non-residues found: equal powers mean one coset (utils.rs:651-686)
    uint64_t cur = 1;
    for (uint32_t found = 1; found < num;) {
        cur++;
        if (gl::canon(gl::pow(cur, (gl::P - 1) / 2)) != gl::P - 1) continue;  // not a quadratic non-residue
        const uint64_t t = pow_n(cur);
        if (t == 1) continue;  // in the domain
        bool unique = true;
        for (uint64_t s : seen) unique = unique && s != t;
        if (!unique) continue;
        seen.push_back(t);
        out[found++] = cur;
    }
    return BJ_OK;
}

}  // extern "C"
