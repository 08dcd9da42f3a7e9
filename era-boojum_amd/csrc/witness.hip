// Witness materialisation: the trace columns from a WitnessVec's all_values and the circuit's dense
// copy hints, the multiplicity column, and the sigma columns of the setup -- on columns that are
// born on the device.
//
// * bj_copy_hint_upload_d / _info / _release: a DenseVariablesCopyHint or DenseWitnessCopyHint
//   (cs/implementations/hints/mod.rs:10-20) packed to one u32 per cell and kept on the device.  A
//   Variable / Witness is a u64 with bit 63 the placeholder flag and the index in the low 48 bits
//   (cs/mod.rs:44-47, 159-213); the packed cell is the index, or HINT_PLACEHOLDER.
// * bj_materialize_columns_d: the copy loops of witness_set_from_witness_vec
//   (cs/implementations/witness.rs:419-441, 466-488; the same loops at :108-385):
//   out[c][r] = all_values[index], 0 for a placeholder, words moved bit for bit.
// * bj_materialize_multiplicities_d: the multiplicity column (witness.rs:493-519).
// * bj_permutation_polys_d: create_permutation_polys (setup.rs:401-484) from the map of previous
//   occurrences, over materialize_x_by_non_residue_polys (setup.rs:24-76): the identity value of
//   (col, row) is k_col w_n^row with the rows in natural order (materialize_x_poly,
//   utils.rs:690-721).
//
// The gather is bound by where all_values sits in the cache hierarchy, not by arithmetic.  A lane
// owns a row and WIT_COLS columns of it: the wave reads 64 consecutive packed indices of a column
// in one 256-byte load, a thread issues the gathers of all its columns before it uses the first,
// and the indices and the output go through nontemporal loads and stores, which are read and
// written once, so that all_values keeps the L2 and the Infinity Cache.  Workgroups are numbered
// so that the column tiles of one row block follow each other on one XCD (blocks b and b + 8 are
// observed to share one; a speed choice only, any placement is correct): with a placement that
// fills the trace row by row they read the same stretch of all_values out of that XCD's L2.
//
// No kernel reads outside all_values: the largest index of a hint is recorded at upload and the
// call compares num_values with it on the host, so there is no bound check per lane and no status
// record.
#include <hip/hip_runtime.h>
#include <new>
#include <vector>
#include "gl.hpp"
#include "stage_host.hpp"

// the A/B switches of DESIGN 4.14, compile time only
#ifndef BJ_WIT_DEAL_BY_XCD
#define BJ_WIT_DEAL_BY_XCD 1  // 0: workgroups in column-tile-major order
#endif
#ifndef BJ_WIT_COLS
#define BJ_WIT_COLS 4
#endif

namespace bj {

namespace {

constexpr uint64_t HINT_MAGIC = 0x31544E4948504A42ull;  // "BJPHINT1"
constexpr uint32_t HINT_PLACEHOLDER = 0xffffffffu;
constexpr uint64_t PLACEHOLDER_BIT = (uint64_t)1 << 63;  // cs/mod.rs:44
constexpr uint64_t LOW_U48_MASK = ((uint64_t)1 << 48) - 1;  // cs/mod.rs:47
constexpr uint32_t WIT_THREADS = 256;
constexpr uint32_t WIT_COLS = BJ_WIT_COLS;  // columns of a thread: its gathers in flight
constexpr uint32_t WIT_XCDS = 8;

struct CopyHint {
    uint64_t magic;
    uint32_t* cells_d;  // [n_cols][n_rows], packed
    uint32_t n_cols;
    uint64_t n_rows;
    uint64_t max_index;       // 0 for a hint of placeholders only
    uint64_t n_placeholders;
};

// Workgroup b -> (row block, column tile).  Row blocks come in groups of WIT_XCDS; within a group
// the workgroup ids run over the column tiles with the row block in the low three bits, so the
// tiles of a row block are WIT_XCDS ids apart.  Row blocks past the end (the last group's padding)
// return false.
__device__ __forceinline__ bool deal(uint32_t b, uint32_t row_blocks, uint32_t col_tiles, uint32_t& rb, uint32_t& ct) {
#if BJ_WIT_DEAL_BY_XCD
    const uint32_t per_group = WIT_XCDS * col_tiles;
    const uint32_t g = b / per_group, rem = b - g * per_group;
    ct = rem / WIT_XCDS;
    rb = g * WIT_XCDS + (rem & (WIT_XCDS - 1));
#else
    const uint32_t padded = (row_blocks + WIT_XCDS - 1) / WIT_XCDS * WIT_XCDS;
    ct = b / padded;
    rb = b - ct * padded;
#endif
    return rb < row_blocks;
}

__global__ __launch_bounds__(WIT_THREADS) void materialize_kernel(const uint32_t* __restrict__ cells, uint32_t n_cols,
                                                                  size_t n_rows, uint32_t row_blocks, uint32_t col_tiles,
                                                                  const uint64_t* __restrict__ all_values,
                                                                  uint64_t* __restrict__ out, size_t out_stride) {
    uint32_t rb, ct;
    if (!deal(blockIdx.x, row_blocks, col_tiles, rb, ct)) return;
    const size_t row = (size_t)rb * WIT_THREADS + threadIdx.x;
    if (row >= n_rows) return;
    const uint32_t c0 = ct * WIT_COLS;
    uint32_t idx[WIT_COLS];
    uint64_t v[WIT_COLS];
#pragma unroll
    for (uint32_t j = 0; j < WIT_COLS; j++)
        idx[j] = c0 + j < n_cols ? __builtin_nontemporal_load(cells + (size_t)(c0 + j) * n_rows + row) : HINT_PLACEHOLDER;
#pragma unroll
    for (uint32_t j = 0; j < WIT_COLS; j++) {
        v[j] = 0;
        if (idx[j] != HINT_PLACEHOLDER) v[j] = all_values[idx[j]];
    }
#pragma unroll
    for (uint32_t j = 0; j < WIT_COLS; j++)
        if (c0 + j < n_cols) __builtin_nontemporal_store(v[j], out + (size_t)(c0 + j) * out_stride + row);
}

__global__ __launch_bounds__(WIT_THREADS) void multiplicities_kernel(const uint32_t* __restrict__ mult, size_t len,
                                                                     uint64_t* __restrict__ out, size_t n_rows) {
    const size_t i = blockIdx.x * (size_t)WIT_THREADS + threadIdx.x;
    if (i >= n_rows) return;
    out[i] = i < len ? (uint64_t)mult[i] : 0;  // from_u64_unchecked(src as u64), witness.rs:515
}

// One cell per lane: the identity value of the cell prev names.  tab: [n_cols non-residues |
// w_n^i, i < n / 2], canonical; w_n^(i + n/2) = -w_n^i.  An entry that names no cell of the trace
// gives 0, which is no identity value, and reads nothing.
__global__ __launch_bounds__(WIT_THREADS) void permutation_polys_kernel(const uint32_t* __restrict__ prev,
                                                                        uint32_t n_cols, uint32_t log_n,
                                                                        const uint64_t* __restrict__ tab,
                                                                        uint64_t* __restrict__ out, size_t out_stride) {
    const size_t n = (size_t)1 << log_n;
    const size_t row = blockIdx.x * (size_t)WIT_THREADS + threadIdx.x;
    if (row >= n) return;
    const uint32_t col = blockIdx.y;
    const uint64_t src = __builtin_nontemporal_load(prev + (size_t)col * n + row);
    const uint64_t src_col = src >> log_n, src_row = src & (n - 1);
    uint64_t x = 0;
    if (src_col < n_cols) {
        const size_t half = n >> 1;
        const uint64_t w = log_n ? tab[n_cols + (src_row & (half - 1))] : 1;
        x = gl::canon(gl::mul(tab[src_col], w));
        if (log_n && src_row >= half) x = gl::P - x;  // x is a product of units: never 0
    }
    __builtin_nontemporal_store(x, out + (size_t)col * out_stride + row);
}

const CopyHint* live(const void* hint) {
    const CopyHint* h = static_cast<const CopyHint*>(hint);
    return h && h->magic == HINT_MAGIC ? h : nullptr;
}

}  // namespace

}  // namespace bj

extern "C" {

int bj_copy_hint_upload_d(const uint64_t* words, uint32_t n_cols, uint64_t n_rows, size_t stride, void** hint) {
    if (!hint) return bj::set_error(BJ_EINVAL, "bj_copy_hint_upload_d: null hint");
    *hint = nullptr;
    if (!words || n_cols == 0 || n_rows == 0 || n_rows > ((uint64_t)1 << 32))
        return bj::set_error(BJ_EINVAL, "bj_copy_hint_upload_d: null words, no columns, no rows or more than 2^32 rows");
    if (stride < n_rows) return bj::set_error(BJ_EINVAL, "bj_copy_hint_upload_d: the column stride is below n_rows");
    const size_t cells = (size_t)n_cols * n_rows;
    std::vector<uint32_t> packed;
    try {
        packed.resize(cells);
    } catch (const std::bad_alloc&) {
        return bj::set_error(BJ_ENOMEM, "bj_copy_hint_upload_d: out of host memory");
    }
    uint64_t max_index = 0, n_placeholders = 0;
    for (uint32_t c = 0; c < n_cols; c++) {
        const uint64_t* col = words + (size_t)c * stride;
        uint32_t* dst = packed.data() + (size_t)c * n_rows;
        for (size_t r = 0; r < n_rows; r++) {
            const uint64_t w = col[r];
            if (w & bj::PLACEHOLDER_BIT) {
                dst[r] = bj::HINT_PLACEHOLDER;
                n_placeholders++;
                continue;
            }
            const uint64_t index = w & bj::LOW_U48_MASK;
            if (index >= bj::HINT_PLACEHOLDER) {
                char msg[200];
                snprintf(msg, sizeof msg,
                         "bj_copy_hint_upload_d: column %u row %zu names index %llu, which does not fit the packed cell "
                         "(an index is below 2^32 - 1)", c, r, (unsigned long long)index);
                return bj::set_error(BJ_EINVAL, msg);
            }
            dst[r] = (uint32_t)index;
            if (index > max_index) max_index = index;
        }
    }
    bj::CopyHint* h = new (std::nothrow) bj::CopyHint;
    if (!h) return bj::set_error(BJ_ENOMEM, "bj_copy_hint_upload_d: out of host memory");
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->cells_d), cells * sizeof(uint32_t));
    if (e == hipSuccess) {
        e = hipMemcpy(h->cells_d, packed.data(), cells * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) (void)hipFree(h->cells_d);
    }
    if (e != hipSuccess) {
        delete h;
        return bj::hip_fail(e, "copy hint upload");
    }
    h->magic = bj::HINT_MAGIC;
    h->n_cols = n_cols;
    h->n_rows = n_rows;
    h->max_index = max_index;
    h->n_placeholders = n_placeholders;
    *hint = h;
    return BJ_OK;
}

int bj_copy_hint_release(void* hint) {
    bj::CopyHint* h = static_cast<bj::CopyHint*>(hint);
    if (!h) return BJ_OK;
    if (h->magic != bj::HINT_MAGIC) return bj::set_error(BJ_EINVAL, "bj_copy_hint_release: not a copy hint");
    h->magic = 0;
    const hipError_t e = hipFree(h->cells_d);
    delete h;
    return bj::ok_or(e, "copy hint release");
}

int bj_copy_hint_info(const void* hint, uint32_t* n_cols, uint64_t* n_rows, uint64_t* max_index,
                      uint64_t* n_placeholders) {
    const bj::CopyHint* h = bj::live(hint);
    if (!h) return bj::set_error(BJ_EINVAL, "bj_copy_hint_info: not a copy hint");
    if (n_cols) *n_cols = h->n_cols;
    if (n_rows) *n_rows = h->n_rows;
    if (max_index) *max_index = h->max_index;
    if (n_placeholders) *n_placeholders = h->n_placeholders;
    return BJ_OK;
}

int bj_materialize_columns_d(const void* hint, const uint64_t* all_values, uint64_t num_values, uint64_t* out,
                             size_t out_stride, void* stream) {
    const bj::CopyHint* h = bj::live(hint);
    if (!h) return bj::set_error(BJ_EINVAL, "bj_materialize_columns_d: not a copy hint");
    if (!all_values || !out) return bj::set_error(BJ_EINVAL, "bj_materialize_columns_d: null pointer");
    if (out_stride < h->n_rows) return bj::set_error(BJ_EINVAL, "bj_materialize_columns_d: out_stride is below n_rows");
    if (num_values <= h->max_index) {
        char msg[160];
        snprintf(msg, sizeof msg, "bj_materialize_columns_d: the hint names index %llu and all_values holds %llu",
                 (unsigned long long)h->max_index, (unsigned long long)num_values);
        return bj::set_error(BJ_EINVAL, msg);
    }
    const uint64_t row_blocks = (h->n_rows + bj::WIT_THREADS - 1) / bj::WIT_THREADS;
    const uint64_t col_tiles = (h->n_cols + bj::WIT_COLS - 1) / bj::WIT_COLS;
    const uint64_t padded = (row_blocks + bj::WIT_XCDS - 1) / bj::WIT_XCDS * bj::WIT_XCDS;
    if (padded * col_tiles > 0x7fffffffull)
        return bj::set_error(BJ_EINVAL, "bj_materialize_columns_d: more workgroups than one grid holds");
    hipLaunchKernelGGL(bj::materialize_kernel, dim3((unsigned)(padded * col_tiles)), dim3(bj::WIT_THREADS), 0,
                       bj::S(stream), h->cells_d, h->n_cols, (size_t)h->n_rows, (uint32_t)row_blocks,
                       (uint32_t)col_tiles, all_values, out, out_stride);
    return bj::ok_or(hipGetLastError(), "materialize columns");
}

int bj_materialize_multiplicities_d(const uint32_t* mult_u32, uint64_t len, uint64_t* out, uint64_t n_rows,
                                    void* stream) {
    if (!out || n_rows == 0) return bj::set_error(BJ_EINVAL, "bj_materialize_multiplicities_d: null out or no rows");
    if (len > n_rows) return bj::set_error(BJ_EINVAL, "bj_materialize_multiplicities_d: more counts than rows");
    if (len && !mult_u32) return bj::set_error(BJ_EINVAL, "bj_materialize_multiplicities_d: null counts");
    const uint64_t blocks = (n_rows + bj::WIT_THREADS - 1) / bj::WIT_THREADS;
    if (blocks > 0x7fffffffull)
        return bj::set_error(BJ_EINVAL, "bj_materialize_multiplicities_d: more workgroups than one grid holds");
    hipLaunchKernelGGL(bj::multiplicities_kernel, dim3((unsigned)blocks), dim3(bj::WIT_THREADS), 0,
                       bj::S(stream), mult_u32, (size_t)len, out, (size_t)n_rows);
    return bj::ok_or(hipGetLastError(), "materialize multiplicities");
}

int bj_permutation_polys_d(const uint32_t* prev, uint32_t n_cols, uint64_t n_rows, const uint64_t* non_residues,
                           uint64_t* out, size_t out_stride, void* stream) {
    if (n_rows == 0 || (n_rows & (n_rows - 1)) || n_rows > ((uint64_t)1 << 32))
        return bj::set_error(BJ_EINVAL, "bj_permutation_polys_d: n_rows must be a power of two of at most 2^32");
    if (!prev || !non_residues || !out) return bj::set_error(BJ_EINVAL, "bj_permutation_polys_d: null pointer");
    const uint64_t n = n_rows;
    const uint32_t log_n = (uint32_t)__builtin_ctzll(n);
    if (n_cols == 0 || n_cols > 65535 || (uint64_t)n_cols * n > ((uint64_t)1 << 32))
        return bj::set_error(BJ_EINVAL, "bj_permutation_polys_d: n_cols outside 1..65535 or more than 2^32 cells");
    if (out_stride < n) return bj::set_error(BJ_EINVAL, "bj_permutation_polys_d: out_stride is below n_rows");
    hipStream_t st = bj::S(stream);
    const size_t half = log_n ? (size_t)(n >> 1) : 0;
    std::vector<uint64_t> k(n_cols);
    for (uint32_t c = 0; c < n_cols; c++) k[c] = gl::canon(non_residues[c]);
    bj::Workspace ws(st);
    uint64_t* tab = nullptr;
    hipError_t e = ws.alloc(&tab, n_cols + half);
    if (e != hipSuccess) return bj::hip_fail(e, "permutation polys table");
    // k is pageable host memory: the copy has left it when the call returns
    e = hipMemcpyAsync(tab, k.data(), n_cols * sizeof(uint64_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess && log_n) e = bj::launch_twiddles_natural(tab + n_cols, log_n, false, st);
    if (e == hipSuccess) {
        const uint64_t blocks = (n + bj::WIT_THREADS - 1) / bj::WIT_THREADS;
        hipLaunchKernelGGL(bj::permutation_polys_kernel, dim3((unsigned)blocks, n_cols), dim3(bj::WIT_THREADS), 0, st,
                           prev, n_cols, log_n, tab, out, out_stride);
        e = hipGetLastError();
    }
    return bj::ok_or(e, "permutation polys");
}

}  // extern "C"
