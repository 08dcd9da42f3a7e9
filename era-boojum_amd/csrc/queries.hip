// The query phase (prover.rs:2161-2266): every OracleQuery of a proof in one launch.
//
// An OracleQuery (proof.rs:64-97) is the elements a leaf hashed (QuerySource::get_elements,
// fri/mod.rs:683-927) and the leaf's Merkle path (MerkleTreeWithCap::get_proof,
// merkle_tree.rs:462-480).  Both are copies: nothing here does field arithmetic, so the digests of
// the byte-output hashers pass through unreduced.  The reference's index arithmetic,
//   tree_idx = (coset_idx << (log2 domain_size - log2 num_elements)) + inner_idx / num_elements,
// is one shift of the flat leaf index coset_idx * domain_size + inner_idx, and each FRI oracle's
// index is a further shift of the base oracles' (inner_idx >>= s_k, domain_size >>= s_k at
// prover.rs:2251-2252), so an oracle is described by its buffers and one index_shift.
//
// The work is latency: a record is a few hundred 8-byte loads that share no sector (one per
// source column, col_stride apart) plus 4 (depth + 1) digest words.  One block copies one record,
// a lane one word at a time, and a lane issues all its loads of a pass before it stores any.
//
// The same copy answers queries on a sharded tree (bj_sharded_queries_d, collective.hip): the rank
// that owns a leaf writes the record from its subtree and the gathered top levels, one all-gather
// carries every rank's records, and a second launch selects each query's owner's copy.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include "queries_sharded.hpp"
#include "stage_host.hpp"

namespace bj {

namespace {

constexpr uint32_t QUERY_THREADS = 256;
constexpr uint32_t QUERY_MAX_UNROLL = 4;     // words per lane with their loads in flight together
constexpr uint32_t QUERY_MAX_BLOCKS_X = 1u << 20;

struct QueryArgs {
    bj_query_oracle_t o[BJ_QUERY_MAX_ORACLES];
};
static_assert(sizeof(bj_query_oracle_t) == 56, "bj_query_oracle_t is 56 bytes (include/boojum_mi355x.h)");

__host__ __device__ inline uint32_t log2_u64(uint64_t v) {  // v a power of two
    return (uint32_t)__builtin_ctzll(v);
}
__host__ __device__ inline uint64_t leaf_words(const bj_query_oracle_t& d) {
    return (uint64_t)d.n_cols << d.log_elems_per_leaf;
}
__host__ __device__ inline uint64_t record_words(const bj_query_oracle_t& d) {
    return leaf_words(d) + 4 + 4 * (uint64_t)(log2_u64(d.n_leaves) - log2_u64(d.cap_size));
}

// a pointer known to be global memory, so that an address put together from integers is read with a
// global load and not a flat one
typedef const uint64_t __attribute__((address_space(1))) * global_words;

// Where word w of the record of tree index t comes from.  Words [0, n_el): the leaf's elements,
// column-major; then the leaf hash; then sibling l = entry (t >> l) ^ 1 of level l, level 0 the
// leaves and level l >= 1 at digest n_leaves - (n_leaves >> (l - 1)) of nodes.  Both candidates are
// computed as integers and one is selected, so a lane's loads do not sit behind branches; the
// candidate that is not selected may be a meaningless number and is never dereferenced.
__device__ __forceinline__ global_words word_source(const bj_query_oracle_t& d, uint64_t n_el, uint64_t t,
                                                       uint64_t w) {
    const uint32_t e = d.log_elems_per_leaf;
    const uint64_t c = w >> e, k = w & (((uint64_t)1 << e) - 1);
    const uintptr_t elem = (uintptr_t)d.src + 8 * (c * (uint64_t)d.col_stride + (t << e) + k);
    const uint64_t g = w - n_el;                  // word of the digest part
    const uint64_t which = g >> 2;                // 0: the leaf hash; l + 1: sibling l
    const uint32_t lvl = which ? (uint32_t)(which - 1) & 63 : 0;
    const uint64_t entry = which ? ((t >> lvl) ^ 1) : t;
    const uint64_t level_start = d.n_leaves - (d.n_leaves >> ((lvl ? lvl - 1 : 0) & 63));
    const uintptr_t level = lvl ? (uintptr_t)d.nodes + 32 * level_start : (uintptr_t)d.leaves;
    const uintptr_t digest = level + 32 * entry + 8 * (g & 3);
    return (global_words)(w < n_el ? elem : digest);
}

// Words [base + j * 256 + lane, j < U) of one record: U addresses, U loads, then U stores.  source(w)
// is where word w is read; a word past the record's end reads word `safe` instead (always there)
// and stores nothing.
template <uint32_t U, class Source>
__device__ __forceinline__ void copy_pass(const Source source, uint64_t safe, uint64_t n_words, uint64_t base,
                                          uint64_t* __restrict__ rec) {
    global_words p[U];
    uint64_t v[U];
#pragma unroll
    for (uint32_t j = 0; j < U; j++) {
        const uint64_t w = base + j * QUERY_THREADS + threadIdx.x;
        p[j] = source(w < n_words ? w : safe);
    }
#pragma unroll
    for (uint32_t j = 0; j < U; j++) v[j] = *p[j];
#pragma unroll
    for (uint32_t j = 0; j < U; j++) {
        const uint64_t w = base + j * QUERY_THREADS + threadIdx.x;
        if (w < n_words) rec[w] = v[j];
    }
}

// One record by one block: up to four words per lane in flight, as many passes as the record needs.
template <class Source>
__device__ __forceinline__ void copy_record(const Source source, uint64_t safe, uint64_t n_words,
                                            uint64_t* __restrict__ rec) {
    for (uint64_t base = 0; base < n_words; base += QUERY_MAX_UNROLL * QUERY_THREADS) {
        const uint64_t rest = n_words - base;  // block-uniform
        if (rest > 2 * QUERY_THREADS)
            copy_pass<4>(source, safe, n_words, base, rec);
        else if (rest > QUERY_THREADS)
            copy_pass<2>(source, safe, n_words, base, rec);
        else
            copy_pass<1>(source, safe, n_words, base, rec);
    }
}

// The status record, by one block: it looks at every index itself, so nothing has to be zeroed
// before the launch.
__device__ __forceinline__ void write_status(const uint64_t* __restrict__ indices, uint32_t n_queries, uint64_t domain,
                                             uint64_t* __restrict__ status) {
    __shared__ uint64_t bad_s[QUERY_THREADS / 64], first_s[QUERY_THREADS / 64];
    uint64_t bad = 0, first = ~(uint64_t)0;
    for (uint64_t q = threadIdx.x; q < n_queries; q += QUERY_THREADS) {
        if (indices[q] >= domain) {
            bad++;
            if (q < first) first = q;
        }
    }
#pragma unroll
    for (int s = 32; s; s >>= 1) {
        bad += (uint64_t)__shfl_down((unsigned long long)bad, s, 64);
        const uint64_t f = (uint64_t)__shfl_down((unsigned long long)first, s, 64);
        if (f < first) first = f;
    }
    if ((threadIdx.x & 63) == 0) {
        bad_s[threadIdx.x >> 6] = bad;
        first_s[threadIdx.x >> 6] = first;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t i = 1; i < QUERY_THREADS / 64; i++) {
            bad += bad_s[i];
            if (first_s[i] < first) first = first_s[i];
        }
        status[0] = bad;
        status[1] = first;
        status[2] = 0;
        status[3] = 0;
    }
}

// Block (x, y): the records of oracle y for queries x, x + gridDim.x, ...  Block (0, 0) also writes
// the status record.
__global__ __launch_bounds__(QUERY_THREADS) void oracle_queries_kernel(const QueryArgs a,
                                                                       const uint64_t* __restrict__ indices,
                                                                       uint32_t n_queries, uint64_t* __restrict__ out,
                                                                       uint64_t* __restrict__ status) {
    const uint32_t o = blockIdx.y;
    const bj_query_oracle_t d = a.o[o];
    uint64_t words_before = 0;
    for (uint32_t i = 0; i < o; i++) words_before += record_words(a.o[i]);
    const uint64_t n_words = record_words(d), n_el = leaf_words(d);
    const uint64_t domain = d.n_leaves << d.index_shift;
    uint64_t* block = out + (uint64_t)n_queries * words_before;
    for (uint64_t q = blockIdx.x; q < n_queries; q += gridDim.x) {
        const uint64_t idx = indices[q];
        uint64_t* rec = block + q * n_words;
        if (idx >= domain) {  // block-uniform
            for (uint64_t w = threadIdx.x; w < n_words; w += QUERY_THREADS) rec[w] = 0;
            continue;
        }
        const uint64_t t = idx >> d.index_shift;
        copy_record([=](uint64_t w) { return word_source(d, n_el, t, w); }, n_el, n_words, rec);
    }
    if (blockIdx.x == 0 && o == 0) write_status(indices, n_queries, domain, status);
}

bool pow2(uint64_t v) { return v && !(v & (v - 1)); }

// NULL when the descriptor is usable, else what is wrong with it
const char* oracle_fault(const bj_query_oracle_t& d) {
    if (!pow2(d.n_leaves) || !pow2(d.cap_size)) return "n_leaves and cap_size must be powers of two";
    if (d.n_leaves < d.cap_size) return "n_leaves < cap_size";
    if (!d.leaves) return "null leaves";
    if (!d.nodes && d.n_leaves != d.cap_size) return "null nodes with n_leaves > cap_size";
    if (d.log_elems_per_leaf > 31 || d.index_shift > 63) return "log_elems_per_leaf or index_shift out of range";
    if ((d.n_leaves << d.index_shift) >> d.index_shift != d.n_leaves) return "n_leaves << index_shift overflows";
    if (d.n_cols) {
        if (!d.src) return "null src with n_cols > 0";
        if ((d.n_leaves << d.log_elems_per_leaf) >> d.log_elems_per_leaf != d.n_leaves ||
            d.col_stride < (d.n_leaves << d.log_elems_per_leaf))
            return "col_stride < n_leaves << log_elems_per_leaf";
    }
    return nullptr;
}

// ------------------------------------------------------------------ sharded trees
// Where word w of the record of leaf `local` of the m = 2^log_m this rank (`owner`) holds comes
// from.  Words [0, n_cols): the row; then the leaf hash; then sibling l = entry (local >> l) ^ 1 of
// level l of the rank's subtree for l < local_depth (level 0 the leaves, level l >= 1 at digest
// m - (m >> (l - 1)) of nodes), and for the top_depth levels above it entry (owner >> tl) ^ 1 of
// level tl = l - local_depth over the G gathered subtree roots (level 0 the roots, level tl >= 1
// at digest G - (G >> (tl - 1)) of top).  As in word_source, every candidate is an integer and one
// is selected; local_depth >= 1, so the leaf hash is never taken for a top word.
__device__ __forceinline__ global_words sharded_word_source(const ShardedQueryOracle& d, uint32_t log_m,
                                                            uint32_t log_world, uint64_t owner, uint64_t local,
                                                            uint64_t w) {
    const uint64_t m = (uint64_t)1 << log_m, G = (uint64_t)1 << log_world;
    const uintptr_t elem = (uintptr_t)d.src + 8 * (w * (uint64_t)d.col_stride + local);
    const uint64_t g = w - d.n_cols;              // word of the digest part
    const uint64_t which = g >> 2;                // 0: the leaf hash; l + 1: sibling l
    const uint32_t lvl = which ? (uint32_t)(which - 1) & 63 : 0;
    const uint64_t entry = which ? ((local >> lvl) ^ 1) : local;
    const uint64_t level_start = m - (m >> ((lvl ? lvl - 1 : 0) & 63));
    const uintptr_t level = lvl ? (uintptr_t)d.nodes + 32 * level_start : (uintptr_t)d.leaves;
    const uint32_t tl = (lvl - d.local_depth) & 63;
    const uint64_t top_start = G - (G >> ((tl ? tl - 1 : 0) & 63));
    const uintptr_t top_level = tl ? (uintptr_t)d.top + 32 * top_start : (uintptr_t)d.roots;
    const uintptr_t low = level + 32 * entry, high = top_level + 32 * ((owner >> tl) ^ 1);
    const uintptr_t digest = (lvl >= d.local_depth ? high : low) + 8 * (g & 3);
    return (global_words)(w < d.n_cols ? elem : digest);
}

__device__ __forceinline__ uint64_t sharded_words_before(const ShardedQueryArgs& a, uint32_t o) {
    uint64_t words = 0;
    for (uint32_t i = 0; i < o; i++) words += sharded_query_words(a.o[i]);
    return words;
}

// Block (x, y): the records of oracle y for those of the queries x, x + gridDim.x, ... whose leaf
// this rank holds, written where the finished output has them; nothing else of `staging` is
// written.  Block (0, 0) also writes the status record.
__global__ __launch_bounds__(QUERY_THREADS) void sharded_records_kernel(const ShardedQueryArgs a,
                                                                        const uint64_t* __restrict__ indices,
                                                                        uint32_t n_queries,
                                                                        uint64_t* __restrict__ staging,
                                                                        uint64_t* __restrict__ status) {
    const uint32_t o = blockIdx.y;
    const ShardedQueryOracle d = a.o[o];
    const uint64_t n_words = sharded_query_words(d), n_el = d.n_cols;
    const uint32_t log_world = a.log_world, log_m = log2_u64(a.n_leaves) - log_world;
    const uint64_t rank = a.rank;
    uint64_t* block = staging + (uint64_t)n_queries * sharded_words_before(a, o);
    for (uint64_t q = blockIdx.x; q < n_queries; q += gridDim.x) {
        const uint64_t idx = indices[q];
        if (idx >= a.n_leaves || (idx >> log_m) != rank) continue;  // block-uniform
        const uint64_t local = idx & (((uint64_t)1 << log_m) - 1);
        copy_record([=](uint64_t w) { return sharded_word_source(d, log_m, log_world, rank, local, w); }, n_el,
                    n_words, block + q * n_words);
    }
    if (blockIdx.x == 0 && o == 0) write_status(indices, n_queries, a.n_leaves, status);
}

// Block (x, y): out's records of oracle y for queries x, x + gridDim.x, ..., each from the block
// of `gathered` that its owner wrote (rank r's block at r * n_queries * the oracles' words).
__global__ __launch_bounds__(QUERY_THREADS) void sharded_select_kernel(const ShardedQueryArgs a, uint32_t n_oracles,
                                                                       const uint64_t* __restrict__ indices,
                                                                       uint32_t n_queries,
                                                                       const uint64_t* __restrict__ gathered,
                                                                       uint64_t* __restrict__ out) {
    const uint32_t o = blockIdx.y;
    const uint64_t n_words = sharded_query_words(a.o[o]);
    const uint32_t log_m = log2_u64(a.n_leaves) - a.log_world;
    const uint64_t at = (uint64_t)n_queries * sharded_words_before(a, o);
    const uint64_t per_rank = (uint64_t)n_queries * sharded_words_before(a, n_oracles);
    for (uint64_t q = blockIdx.x; q < n_queries; q += gridDim.x) {
        const uint64_t idx = indices[q];
        uint64_t* rec = out + at + q * n_words;
        if (idx >= a.n_leaves) {  // block-uniform
            for (uint64_t w = threadIdx.x; w < n_words; w += QUERY_THREADS) rec[w] = 0;
            continue;
        }
        const uintptr_t from = (uintptr_t)(gathered + (idx >> log_m) * per_rank + at + q * n_words);
        copy_record([=](uint64_t w) { return (global_words)(from + 8 * w); }, 0, n_words, rec);
    }
}

uint32_t query_blocks_x(uint32_t n_queries) { return n_queries < QUERY_MAX_BLOCKS_X ? n_queries : QUERY_MAX_BLOCKS_X; }

}  // namespace

hipError_t sharded_query_records(const ShardedQueryArgs& a, uint32_t n_oracles, const uint64_t* indices,
                                 uint32_t n_queries, uint64_t* staging, uint64_t* status, hipStream_t st) {
    hipLaunchKernelGGL(sharded_records_kernel, dim3(query_blocks_x(n_queries), n_oracles), dim3(QUERY_THREADS), 0, st,
                       a, indices, n_queries, staging, status);
    return hipGetLastError();
}

hipError_t sharded_query_select(const ShardedQueryArgs& a, uint32_t n_oracles, const uint64_t* indices,
                                uint32_t n_queries, const uint64_t* gathered, uint64_t* out, hipStream_t st) {
    hipLaunchKernelGGL(sharded_select_kernel, dim3(query_blocks_x(n_queries), n_oracles), dim3(QUERY_THREADS), 0, st, a,
                       n_oracles, indices, n_queries, gathered, out);
    return hipGetLastError();
}

}  // namespace bj

extern "C" {

size_t bj_oracle_query_words(const bj_query_oracle_t* o) {
    if (!o || !bj::pow2(o->n_leaves) || !bj::pow2(o->cap_size) || o->n_leaves < o->cap_size ||
        o->log_elems_per_leaf > 31)
        return 0;
    return (size_t)bj::record_words(*o);
}

int bj_oracle_queries_d(const bj_query_oracle_t* oracles, uint32_t n_oracles, const uint64_t* indices_d,
                        uint32_t n_queries, uint64_t* out_d, size_t out_words, uint64_t* status_d, void* stream) {
    if (n_oracles < 1 || n_oracles > BJ_QUERY_MAX_ORACLES)
        return bj::set_error(BJ_EINVAL, "bj_oracle_queries_d: n_oracles outside 1..16");
    if (n_queries == 0) return bj::set_error(BJ_EINVAL, "bj_oracle_queries_d: n_queries is 0");
    if (!oracles || !indices_d || !out_d || !status_d)
        return bj::set_error(BJ_EINVAL, "bj_oracle_queries_d: null pointer");
    bj::QueryArgs a;
    memset(&a, 0, sizeof a);
    uint64_t words = 0;
    char msg[160];
    for (uint32_t i = 0; i < n_oracles; i++) {
        if (const char* f = bj::oracle_fault(oracles[i])) {
            snprintf(msg, sizeof msg, "bj_oracle_queries_d: oracle %u: %s", i, f);
            return bj::set_error(BJ_EINVAL, msg);
        }
        if (oracles[i].n_leaves << oracles[i].index_shift != oracles[0].n_leaves << oracles[0].index_shift) {
            snprintf(msg, sizeof msg, "bj_oracle_queries_d: oracle %u covers another domain than oracle 0", i);
            return bj::set_error(BJ_EINVAL, msg);
        }
        a.o[i] = oracles[i];
        words += bj::record_words(oracles[i]);
    }
    if (words > ~(uint64_t)0 / n_queries || out_words < words * n_queries)
        return bj::set_error(BJ_EINVAL, "bj_oracle_queries_d: out_words below n_queries * the oracles' record words");
    const uint32_t bx = n_queries < bj::QUERY_MAX_BLOCKS_X ? n_queries : bj::QUERY_MAX_BLOCKS_X;
    hipLaunchKernelGGL(bj::oracle_queries_kernel, dim3(bx, n_oracles), dim3(bj::QUERY_THREADS), 0,
                       bj::S(stream), a, indices_d, n_queries, out_d, status_d);
    return bj::ok_or(hipGetLastError(), "oracle queries");
}

}  // extern "C"
