// The two launches of bj_sharded_queries_d: the kernels are in queries.hip, the collective call
// that orders them around its exchanges in collective.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace bj {

constexpr uint32_t SHARDED_QUERY_MAX_ORACLES = 16;  // BJ_QUERY_MAX_ORACLES

// One oracle as rank `rank` of 2^log_world sees it: its m = n_leaves >> log_world leaves, its
// subtree of local_depth levels and, when the cap is smaller than the world, the gathered subtree
// roots (world x 4) with the levels hashed over them (bj::tree_nodes' layout), top_depth of which
// lie below the cap.
struct ShardedQueryOracle {
    const uint64_t* src;  // this rank's rows of column c at src + c * col_stride
    size_t col_stride;
    const uint64_t* leaves;
    const uint64_t* nodes;
    const uint64_t* roots;  // top_depth > 0 only
    const uint64_t* top;    // top_depth > 1 only
    uint32_t n_cols, local_depth, top_depth, reserved;
};
struct ShardedQueryArgs {
    ShardedQueryOracle o[SHARDED_QUERY_MAX_ORACLES];
    uint64_t n_leaves;  // of the global tree, the same for every oracle
    uint32_t log_world, rank;
};

// Words of one record: the leaf's elements, the leaf hash, the local and then the top siblings.
__host__ __device__ inline uint64_t sharded_query_words(const ShardedQueryOracle& o) {
    return (uint64_t)o.n_cols + 4 + 4 * (uint64_t)(o.local_depth + o.top_depth);
}

// The records this rank owns, at their final offsets in `staging` (n_queries * the sum of the
// oracles' words); the records of other ranks' leaves and of indices >= n_leaves are not touched.
// status[4] as bj_oracle_queries_d writes it.
hipError_t sharded_query_records(const ShardedQueryArgs& a, uint32_t n_oracles, const uint64_t* indices,
                                 uint32_t n_queries, uint64_t* staging, uint64_t* status, hipStream_t st);

// out <- for every query its owner's copy, gathered + owner * (n_queries * the sum of words), and
// zeros for an index >= n_leaves.  Records that no owner wrote are not read.
hipError_t sharded_query_select(const ShardedQueryArgs& a, uint32_t n_oracles, const uint64_t* indices,
                                uint32_t n_queries, const uint64_t* gathered, uint64_t* out, hipStream_t st);

}  // namespace bj
