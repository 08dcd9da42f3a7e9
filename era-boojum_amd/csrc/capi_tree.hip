// C ABI of the Merkle trees (include/boojum_mi355x.h): the Poseidon2, Blake2s256 and Keccak256
// tree entry points and their host-pointer seams.  Host-side only: one table of the three
// hashers' launchers, the argument checks (the reference's asserts) written once, and the
// extern "C" names as calls of them.
#include "capi_common.hpp"

using namespace bj::capi;

namespace bj {

const TreeOps* tree_ops(int hasher) {
    static const TreeOps ops[] = {
        // BJ_HASHER_POSEIDON2: the carried state is the sponge's capacity, whatever went before
        {[](const uint64_t* src, size_t col_stride, uint32_t n_cols, size_t n_leaves, uint64_t, const uint64_t* cap_in,
            uint64_t* out, bool final_, hipStream_t st) {
             return launch_leaves_partial(src, col_stride, n_cols, n_leaves, cap_in, out, final_, st);
         },
         launch_leaves_chunked, launch_nodes,
         [](const uint64_t* words, uint32_t n_words, uint64_t* out4, hipStream_t st) {
             return launch_leaves(words, 1, n_words, 1, out4, st);  // n_words one-row columns of one leaf
         },
         true},
        // BJ_HASHER_BLAKE2S
        {launch_b2s_leaves, launch_b2s_leaves_chunked,
         [](const uint64_t* leaves, size_t n_leaves, uint32_t cap_size, uint64_t* nodes, hipStream_t st) {
             return launch_nodes_per_lane<B2sNode>(leaves, n_leaves, cap_size, nodes, NODE_TAIL_MAX, st);
         },
         launch_b2s_words, true},
        // BJ_HASHER_KECCAK256: whole leaves only (tree_leaves_partial refuses anything else)
        {[](const uint64_t* src, size_t col_stride, uint32_t n_cols, size_t n_leaves, uint64_t, const uint64_t*,
            uint64_t* out, bool, hipStream_t st) { return launch_kc_leaves(src, col_stride, n_cols, n_leaves, out, st); },
         launch_kc_leaves_chunked,
         [](const uint64_t* leaves, size_t n_leaves, uint32_t cap_size, uint64_t* nodes, hipStream_t st) {
             return launch_nodes_per_lane<KcNode>(leaves, n_leaves, cap_size, nodes, NODE_TAIL_MAX, st);
         },
         [](const uint64_t* words, uint32_t n_words, uint64_t* out4, hipStream_t st) {
             return launch_kc_leaves(words, 1, n_words, 1, out4, st);
         },
         false},
    };
    static_assert(BJ_HASHER_POSEIDON2 == 0 && BJ_HASHER_BLAKE2S == 1 && BJ_HASHER_KECCAK256 == 2, "table order");
    return hasher >= BJ_HASHER_POSEIDON2 && hasher <= BJ_HASHER_KECCAK256 ? &ops[hasher] : nullptr;
}

int tree_nodes(int hasher, const uint64_t* leaves, size_t n_leaves, uint32_t cap_size, uint64_t* nodes,
               hipStream_t st) {
    if (!is_pow2(n_leaves) || !is_pow2(cap_size) || n_leaves <= cap_size)
        return fail(BJ_EINVAL, "need power-of-two n_leaves > cap_size (merkle_tree.rs:83-96)");
    HIP_TRY(tree_ops(hasher)->nodes(leaves, n_leaves, cap_size, nodes, st), "nodes");
    return BJ_OK;
}

int tree_leaves_chunked(int hasher, const uint64_t* src, uint32_t n_cols, size_t col_stride, size_t n_leaves,
                        uint32_t elems_per_leaf, uint64_t* out, hipStream_t st) {
    if (!is_pow2(elems_per_leaf)) return fail(BJ_EINVAL, "elements_to_take_per_leaf must be a power of two");
    const uint32_t log_e = log2u(elems_per_leaf);
    if ((uint64_t)n_cols << log_e > 0xFFFFFFFFull) return fail(BJ_EINVAL, "leaf too long");
    HIP_TRY(tree_ops(hasher)->leaves_chunked(src, col_stride, n_cols, log_e, n_leaves, out, st), "leaves");
    return BJ_OK;
}

int tree_leaves_partial(int hasher, const uint64_t* src, uint32_t n_cols, size_t col_stride, size_t n_leaves,
                        uint64_t cols_before, const uint64_t* state_in, uint64_t* out, bool final_, hipStream_t st) {
    const TreeOps* ops = tree_ops(hasher);
    if (!ops->continues && (state_in || !final_))
        return fail(BJ_EINVAL, "internal: this hasher absorbs a leaf in one column range");
    HIP_TRY(ops->leaves(src, col_stride, n_cols, n_leaves, cols_before, state_in, out, final_, st), "leaves");
    return BJ_OK;
}

int tree_node_h(int hasher, const uint64_t* left4, const uint64_t* right4, uint64_t* out4) {
    SEAM_BEGIN;
    DBuf d(st);
    HIP_TRY(d.alloc(96), "hipMallocAsync");
    H2D(d.p, left4, 32);
    H2D(d.p + 4, right4, 32);
    if (int r = tree_nodes(hasher, d.p, 2, 1, d.p + 8, st)) return r;
    D2H(out4, d.p + 8, 32);
    SEAM_END;
    return BJ_OK;
}

int tree_leaf_h(int hasher, const uint64_t* elems, size_t n_elems, uint64_t* out4) {
    if (n_elems > 0xFFFFFFFFull) return fail(BJ_EINVAL, "leaf too long");
    SEAM_BEGIN;
    DBuf d(st), o(st);
    HIP_TRY(d.alloc(n_elems * 8), "hipMallocAsync");
    HIP_TRY(o.alloc(32), "hipMallocAsync");
    if (n_elems) H2D(d.p, elems, n_elems * 8);
    HIP_TRY(tree_ops(hasher)->message(d.p, (uint32_t)n_elems, o.p, st), "leaves");
    D2H(out4, o.p, 32);
    SEAM_END;
    return BJ_OK;
}

}  // namespace bj

extern "C" {

int bj_poseidon2_permute_d(uint64_t* states, size_t count, void* stream) {
    HIP_TRY(bj::launch_permute(states, count, S(stream)), "permute");
    return BJ_OK;
}

int bj_poseidon2_permute_h(uint64_t* state12) {
    SEAM_BEGIN;
    DBuf d(st);
    HIP_TRY(d.alloc(96), "hipMallocAsync");
    H2D(d.p, state12, 96);
    if (int r = bj_poseidon2_permute_d(d.p, 1, st)) return r;
    D2H(state12, d.p, 96);
    SEAM_END;
    return BJ_OK;
}

// ------------------------------------------------------------ Poseidon2 trees

int bj_merkle_leaves_d(const uint64_t* src, uint32_t n_cols, size_t col_stride, size_t n_leaves, uint64_t* leaves,
                       void* stream) {
    return bj::tree_leaves_partial(BJ_HASHER_POSEIDON2, src, n_cols, col_stride, n_leaves, 0, nullptr, leaves, true,
                                   S(stream));
}

int bj_merkle_leaves_partial_d(const uint64_t* src, uint32_t n_cols, size_t col_stride, size_t n_leaves,
                               const uint64_t* cap_in, uint64_t* out, int final_, void* stream) {
    if (!final_ && (n_cols & 7))
        return fail(BJ_EINVAL, "a non-final column range must be a multiple of the sponge rate (8)");
    if (final_ && cap_in && n_cols == 0)
        return fail(BJ_EINVAL, "the final column range of a continued sponge must be non-empty");
    return bj::tree_leaves_partial(BJ_HASHER_POSEIDON2, src, n_cols, col_stride, n_leaves, 0, cap_in, out, final_ != 0,
                                   S(stream));
}

int bj_merkle_leaves_chunked_d(const uint64_t* src, uint32_t n_cols, size_t col_stride, size_t n_leaves,
                               uint32_t elems_per_leaf, uint64_t* out, void* stream) {
    return bj::tree_leaves_chunked(BJ_HASHER_POSEIDON2, src, n_cols, col_stride, n_leaves, elems_per_leaf, out,
                                   S(stream));
}

int bj_merkle_nodes_d(const uint64_t* leaves, size_t n_leaves, uint32_t cap_size, uint64_t* nodes, void* stream) {
    return bj::tree_nodes(BJ_HASHER_POSEIDON2, leaves, n_leaves, cap_size, nodes, S(stream));
}

int bj_hash_into_leaf_h(const uint64_t* elems, size_t n_elems, uint64_t* out4) {
    return bj::tree_leaf_h(BJ_HASHER_POSEIDON2, elems, n_elems, out4);
}

int bj_hash_into_node_h(const uint64_t* left4, const uint64_t* right4, uint64_t* out4) {
    return bj::tree_node_h(BJ_HASHER_POSEIDON2, left4, right4, out4);
}

// ------------------------------------------------------------ Blake2s256 trees

int bj_blake2s_leaves_d(const uint64_t* src, uint32_t n_cols, size_t col_stride, size_t n_leaves, uint64_t* leaves,
                        void* stream) {
    return bj::tree_leaves_partial(BJ_HASHER_BLAKE2S, src, n_cols, col_stride, n_leaves, 0, nullptr, leaves, true,
                                   S(stream));
}

int bj_blake2s_leaves_partial_d(const uint64_t* src, uint32_t n_cols, size_t col_stride, size_t n_leaves,
                                uint64_t cols_before, const uint64_t* state_in, uint64_t* out, int final_,
                                void* stream) {
    if (cols_before & 7) return fail(BJ_EINVAL, "cols_before must be a multiple of the block (8 elements)");
    if ((cols_before != 0) != (state_in != nullptr))
        return fail(BJ_EINVAL, "state_in is required exactly when cols_before > 0");
    if (!final_ && (n_cols & 7))
        return fail(BJ_EINVAL, "a non-final column range must be a multiple of the block (8 elements)");
    if (final_ && cols_before && n_cols == 0)
        return fail(BJ_EINVAL, "the final column range of a continued message must be non-empty");
    return bj::tree_leaves_partial(BJ_HASHER_BLAKE2S, src, n_cols, col_stride, n_leaves, cols_before, state_in, out,
                                   final_ != 0, S(stream));
}

int bj_blake2s_leaves_chunked_d(const uint64_t* src, uint32_t n_cols, size_t col_stride, size_t n_leaves,
                                uint32_t elems_per_leaf, uint64_t* out, void* stream) {
    return bj::tree_leaves_chunked(BJ_HASHER_BLAKE2S, src, n_cols, col_stride, n_leaves, elems_per_leaf, out,
                                   S(stream));
}

int bj_blake2s_nodes_d(const uint64_t* leaves, size_t n_leaves, uint32_t cap_size, uint64_t* nodes, void* stream) {
    return bj::tree_nodes(BJ_HASHER_BLAKE2S, leaves, n_leaves, cap_size, nodes, S(stream));
}

int bj_blake2s_leaf_h(const uint64_t* elems, size_t n_elems, uint64_t* out4) {
    return bj::tree_leaf_h(BJ_HASHER_BLAKE2S, elems, n_elems, out4);
}

int bj_blake2s_node_h(const uint64_t* left4, const uint64_t* right4, uint64_t* out4) {
    return bj::tree_node_h(BJ_HASHER_BLAKE2S, left4, right4, out4);
}

// ------------------------------------------------------------ Keccak256 trees

int bj_keccak256_leaves_d(const uint64_t* src, uint32_t n_cols, size_t col_stride, size_t n_leaves, uint64_t* leaves,
                          void* stream) {
    return bj::tree_leaves_partial(BJ_HASHER_KECCAK256, src, n_cols, col_stride, n_leaves, 0, nullptr, leaves, true,
                                   S(stream));
}

int bj_keccak256_leaves_chunked_d(const uint64_t* src, uint32_t n_cols, size_t col_stride, size_t n_leaves,
                                  uint32_t elems_per_leaf, uint64_t* out, void* stream) {
    return bj::tree_leaves_chunked(BJ_HASHER_KECCAK256, src, n_cols, col_stride, n_leaves, elems_per_leaf, out,
                                   S(stream));
}

int bj_keccak256_nodes_d(const uint64_t* leaves, size_t n_leaves, uint32_t cap_size, uint64_t* nodes,
                         void* stream) {
    return bj::tree_nodes(BJ_HASHER_KECCAK256, leaves, n_leaves, cap_size, nodes, S(stream));
}

int bj_keccak256_leaf_h(const uint64_t* elems, size_t n_elems, uint64_t* out4) {
    return bj::tree_leaf_h(BJ_HASHER_KECCAK256, elems, n_elems, out4);
}

int bj_keccak256_node_h(const uint64_t* left4, const uint64_t* right4, uint64_t* out4) {
    return bj::tree_node_h(BJ_HASHER_KECCAK256, left4, right4, out4);
}

}  // extern "C"
