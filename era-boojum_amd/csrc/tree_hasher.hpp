// The Merkle node levels every tree hasher shares (continue_from_leaf_hashes,
// merkle_tree.rs:388-449): one node per lane, level by level, the last levels in one workgroup
// through LDS.  A hasher is a trait H with
//   static __device__ void node(const uint64_t* l, const uint64_t* r, uint64_t* o)
// (hash_into_node over two 4-word digests): P2Node (merkle.hip), B2sNode (blake2s.hip), KcNode
// (keccak.hip).  Every level's nodes go where node_hashes_enumerated_from_leafs puts them, the
// levels concatenated upward from `nodes`.
//
// The leaf kernels are not shared, on purpose: the chunked-leaf loops differ in their block and
// padding rules (Blake2s: 8-element blocks, the last full block is final; Keccak: 17-lane blocks,
// a full block is never final; Poseidon2: capacity or digest output forms), and a common sponge
// concept would be more machinery than the three loops it replaces.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include "bj_internal.hpp"

namespace bj {

template <class H>
__global__ __launch_bounds__(256) void node_level_kernel(const uint64_t* __restrict__ prev,
                                                         uint64_t* __restrict__ next, size_t m) {
    const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
    if (i >= m) return;
    uint64_t lr[8];
#pragma unroll
    for (int k = 0; k < 8; k++) lr[k] = prev[8 * i + k];
    H::node(lr, lr + 4, next + 4 * i);
}

// Remaining levels from `len` digests (len <= NODE_TAIL_MAX: each LDS buffer holds one level of
// at most NODE_TAIL_MAX / 2 nodes) down to cap_size, one workgroup.
template <class H>
__global__ __launch_bounds__(256) void node_tail_kernel(const uint64_t* __restrict__ prev, uint64_t* next,
                                                        uint32_t len, uint32_t cap_size) {
    __shared__ uint64_t buf[2][NODE_TAIL_MAX / 2 * 4];
    int cur = 0;
    uint64_t* outp = next;
    uint32_t m = len / 2;
    for (uint32_t i = threadIdx.x; i < m; i += 256) {
        uint64_t lr[8];
        for (int k = 0; k < 8; k++) lr[k] = prev[8 * (size_t)i + k];
        uint64_t o[4];
        H::node(lr, lr + 4, o);
        for (int k = 0; k < 4; k++) {
            buf[cur][4 * i + k] = o[k];
            outp[4 * (size_t)i + k] = o[k];
        }
    }
    outp += 4 * (size_t)m;
    __syncthreads();
    while (m > cap_size) {
        const uint32_t m2 = m / 2;
        for (uint32_t i = threadIdx.x; i < m2; i += 256) {
            uint64_t o[4];
            H::node(&buf[cur][8 * i], &buf[cur][8 * i + 4], o);
            for (int k = 0; k < 4; k++) {
                buf[cur ^ 1][4 * i + k] = o[k];
                outp[4 * (size_t)i + k] = o[k];
            }
        }
        outp += 4 * (size_t)m2;
        cur ^= 1;
        m = m2;
        __syncthreads();
    }
}

// Levels of more than tail_from digests as one grid each, then the tail kernel for the rest
// (tail_from is capped at what the tail's buffers hold).
template <class H>
hipError_t launch_nodes_per_lane(const uint64_t* leaves, size_t n_leaves, uint32_t cap_size, uint64_t* nodes,
                                 size_t tail_from, hipStream_t st) {
    tail_from = std::min(tail_from, NODE_TAIL_MAX);
    const uint64_t* prev = leaves;
    uint64_t* out = nodes;
    size_t len = n_leaves;
    while (len > cap_size && len > tail_from) {
        const size_t m = len / 2;
        hipLaunchKernelGGL(node_level_kernel<H>, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, prev, out, m);
        prev = out;
        out += 4 * m;
        len = m;
    }
    if (len > cap_size)
        hipLaunchKernelGGL(node_tail_kernel<H>, dim3(1), dim3(256), 0, st, prev, out, (uint32_t)len, cap_size);
    return hipGetLastError();
}

}  // namespace bj
