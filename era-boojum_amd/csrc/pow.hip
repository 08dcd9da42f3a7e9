// Proof-of-work grinding (cs/implementations/pow.rs, prover.rs:2107-2133): the smallest nonce with
//   u64::from_le_bytes(H(seed || nonce.to_le_bytes())[..8]).trailing_zeros() >= pow_bits,
// H = Blake2s256 (pow.rs:51-135) or Keccak256 (pow.rs:137-221).  The reference scans 0, 1, 2, ...
// for pow_bits <= 16 (pow.rs:58-71) and races 2^16-nonce slices above (pow.rs:76-119); returning
// the smallest passing nonce equals the first and is one of the answers of the second.
//
// The search is 2^pow_bits independent hashes with no memory traffic.  The seed's full blocks are
// absorbed once on the host (pow_hash.hpp); the midstate and the tail block(s) reach the kernel
// by value, so they sit in SGPRs and only the nonce words are per lane.  One nonce per lane and
// iteration, consecutive lanes consecutive nonces, a block a contiguous tile of the window and
// lower tiles in lower blocks, so the smallest nonces are tried first.  The result is one u64 in
// device memory combined by minimum; a wave polls it once per iteration and stops once all it
// has left lies above the polled value.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include "capi_common.hpp"
#include "pow_hash.hpp"
#include "stage_host.hpp"

namespace bj {

namespace {

constexpr uint32_t POW_THREADS = 256;
constexpr uint32_t POW_ITERS = 4;  // nonces per lane and tile
constexpr uint64_t POW_TILE = (uint64_t)POW_THREADS * POW_ITERS;
constexpr uint64_t POW_MAX_BLOCKS = (uint64_t)1 << 22;  // larger windows walk tiles blockIdx.x, + gridDim.x, ...

// bj_pow_run_h: the first window holds 2^(pow_bits + 3) nonces (no solution in it: e^-8), at least
// 2^16, and no launch more than POW_LAUNCH_CAP: 2^30 nonces are 24 ms of Blake2s and 95 ms of
// Keccak at the measured 44.1 and 11.3 G hashes/s
constexpr uint64_t POW_LAUNCH_CAP = (uint64_t)1 << 30;
constexpr uint64_t POW_MIN_WINDOW = (uint64_t)1 << 16;

struct B2sPow {
    using Mid = pow::B2sMid;
    static Mid midstate(const uint8_t* seed, size_t n) { return pow::b2s_midstate(seed, n); }
    template <int BLOCKS, bool FAST>
    __host__ __device__ __forceinline__ static uint32_t word0(const Mid& a, uint64_t nonce) {
        return pow::b2s_word0<BLOCKS, FAST>(a, nonce);
    }
};
struct KcPow {
    using Mid = pow::KcMid;
    static Mid midstate(const uint8_t* seed, size_t n) { return pow::kc_midstate(seed, n); }
    template <int BLOCKS, bool FAST>
    __host__ __device__ __forceinline__ static uint32_t word0(const Mid& a, uint64_t nonce) {
        return pow::kc_word0<BLOCKS, FAST>(a, nonce);
    }
};

typedef unsigned long long __attribute__((address_space(1))) * global_u64;

// The running minimum as other workgroups, on any XCD, have left it: a relaxed agent-scope load
// (a plain load may be served from this CU's L1 for ever).
__device__ __forceinline__ unsigned long long poll(global_u64 result) {
    return __hip_atomic_load(result, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint64_t wave_uniform(unsigned long long v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

// The nonce as a value the optimiser knows nothing about.  Left as base + lane, the loop's
// induction-variable passes carry every sum of a message word and a uniform term of the first
// rounds as a register of its own from iteration to iteration (about 70 adds per hash and 200
// VGPRs in the Blake2s kernel).
__device__ __forceinline__ uint64_t opaque(uint64_t v) {
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    asm volatile("" : "+v"(lo), "+v"(hi));
    return ((uint64_t)hi << 32) | lo;
}

// *result = min(*result, smallest passing nonce of [first, first + n)); first + n <= 2^64 - 1.
// The result only ever decreases, so a polled value is an upper bound of the final one however
// old it is.  A wave skips a nonce only when the nonce is above a polled value; the window's
// smallest passing nonce is never above any value the result takes, so it is always tested and
// always offered to the atomic (it is below whatever its wave polled, or equal to it and then
// stored already).  No workgroup waits for another.
template <class H, int BLOCKS, bool FAST>
__global__ __launch_bounds__(POW_THREADS, 4) void pow_search_kernel(const typename H::Mid mid, uint32_t pow_bits,
                                                                 uint64_t first, uint64_t n, uint64_t* result) {
    const global_u64 res = (global_u64)result;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t n_tiles = (n + POW_TILE - 1) / POW_TILE;
    uint64_t best = wave_uniform(poll(res));
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        uint64_t off = tile * POW_TILE + wave * 64;  // of this wave's lane 0 in the window
        for (uint32_t it = 0; it < POW_ITERS; it++, off += POW_THREADS) {
            if (off >= n) return;                // the window ends before this wave's nonces
            const uint64_t wave_first = first + off;
            if (wave_first > best) return;       // all that is left here is above the polled minimum
            const unsigned long long polled = poll(res);  // issued before the hash, read after it
            const uint64_t nonce = opaque(wave_first + lane);  // 64-bit: the carry may fall inside a tile
            const uint32_t w0 = H::template word0<BLOCKS, FAST>(mid, nonce);
            const bool ok = off + lane < n && pow::pow_passes(w0, pow_bits);
            const uint64_t hits = __ballot(ok);
            best = wave_uniform(polled);
            if (hits) {
                // consecutive lanes hold consecutive nonces: the lowest passing lane is the wave's minimum
                const uint64_t found = wave_first + (uint32_t)__builtin_ctzll(hits);
                if (found < best && lane == 0)
                    __hip_atomic_fetch_min(res, (unsigned long long)found, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return;  // this wave's later nonces, in this tile and the next ones, are all larger
            }
        }
    }
}

template <class H, int BLOCKS, bool FAST>
void launch_one(const typename H::Mid& mid, uint32_t pow_bits, uint64_t first, uint64_t n, uint64_t* result_d,
                hipStream_t st) {
    const uint64_t tiles = (n + POW_TILE - 1) / POW_TILE;
    const uint32_t grid = (uint32_t)(tiles < POW_MAX_BLOCKS ? tiles : POW_MAX_BLOCKS);
    hipLaunchKernelGGL((pow_search_kernel<H, BLOCKS, FAST>), dim3(grid), dim3(POW_THREADS), 0, st, mid, pow_bits,
                       first, n, result_d);
}

template <class H>
void launch(const uint8_t* seed, size_t seed_len, uint32_t pow_bits, uint64_t first, uint64_t n, uint64_t* result_d,
            hipStream_t st) {
    const typename H::Mid mid = H::midstate(seed, seed_len);
    if (seed_len == H::Mid::FAST_POS)
        launch_one<H, 1, true>(mid, pow_bits, first, n, result_d, st);
    else if (mid.blocks() == 1)
        launch_one<H, 1, false>(mid, pow_bits, first, n, result_d, st);
    else
        launch_one<H, 2, false>(mid, pow_bits, first, n, result_d, st);
}

template <class H>
uint32_t host_word0(const uint8_t* seed, size_t seed_len, uint64_t nonce) {
    const typename H::Mid mid = H::midstate(seed, seed_len);
    return mid.blocks() == 1 ? H::template word0<1, false>(mid, nonce) : H::template word0<2, false>(mid, nonce);
}

// NULL when the arguments every entry shares are usable, else what is wrong with them
const char* pow_fault(uint32_t hasher, const uint8_t* seed, size_t seed_len, uint32_t pow_bits) {
    if (hasher == BJ_HASHER_POSEIDON2) return "no Poseidon2 PoW runner (the reference has none)";
    if (hasher != BJ_HASHER_BLAKE2S && hasher != BJ_HASHER_KECCAK256) return "unknown hasher";
    if (pow_bits > 32) return "pow_bits > 32 (pow.rs:53)";
    if (!seed && seed_len) return "null seed with a non-zero length";
    return nullptr;
}

int pow_einval(const char* entry, const char* what) {
    char msg[160];
    snprintf(msg, sizeof msg, "%s: %s", entry, what);
    return bj::set_error(BJ_EINVAL, msg);
}

}  // namespace

}  // namespace bj

extern "C" {

int bj_pow_search_d(uint32_t hasher, const uint8_t* seed, size_t seed_len, uint32_t pow_bits, uint64_t first_nonce,
                    uint64_t n_nonces, uint64_t* result_d, void* stream) {
    if (const char* f = bj::pow_fault(hasher, seed, seed_len, pow_bits)) return bj::pow_einval("bj_pow_search_d", f);
    if (!result_d) return bj::pow_einval("bj_pow_search_d", "null result_d");
    if (n_nonces == 0) return bj::pow_einval("bj_pow_search_d", "n_nonces is 0");
    // the last nonce a window may hold is 2^64 - 2: 2^64 - 1 is BJ_POW_NO_RESULT (pow.rs:48, 61)
    if (n_nonces > BJ_POW_NO_RESULT - first_nonce)
        return bj::pow_einval("bj_pow_search_d", "first_nonce + n_nonces overflows");
    const hipStream_t st = bj::S(stream);
    if (hasher == BJ_HASHER_BLAKE2S)
        bj::launch<bj::B2sPow>(seed, seed_len, pow_bits, first_nonce, n_nonces, result_d, st);
    else
        bj::launch<bj::KcPow>(seed, seed_len, pow_bits, first_nonce, n_nonces, result_d, st);
    return bj::ok_or(hipGetLastError(), "pow search");
}

int bj_pow_run_h(uint32_t hasher, const uint8_t* seed, size_t seed_len, uint32_t pow_bits, uint64_t* nonce_out) {
    using namespace bj::capi;
    if (const char* f = bj::pow_fault(hasher, seed, seed_len, pow_bits)) return bj::pow_einval("bj_pow_run_h", f);
    if (!nonce_out) return bj::pow_einval("bj_pow_run_h", "null nonce_out");
    if (pow_bits == 0) {  // every nonce passes; the prover skips PoW altogether (prover.rs:2109, 2133)
        *nonce_out = 0;
        return BJ_OK;
    }
    SEAM_BEGIN;
    DBuf res(st);
    HIP_TRY(res.alloc(sizeof(uint64_t)), "pow result");
    uint64_t found = BJ_POW_NO_RESULT;
    H2D(res.p, &found, sizeof found);
    uint64_t window = (uint64_t)1 << (pow_bits + 3);
    if (window < bj::POW_MIN_WINDOW) window = bj::POW_MIN_WINDOW;
    if (window > bj::POW_LAUNCH_CAP) window = bj::POW_LAUNCH_CAP;
    for (uint64_t first = 0; first < BJ_POW_NO_RESULT && found == BJ_POW_NO_RESULT;) {
        const uint64_t rest = BJ_POW_NO_RESULT - first, n = window < rest ? window : rest;
        if (int r = bj_pow_search_d(hasher, seed, seed_len, pow_bits, first, n, res.p, st)) return r;
        D2H(&found, res.p, sizeof found);
        SEAM_END;
        first += n;
    }
    *nonce_out = found;
    return BJ_OK;
}

int bj_pow_verify_h(uint32_t hasher, const uint8_t* seed, size_t seed_len, uint32_t pow_bits, uint64_t nonce) {
    if (const char* f = bj::pow_fault(hasher, seed, seed_len, pow_bits)) return bj::pow_einval("bj_pow_verify_h", f);
    const uint32_t w0 = hasher == BJ_HASHER_BLAKE2S ? bj::host_word0<bj::B2sPow>(seed, seed_len, nonce)
                                                    : bj::host_word0<bj::KcPow>(seed, seed_len, nonce);
    return bj::pow::pow_passes(w0, pow_bits) ? 1 : 0;
}

}  // extern "C"
