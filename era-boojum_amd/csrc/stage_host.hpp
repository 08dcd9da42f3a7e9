// What the prover-stage sources (fri.hip, deep.hip, stage2.hip, quotient.hip, gates.hip, witness.hip,
// queries.hip, pow.hip) share on the host: the BJ_EHIP return, the stream cast, stream-ordered
// scratch, the domain checks and the constants that travel by value in kernel arguments.  A new
// stage takes these from here and its Ext2 from ext2.hpp.  Everything has internal linkage, so the
// library exports nothing of it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include "gl.hpp"
#include "bj_internal.hpp"
#include "../../include/boojum_mi355x.h"

namespace bj {

namespace {

// BJ_EHIP with "<what>: <the runtime's text>" as the calling thread's bj_last_error()
int hip_error(hipError_t e, const char* what) {
    char msg[256];
    snprintf(msg, sizeof msg, "%s: %s", what, hipGetErrorString(e));
    return set_error(BJ_EHIP, msg);
}
int ok_or(hipError_t e, const char* what) { return e == hipSuccess ? BJ_OK : hip_error(e, what); }

hipStream_t stream_of(void* stream) { return reinterpret_cast<hipStream_t>(stream); }

// stream-ordered scratch from the library's pool, freed on the same stream when it goes out of scope
struct Scratch {
    uint64_t* p = nullptr;
    hipStream_t st;
    explicit Scratch(hipStream_t s) : st(s) {}
    hipError_t alloc(size_t words) { return pool_alloc((void**)&p, words * 8, st); }
    ~Scratch() {
        if (p) (void)hipFreeAsync(p, st);
    }
};

// the size checks of a domain of 2^log_n points and of its 2^log_q cosets; NULL when they are fine
const char* bad_log_n(uint32_t log_n) {
    return log_n > 32 ? "log_n exceeds the 2-adicity (32) of the field" : nullptr;
}
const char* bad_domain(uint32_t log_n, uint32_t log_q) {
    if (log_n > 32 || log_q > 32 || log_n + log_q > 32)
        return "log_n + log_q exceeds the 2-adicity (32) of the field";
    return nullptr;
}

// wpow[b] = w^(2^b), w the generator of the domain of 2^log points, canonical
void fill_wpow(uint64_t (&wpow)[32], uint32_t log) {
    uint64_t w = gl::domain_generator(log);
    for (uint32_t b = 0; b < 32; b++) {
        wpow[b] = gl::canon(w);
        w = gl::mul(w, w);
    }
}

// The source columns of a lookup sum beta + sum_t g_t src_t with their Ext2 coefficients, by value
// in the kernel arguments (stage2.hip's encodings, quotient.hip's lookup term).
constexpr uint32_t LOOKUP_MAX_SRC = 16;
struct LookupSources {
    const uint64_t* src[LOOKUP_MAX_SRC];
    uint64_t g[2 * LOOKUP_MAX_SRC];  // canonical
};
// false when one of the n_src <= LOOKUP_MAX_SRC columns is null
bool fill_lookup_sources(LookupSources& k, const uint64_t* const* srcs, uint32_t n_src, const uint64_t* g) {
    for (uint32_t t = 0; t < LOOKUP_MAX_SRC; t++) {
        k.src[t] = t < n_src ? srcs[t] : nullptr;
        k.g[2 * t] = t < n_src ? gl::canon(g[2 * t]) : 0;
        k.g[2 * t + 1] = t < n_src ? gl::canon(g[2 * t + 1]) : 0;
        if (t < n_src && !srcs[t]) return false;
    }
    return true;
}

}  // namespace

}  // namespace bj
