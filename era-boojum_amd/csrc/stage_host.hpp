// What the prover-stage sources (fri.hip, deep.hip, stage2.hip, quotient.hip, gates.hip, witness.hip,
// queries.hip, pow.hip) add to host.hpp on the host: the domain checks and the constants that
// travel by value in kernel arguments.  A new stage takes the error returns, the stream cast and
// its scratch from host.hpp, these from here and its Ext2 from ext2.hpp.  Everything has internal
// linkage, so the library exports nothing of it.
#pragma once
#include "gl.hpp"
#include "host.hpp"

namespace bj {

namespace {

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
