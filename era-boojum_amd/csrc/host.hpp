// What every source of the library shares on the host: the error returns, the stream cast,
// stream-ordered workspace, event sets and the power-of-two helpers.  One copy of each; the C ABI
// files add their *_h seam to it (capi_common.hpp), the prover stages their domain checks
// (stage_host.hpp).  Host only.  Everything has internal linkage, so the library exports nothing
// of it.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/boojum_mi355x.h"
#include "bj_internal.hpp"

namespace bj {

namespace {

// `code`, with msg as the calling thread's bj_last_error() string (bj::set_error, capi.hip)
int fail(int code, const std::string& msg) { return set_error(code, msg.c_str()); }

// BJ_EHIP with "<what>: <the runtime's text>"
int hip_fail(hipError_t e, const char* what) {
    return fail(BJ_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}
int ok_or(hipError_t e, const char* what) { return e == hipSuccess ? BJ_OK : hip_fail(e, what); }

// return from the calling function on a HIP error ...
#define HIP_TRY(expr, what)                                    \
    do {                                                       \
        hipError_t _e = (expr);                                \
        if (_e != hipSuccess) return ::bj::hip_fail(_e, what); \
    } while (0)
// ... and on a non-zero code of one of the library's own calls, whose message is already set
#define BJ_TRY(expr)                    \
    do {                                \
        if (int r_ = (expr)) return r_; \
    } while (0)

hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

// Stream-ordered allocations from the library's pool, freed on the same stream, in the order they
// were made, when the workspace goes out of scope.  One buffer or many.
struct Workspace {
    hipStream_t st;
    std::vector<void*> ptrs;
    explicit Workspace(hipStream_t s) : st(s) {}
    Workspace(const Workspace&) = delete;
    Workspace& operator=(const Workspace&) = delete;
    hipError_t alloc_bytes(uint64_t** p, size_t bytes) {
        hipError_t e = pool_alloc(reinterpret_cast<void**>(p), bytes, st);
        if (e == hipSuccess) ptrs.push_back(*p);
        return e;
    }
    hipError_t alloc(uint64_t** p, size_t words) { return alloc_bytes(p, words * 8); }
    ~Workspace() {
        for (void* p : ptrs) (void)hipFreeAsync(p, st);
    }
};

// Events without timing, destroyed at scope exit.
struct Events {
    std::vector<hipEvent_t> ev;
    Events() = default;
    Events(const Events&) = delete;
    Events& operator=(const Events&) = delete;
    // n more events; on an error the ones already made stay in the set
    hipError_t make(size_t n) {
        for (size_t i = 0; i < n; i++) {
            hipEvent_t e;
            hipError_t r = hipEventCreateWithFlags(&e, hipEventDisableTiming);
            if (r != hipSuccess) return r;
            ev.push_back(e);
        }
        return hipSuccess;
    }
    ~Events() {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
};

bool is_pow2(uint64_t x) { return x && !(x & (x - 1)); }

// log2 of a power of two (of the next one up, for any other x <= 2^63)
uint32_t log2u(uint64_t x) {
    uint32_t l = 0;
    while ((1ull << l) < x) l++;
    return l;
}

}  // namespace

}  // namespace bj
