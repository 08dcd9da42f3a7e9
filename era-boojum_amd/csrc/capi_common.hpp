// What the C ABI files (capi.hip, capi_tree.hip) share, host only: error returns, the stream
// cast, and the stream and buffers of the host-pointer (*_h) entry points.
#pragma once
#include <hip/hip_runtime.h>
#include <map>
#include <string>

#include "../../include/boojum_mi355x.h"
#include "bj_internal.hpp"

namespace bj {
namespace capi {

// the message goes to the calling thread's bj_last_error() string (bj::set_error, capi.hip)
inline int fail(int code, const std::string& msg) { return bj::set_error(code, msg.c_str()); }

inline int hip_fail(hipError_t e, const char* what) {
    return fail(BJ_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define HIP_TRY(expr, what)                       \
    do {                                          \
        hipError_t _e = (expr);                   \
        if (_e != hipSuccess) return hip_fail(_e, what); \
    } while (0)

inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

inline bool is_pow2(size_t x) { return x && !(x & (x - 1)); }

// The *_h entry points run on a stream of their own per calling thread and device (created
// once; stream creation costs milliseconds on ROCm), with stream-ordered device buffers and
// explicit copies + synchronisation.  Nothing of theirs touches the legacy null stream, which
// every host thread shares.
inline int seam_stream(hipStream_t* out) {
    thread_local std::map<int, hipStream_t> tl;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev), "hipGetDevice");
    auto it = tl.find(dev);
    if (it == tl.end()) {
        hipStream_t st;
        HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking), "hipStreamCreate");
        it = tl.emplace(dev, st).first;
    }
    *out = it->second;
    return BJ_OK;
}

// Stream-ordered device buffer RAII for the *_h entry points.
struct DBuf {
    uint64_t* p = nullptr;
    hipStream_t st = nullptr;
    explicit DBuf(hipStream_t s) : st(s) {}
    hipError_t alloc(size_t bytes) { return bj::pool_alloc((void**)&p, bytes, st); }
    ~DBuf() { if (p) (void)hipFreeAsync(p, st); }
};

#define SEAM_BEGIN            \
    hipStream_t st;           \
    if (int r_ = seam_stream(&st)) return r_
#define H2D(dst, src, bytes) HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st), "memcpy")
#define D2H(dst, src, bytes) HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st), "memcpy")
#define SEAM_END HIP_TRY(hipStreamSynchronize(st), "sync")

}  // namespace capi
}  // namespace bj
