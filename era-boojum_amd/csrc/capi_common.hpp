// What the C ABI files (capi.hip, capi_tree.hip) add to host.hpp: the stream and buffers of the
// host-pointer (*_h) entry points.  Host only.
#pragma once
#include <map>

#include "host.hpp"

namespace bj {
namespace capi {

// the shared names (host.hpp) that capi.hip and capi_tree.hip use through this namespace
using bj::fail;
using bj::hip_fail;
using bj::is_pow2;
using bj::S;

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

// One stream-ordered device buffer of the *_h entry points, sized in bytes.
namespace {
struct DBuf {
    uint64_t* p = nullptr;
    Workspace ws;
    explicit DBuf(hipStream_t s) : ws(s) {}
    hipError_t alloc(size_t bytes) { return ws.alloc_bytes(&p, bytes); }
};
}  // namespace

#define SEAM_BEGIN            \
    hipStream_t st;           \
    if (int r_ = seam_stream(&st)) return r_
#define H2D(dst, src, bytes) HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st), "memcpy")
#define D2H(dst, src, bytes) HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st), "memcpy")
#define SEAM_END HIP_TRY(hipStreamSynchronize(st), "sync")

}  // namespace capi
}  // namespace bj
