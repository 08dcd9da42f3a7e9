// csrc/host.hpp on the host alone (test infrastructure; tests/test_host_shim.py): the power-of-two
// helpers, the BJ_EHIP message, and the workspace and event set against counting stand-ins for the
// runtime calls they make.  Needs no device: only hipGetErrorString comes from the HIP runtime.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../era-boojum_amd/csrc/host.hpp"

static std::string last_error;
static std::vector<void*> freed, destroyed;
static int made = 0;

// the two functions of the library that host.hpp calls
namespace bj {
int set_error(int code, const char* msg) {
    last_error = msg;
    return code;
}
hipError_t pool_alloc(void** p, size_t bytes, hipStream_t) {
    *p = malloc(bytes ? bytes : 1);
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
}  // namespace bj

// the program's own definitions take the place of the runtime's
extern "C" hipError_t hipFreeAsync(void* p, hipStream_t) {
    freed.push_back(p);
    free(p);
    return hipSuccess;
}
extern "C" hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags) {
    if (flags != hipEventDisableTiming) return hipErrorInvalidValue;
    *e = reinterpret_cast<hipEvent_t>(static_cast<uintptr_t>(++made));
    return hipSuccess;
}
extern "C" hipError_t hipEventDestroy(hipEvent_t e) {
    destroyed.push_back(e);
    return hipSuccess;
}

static int failures = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            fprintf(stderr, "line %d: %s is false\n", __LINE__, #cond); \
            failures++;                                               \
        }                                                             \
    } while (0)

static int try_hip(hipError_t e) {
    HIP_TRY(e, "try");
    return BJ_OK;
}
static int try_bj(int r) {
    BJ_TRY(r);
    return 77;
}

int main() {
    const uint64_t top = 1ull << 63;
    CHECK(!bj::is_pow2(0) && bj::is_pow2(1) && bj::is_pow2(2) && !bj::is_pow2(3));
    CHECK(bj::is_pow2(top) && !bj::is_pow2(top + 1));
    CHECK(bj::log2u(1) == 0 && bj::log2u(2) == 1 && bj::log2u(1ull << 31) == 31 && bj::log2u(top) == 63);

    const std::string want = std::string("what: ") + hipGetErrorString(hipErrorInvalidValue);
    CHECK(bj::hip_fail(hipErrorInvalidValue, "what") == BJ_EHIP && last_error == want);
    CHECK(bj::ok_or(hipSuccess, "fine") == BJ_OK && last_error == want);
    CHECK(bj::ok_or(hipErrorInvalidValue, "what") == BJ_EHIP && last_error == want);
    CHECK(bj::fail(BJ_EINVAL, std::string(300, 'x')) == BJ_EINVAL && last_error.size() == 300);  // no truncation
    CHECK(try_hip(hipSuccess) == BJ_OK && try_hip(hipErrorInvalidValue) == BJ_EHIP);
    CHECK(last_error == std::string("try: ") + hipGetErrorString(hipErrorInvalidValue));
    CHECK(try_bj(0) == 77 && try_bj(BJ_EINVAL) == BJ_EINVAL);
    int x = 0;
    CHECK(bj::S(&x) == reinterpret_cast<hipStream_t>(&x) && bj::S(nullptr) == nullptr);

    // nothing allocated, nothing made: no call into the runtime
    {
        bj::Workspace ws(nullptr);
        bj::Events ev;
        CHECK(ev.make(0) == hipSuccess);
    }
    CHECK(freed.empty() && destroyed.empty() && made == 0);
    // every allocation is freed once, in the order made; every event is destroyed
    std::vector<void*> got;
    {
        bj::Workspace ws(nullptr);
        uint64_t *a = nullptr, *b = nullptr, *c = nullptr;
        CHECK(ws.alloc(&a, 3) == hipSuccess && ws.alloc(&b, 0) == hipSuccess && ws.alloc_bytes(&c, 5) == hipSuccess);
        a[2] = 1;  // three words
        got = {a, b, c};
        bj::Events ev;
        CHECK(ev.make(2) == hipSuccess && ev.make(1) == hipSuccess && ev.ev.size() == 3);
        CHECK(freed.empty() && destroyed.empty());
    }
    CHECK(freed == got && destroyed.size() == 3 && made == 3);
    if (failures) return 1;
    puts("host shim ok");
    return 0;
}
