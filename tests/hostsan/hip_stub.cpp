// hip_stub.cpp — the nine HIP runtime calls the host layer makes, on malloc / free / memcpy (see stub_common.h).
// TEST INFRASTRUCTURE ONLY.  No libamdhip64 is linked: "device" and "pinned" memory are heap blocks of exactly the size
// asked for, so an overrun of either is an AddressSanitizer finding.  Also home of the fault-injection / jitter state
// both stubs share.
#include <hip/hip_runtime_api.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "stub_common.h"

namespace {
struct Armed { int n, status; };
struct State {
    std::mutex m;
    std::map<std::string, int> calls;
    std::map<std::string, std::vector<Armed>> armed;
    uint64_t rng = 0;
    unsigned max_us = 0;
    std::map<void *, size_t> live; // blocks handed out by the stubbed runtime
    uint64_t live_bytes = 0;
};
State &st() { static State s; return s; }

uint64_t splitmix(uint64_t &s) {
    uint64_t z = (s += 0x9e3779b97f4a7c15ULL);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}

hipError_t stub_alloc(const char *fn, void **p, size_t bytes) {
    if (const int e = stub_enter(fn)) return (hipError_t)e;
    if (!p) return hipErrorInvalidValue;
    void *q = malloc(bytes ? bytes : 1);
    if (!q) return hipErrorOutOfMemory;
    State &s = st();
    std::lock_guard<std::mutex> l(s.m);
    s.live[q] = bytes;
    s.live_bytes += bytes;
    *p = q;
    return hipSuccess;
}
hipError_t stub_release(const char *fn, void *p) {
    if (const int e = stub_enter(fn)) return (hipError_t)e;
    if (!p) return hipSuccess;
    {
        State &s = st();
        std::lock_guard<std::mutex> l(s.m);
        auto it = s.live.find(p);
        if (it == s.live.end()) { // not ours, or freed twice: the real runtime only returns an error, here it is a finding
            fprintf(stderr, "hip_stub: %s(%p): not a live block of the stubbed runtime (double free?)\n", fn, p);
            free(p); // (AddressSanitizer reports the double free here, with the stacks of both frees)
            abort();
        }
        s.live_bytes -= it->second;
        s.live.erase(it);
    }
    free(p);
    return hipSuccess;
}
} // namespace

extern "C" void stub_fail_nth(const char *fn, int n, int status) {
    State &s = st();
    std::lock_guard<std::mutex> l(s.m);
    s.armed[fn].push_back({s.calls[fn] + n, status});
}
extern "C" void stub_jitter(uint64_t seed, unsigned max_us) {
    State &s = st();
    std::lock_guard<std::mutex> l(s.m);
    s.rng = seed;
    s.max_us = max_us;
}
extern "C" int stub_call_count(const char *fn) {
    State &s = st();
    std::lock_guard<std::mutex> l(s.m);
    auto it = s.calls.find(fn);
    return it == s.calls.end() ? 0 : it->second;
}
extern "C" void stub_reset(void) {
    State &s = st();
    std::lock_guard<std::mutex> l(s.m);
    s.calls.clear();
    s.armed.clear();
}
extern "C" uint64_t stub_live_bytes(void) {
    State &s = st();
    std::lock_guard<std::mutex> l(s.m);
    return s.live_bytes;
}
extern "C" int stub_enter(const char *fn) {
    State &s = st();
    unsigned us = 0;
    int status = 0;
    {
        std::lock_guard<std::mutex> l(s.m);
        if (s.max_us) us = (unsigned)(splitmix(s.rng) % (s.max_us + 1));
        const int c = ++s.calls[fn];
        auto it = s.armed.find(fn);
        if (it != s.armed.end())
            for (const Armed &a : it->second)
                if (a.n == c) status = a.status;
    }
    if (us) std::this_thread::sleep_for(std::chrono::microseconds(us));
    return status;
}

// ---- the runtime -----------------------------------------------------------------------------------------------------
// One device (ordinal 0).  A stream is an opaque heap block, so a leaked or doubly destroyed one is reported too.
extern "C" hipError_t hipSetDevice(int device) {
    if (const int e = stub_enter("hipSetDevice")) return (hipError_t)e;
    return device == 0 ? hipSuccess : hipErrorInvalidDevice;
}
extern "C" hipError_t hipStreamCreateWithFlags(hipStream_t *stream, unsigned int) {
    void *p = nullptr;
    const hipError_t e = stub_alloc("hipStreamCreateWithFlags", &p, 8);
    if (e == hipSuccess) *stream = (hipStream_t)p;
    return e;
}
extern "C" hipError_t hipStreamDestroy(hipStream_t stream) { return stub_release("hipStreamDestroy", (void *)stream); }
extern "C" hipError_t hipStreamSynchronize(hipStream_t) { return (hipError_t)stub_enter("hipStreamSynchronize"); }
extern "C" hipError_t hipMalloc(void **ptr, size_t size) { return stub_alloc("hipMalloc", ptr, size); }
extern "C" hipError_t hipFree(void *ptr) { return stub_release("hipFree", ptr); }
extern "C" hipError_t hipHostMalloc(void **ptr, size_t size, unsigned int) { return stub_alloc("hipHostMalloc", ptr, size); }
extern "C" hipError_t hipHostFree(void *ptr) { return stub_release("hipHostFree", ptr); }
extern "C" hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind, hipStream_t) {
    if (const int e = stub_enter("hipMemcpyAsync")) return (hipError_t)e;
    if (bytes && (!dst || !src)) return hipErrorInvalidValue;
    if (bytes) memcpy(dst, src, bytes);
    return hipSuccess;
}
