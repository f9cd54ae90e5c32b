// owners.h — the host side's HIP resources as owners: device memory, page-locked host memory, a stream, an event.  Each frees what it holds
// when it goes; none can be copied, all can be moved (std::vector<PinnedBuf> grows, a table of DevBufs is handed over).  The four HIP calls
// that free or destroy appear here and nowhere else.  Who owns what, and in which order it goes: DESIGN.md 4, "Ownership on the host side".
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <chrono>
#include <utility>
#include "env.h"

namespace {

inline double wall_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// WGBSSEG_PROFILE=1: where the host time of a call goes (allocations, upload), on stderr.  A process-wide latch, unlike every other
// switch: the allocators below consult it and have no context to keep it in.
inline bool profiling() { static const bool on = env_flag("WGBSSEG_PROFILE", false); return on; }
std::atomic<long long> g_alloc_us(0), g_alloc_bytes(0), g_alloc_calls(0);
inline void count_alloc(double t0, size_t bytes) { g_alloc_us += (long long)((wall_s() - t0) * 1e6); g_alloc_bytes += (long long)bytes; g_alloc_calls += 1; }

struct DevBuf {             // grow-only device buffer
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept { swap(o); }
    DevBuf& operator=(DevBuf&& o) noexcept { DevBuf t(std::move(o)); swap(t); return *this; }      // (what this held goes with t)
    ~DevBuf() { release(); }
    void swap(DevBuf& o) { std::swap(p, o.p); std::swap(cap, o.cap); }
    hipError_t ensure(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        const double t0 = profiling() ? wall_s() : 0.0;
        if (p) { hipError_t e = hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
        size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) { e = hipMalloc(&p, bytes); want = bytes; }
        if (e == hipSuccess) cap = want;
        if (profiling()) count_alloc(t0, want);
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

struct PinnedBuf {          // grow-only page-locked host buffer (fast, truly asynchronous D2H)
    void* p = nullptr;
    size_t cap = 0;
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf&& o) noexcept { swap(o); }
    PinnedBuf& operator=(PinnedBuf&& o) noexcept { PinnedBuf t(std::move(o)); swap(t); return *this; }
    ~PinnedBuf() { release(); }
    void swap(PinnedBuf& o) { std::swap(p, o.p); std::swap(cap, o.cap); }
    bool ensure(size_t bytes)
    {
        if (bytes <= cap) return true;
        const double t0 = profiling() ? wall_s() : 0.0;
        if (!ensure_exact(bytes + bytes / 4 + 4096)) return false;
        if (profiling()) count_alloc(t0, cap);
        return true;
    }
    bool ensure_exact(size_t bytes)
    {
        if (bytes <= cap) return true;
        release();
        if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { p = nullptr; return false; }
        cap = bytes;
        return true;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
};

// A stream or an event: converts to the raw handle, so a launch or a HIP call takes it as it took the handle.
template <class H, hipError_t (*Destroy)(H)>
struct Handle {
    H h = nullptr;
    Handle() = default;
    Handle(Handle&& o) noexcept : h(o.h) { o.h = nullptr; }
    Handle& operator=(Handle&& o) noexcept { std::swap(h, o.h); return *this; }      // (what this held goes with o)
    ~Handle() { if (h) (void)Destroy(h); }
    operator H() const { return h; }
};
struct Stream : Handle<hipStream_t, hipStreamDestroy> {
    hipError_t create() { return hipStreamCreateWithFlags(&h, hipStreamNonBlocking); }
    hipError_t create(int priority) { return hipStreamCreateWithPriority(&h, hipStreamNonBlocking, priority); }
};
struct Event : Handle<hipEvent_t, hipEventDestroy> {
    hipError_t create(bool timing = true) { return timing ? hipEventCreate(&h) : hipEventCreateWithFlags(&h, hipEventDisableTiming); }
};

}  // namespace
