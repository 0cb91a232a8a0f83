// rox_host.hpp -- host-side helpers shared by the translation units that define C entry points
// (roxtrace.hip, psf.hip, spotstats.hip): the error path, grow-only scratch blocks, and scratch
// kept per (device, stream).
#pragma once

#include <hip/hip_runtime.h>

#include <mutex>
#include <new>
#include <vector>

#include "../../include/roxtrace.h"

namespace rox {

// sets rox_last_error() from a printf format (roxtrace.hip) and returns code
int host_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

// Returns ROX_E_HIP with "<kHipWhere><expr>: <HIP error>" from the enclosing function when expr
// fails.  Every translation unit that uses it defines kHipWhere, the prefix of its messages.
#define HIP_TRY(expr)                                                                             \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return rox::host_fail(ROX_E_HIP, "%s%s: %s", kHipWhere, #expr, hipGetErrorString(e_)); \
    } while (0)

// Grow-only scratch blocks: a pointer p and its capacity cap, in whatever unit the caller counts.
// `kind` is kDeviceBlock (hipMalloc) or the hipHostMalloc flags of a pinned block.
constexpr unsigned kDeviceBlock = ~0u;

// Frees p and clears p and cap.  hipFree synchronises: no launch still reads the block.  On a
// failure p and cap are left as they were.
template <class T, class N>
hipError_t release(T *&p, N &cap, unsigned kind = kDeviceBlock)
{
    if (p) {
        const hipError_t e = kind == kDeviceBlock ? hipFree(p) : hipHostFree(p);
        if (e != hipSuccess)
            return e;
    }
    p = nullptr;
    cap = 0;
    return hipSuccess;
}

// Replaces p by a new block of `bytes` and capacity new_cap.  The old block is released first,
// so a failed allocation leaves p empty with cap 0, never a stale pointer behind a valid capacity.
template <class T, class N, class M>
hipError_t regrow(T *&p, N &cap, M new_cap, size_t bytes, unsigned kind = kDeviceBlock)
{
    hipError_t e = release(p, cap, kind);
    if (e != hipSuccess)
        return e;
    void *q = nullptr;
    e = kind == kDeviceBlock ? hipMalloc(&q, bytes) : hipHostMalloc(&q, bytes, kind);
    if (e != hipSuccess)
        return e;
    p = static_cast<T *>(q);
    cap = new_cap;
    return hipSuccess;
}

// ... a device block that is zeroed on stream st before its capacity is recorded
template <class T, class N, class M>
hipError_t regrow_zeroed(T *&p, N &cap, M new_cap, size_t bytes, hipStream_t st)
{
    hipError_t e = regrow(p, cap, 0, bytes);
    if (e == hipSuccess && (e = hipMemsetAsync(p, 0, bytes, st)) == hipSuccess)
        cap = new_cap;
    return e;
}

// The host state T of an entry point per (device, stream), made on first use and kept for the
// life of the process.  Calls on one stream take turns on the slot's mutex (stream order then
// keeps their kernels apart); different streams and devices do not meet.
template <class T>
class PerStream {
  public:
    struct Slot {
        int device;
        hipStream_t stream;
        std::mutex mu;
        T data;
    };

    // nullptr when out of host memory
    Slot *get(int device, hipStream_t st)
    {
        std::lock_guard<std::mutex> lock(mu_);
        for (Slot *s : slots_)
            if (s->device == device && s->stream == st)
                return s;
        Slot *s = new (std::nothrow) Slot;
        if (s) {
            s->device = device;
            s->stream = st;
            slots_.push_back(s);
        }
        return s;
    }

  private:
    std::mutex mu_;
    std::vector<Slot *> slots_;
};

}  // namespace rox
