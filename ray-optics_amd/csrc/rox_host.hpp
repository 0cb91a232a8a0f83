// rox_host.hpp -- host-side helpers shared by the translation units that define C entry points
// (roxtrace.hip and the units its header lists, selftest.hip, spotstats.hip, the analyses psf.hip,
// mtf.hip, ee.hip, gmtf.hip and zernike.hip, and through rox_packets.hpp footprint.hip, fresnel.hip,
// solidangle.hip, segfoci.hip, wmaps.hip and wavediff.hip; imgsim.hip and huygens.hip):
// the error path and the argument checks, the environment switches, grow-only scratch blocks,
// scratch kept per (device, stream), the pinned staging of host inputs, the carving of one
// workspace block and an entry's turn on its per-stream state.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/roxtrace.h"

namespace rox {

// sets rox_last_error() from a printf format (roxtrace.hip) and returns code
int host_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

// the host copy of a system's rows (roxtrace.hip); n_ifcs receives their number
const rox_surface *system_rows(const rox_system *sys, int32_t *n_ifcs);
// m[i] = the FULL-packet slot of interface i (-1: a filtered phantom) and m[n_ifcs + i] = the
// number of slots before it, with or without ROX_FILTER_PHANTOMS; n_seg = the number of slots
void system_slot_map(const rox_system *sys, bool filter, std::vector<int32_t> &m, int32_t &n_seg);

// Returns ROX_E_HIP with "<kHipWhere><expr>: <HIP error>" from the enclosing function when expr
// fails.  Every translation unit that uses it defines kHipWhere, the prefix of its messages.
#define HIP_TRY(expr)                                                                             \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return rox::host_fail(ROX_E_HIP, "%s%s: %s", kHipWhere, #expr, hipGetErrorString(e_)); \
    } while (0)

// Returns the ROX_E_* code of expr from the enclosing function when it is not 0.
#define ROX_TRY(expr)                                                                             \
    do {                                                                                          \
        if (const int rc_ = (expr))                                                               \
            return rc_;                                                                           \
    } while (0)

// ---- argument checks: 0, or ROX_E_ARG with a message that starts with the entry's name e

// "<e>: <name> <v> outside [lo, hi]"
inline int check_range(const char *e, const char *name, int v, int lo, int hi)
{
    if (v < lo || v > hi)
        return host_fail(ROX_E_ARG, "%s: %s %d outside [%d, %d]", e, name, v, lo, hi);
    return 0;
}

// pixel pitches [total]: finite and > 0
inline int check_pitch(const char *e, int64_t total, const double *pitch)
{
    for (int64_t i = 0; i < total; ++i)
        if (!(std::isfinite(pitch[i]) && pitch[i] > 0.0))
            return host_fail(ROX_E_ARG, "%s: pitch[%lld] = %g is not finite and > 0", e, (long long)i, pitch[i]);
    return 0;
}

// radii [total][nr]: finite, >= 0, non-decreasing per plane
inline int check_radii(const char *e, int64_t total, int32_t nr, const double *radii)
{
    for (int64_t z = 0; z < total; ++z)
        for (int32_t j = 0; j < nr; ++j) {
            const double r = radii[z * nr + j];
            if (!(std::isfinite(r) && r >= 0.0))
                return host_fail(ROX_E_ARG, "%s: radii[%lld] = %g is not finite and >= 0", e,
                                 (long long)(z * nr + j), r);
            if (j && r < radii[z * nr + j - 1])
                return host_fail(ROX_E_ARG, "%s: radii[%lld] = %g decreases within its plane", e,
                                 (long long)(z * nr + j), r);
        }
    return 0;
}

// centers [total][2] (null: none): finite
inline int check_centers(const char *e, int64_t total, const double *centers)
{
    if (centers)
        for (int64_t i = 0; i < 2 * total; ++i)
            if (!std::isfinite(centers[i]))
                return host_fail(ROX_E_ARG, "%s: centers[%lld] = %g is not finite", e, (long long)i, centers[i]);
    return 0;
}

// frequencies [n]: finite and >= 0
inline int check_freqs(const char *e, int32_t n, const double *freqs)
{
    for (int32_t q = 0; q < n; ++q)
        if (!(std::isfinite(freqs[q]) && freqs[q] >= 0.0))
            return host_fail(ROX_E_ARG, "%s: freqs[%d] = %g is not finite and >= 0", e, q, freqs[q]);
    return 0;
}

// directions [n][2] = (ex, ey): finite, not both zero
inline int check_dirs(const char *e, int64_t n, const double *dirs)
{
    for (int64_t i = 0; i < n; ++i) {
        const double ex = dirs[2 * i], ey = dirs[2 * i + 1];
        if (!(std::isfinite(ex) && std::isfinite(ey)) || (ex == 0.0 && ey == 0.0))
            return host_fail(ROX_E_ARG, "%s: dirs[%lld] = (%g, %g) is not finite or is zero", e, (long long)i, ex,
                             ey);
    }
    return 0;
}

// histogram edges [rows][n_bins + 1]: finite and strictly increasing per row
inline int check_edges(const char *e, int64_t rows, int32_t n_bins, const double *edges)
{
    for (int64_t z = 0; z < rows; ++z)
        for (int32_t j = 0; j <= n_bins; ++j) {
            const int64_t i = z * (n_bins + 1) + j;
            if (!std::isfinite(edges[i]))
                return host_fail(ROX_E_ARG, "%s: edges[%lld] = %g is not finite", e, (long long)i, edges[i]);
            if (j && !(edges[i] > edges[i - 1]))
                return host_fail(ROX_E_ARG, "%s: edges[%lld] = %g does not increase within its row", e,
                                 (long long)i, edges[i]);
        }
    return 0;
}

// ---- environment switches.  One that is "read once" initialises a function-local static const
// with these; the documenting comment stays with the policy function that holds it.

// the integer value of environment variable `name`; dflt when it is unset or empty
inline long long env_int(const char *name, long long dflt)
{
    const char *e = getenv(name);
    return (e && *e) ? atoll(e) : dflt;
}

// whether `name` is set to a non-zero integer
inline bool env_flag(const char *name) { return env_int(name, 0) != 0; }

// ---- sizes and pointers

inline size_t up16(size_t b) { return (b + 15) & ~size_t(15); }
inline size_t up256(size_t b) { return (b + 255) & ~size_t(255); }

// Whether p is device memory.  A pointer HIP does not know (pageable host memory) is not, and
// the error of its failed query is cleared.
inline bool is_device(const void *p)
{
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) == hipSuccess)
        return at.type == hipMemoryTypeDevice;
    (void)hipGetLastError();
    return false;
}

// Planes per launch when each takes per_plane bytes of a scratch capped at cap bytes: at least
// one, at most total and 65535 (a grid dimension).
inline int64_t chunk_for(int64_t total, size_t per_plane, size_t cap)
{
    return std::max<int64_t>(1, std::min<int64_t>({total, (int64_t)(cap / per_plane), 65535}));
}

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

    // The slot of the current device and stream st in *out, or ROX_E_HIP / ROX_E_NOMEM with a
    // message that starts with `where`.
    int take(hipStream_t st, const char *where, Slot **out)
    {
        int device = 0;
        const hipError_t e = hipGetDevice(&device);
        if (e != hipSuccess)
            return host_fail(ROX_E_HIP, "%shipGetDevice(&device): %s", where, hipGetErrorString(e));
        *out = get(device, st);
        return *out ? 0 : host_fail(ROX_E_NOMEM, "%sout of host memory", where);
    }

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

// A pinned block the host fills and copies to the device from.  ev is recorded after the last
// copy that reads the block, and the next call waits for it before it writes the block again.
struct Staging {
    char *h = nullptr;
    size_t cap = 0;                 // bytes
    hipEvent_t ev = nullptr;

    // At least `bytes` of h, free to write: the event is made on first use and waited for after.
    // A block too small is replaced by one of `grow` bytes (default: `bytes`).
    hipError_t acquire(size_t bytes, size_t grow = 0)
    {
        hipError_t e = ev ? hipEventSynchronize(ev) : hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e == hipSuccess && cap < bytes) {
            const size_t n = grow ? grow : bytes;
            e = regrow(h, cap, n, n, hipHostMallocDefault);
        }
        return e;
    }

    // after the last copy that reads h
    hipError_t record(hipStream_t st) { return hipEventRecord(ev, st); }
};

// The state of an analysis entry per (device, stream): a grow-only device block and the staging
// of the call's host inputs.
struct Workspace {
    char *buf = nullptr;
    size_t cap = 0;
    Staging stage;

    // at least `need` bytes of buf; a new block (its old contents lost) when it grows
    hipError_t reserve(size_t need) { return cap < need ? regrow(buf, cap, need, need) : hipSuccess; }
};

// One block as consecutive regions, in the order they are added: size() is the block's bytes and
// carve(base) points each region's pointer into the block at base.
class Layout {
  public:
    template <class T>
    Layout &add(T *&p, size_t bytes)
    {
        assert(n_ < kMaxRegions);
        regions_[n_++] = {&p, bytes, [](void *q, char *at) { *static_cast<T **>(q) = reinterpret_cast<T *>(at); }};
        size_ += bytes;
        return *this;
    }
    size_t size() const { return size_; }
    void carve(char *base) const
    {
        for (int i = 0; i < n_; ++i) {
            regions_[i].set(regions_[i].p, base);
            base += regions_[i].bytes;
        }
    }

  private:
    static constexpr int kMaxRegions = 16;
    struct Region {
        void *p;
        size_t bytes;
        void (*set)(void *p, char *at);
    };
    Region regions_[kMaxRegions];
    int n_ = 0;
    size_t size_ = 0;
};

// An entry's turn on its state T of the current device and stream st: take() finds the slot and
// holds its mutex until the Turn leaves scope.  The Turn then stands for that state (ws->...).
// `where` is the entry's kHipWhere, the prefix of the messages of take() and of the two steps
// below, which spell their HIP calls as the entries did.
template <class T = Workspace>
class Turn {
  public:
    T *ws = nullptr;
    hipStream_t st = nullptr;

    // 0, or ROX_E_HIP / ROX_E_NOMEM as PerStream::take
    int take(PerStream<T> &all, hipStream_t stream, const char *where)
    {
        typename PerStream<T>::Slot *slot;
        ROX_TRY(all.take(stream, where, &slot));
        lock_ = std::unique_lock<std::mutex>(slot->mu);
        ws = &slot->data;
        st = stream;
        where_ = where;
        return 0;
    }
    T *operator->() const { return ws; }

    // The two steps of an entry that stages one block of tables (the packet entries): the device
    // block of L reserved and carved and b_tab bytes of the pinned staging free to write at *h ...
    template <class H>
    int carve(const Layout &L, size_t b_tab, H **h)
    {
        const char *const kHipWhere = where_;
        HIP_TRY(ws->reserve(L.size()));
        L.carve(ws->buf);
        HIP_TRY(ws->stage.acquire(b_tab));
        *h = reinterpret_cast<H *>(ws->stage.h);
        return 0;
    }
    // ... and, once the host has filled them, on their way to d_tab in stream order
    int upload(void *d_tab, size_t b_tab)
    {
        const char *const kHipWhere = where_;
        const char *h = ws->stage.h;
        HIP_TRY(hipMemcpyAsync(d_tab, h, b_tab, hipMemcpyHostToDevice, st));
        HIP_TRY(ws->stage.record(st));
        return 0;
    }

  private:
    std::unique_lock<std::mutex> lock_;
    const char *where_ = "";
};

}  // namespace rox
