// roxtrace.hip -- host side of libroxtrace.so: the C ABI of include/roxtrace.h
// (+ the measurement helpers of include/roxtrace_diag.h) over the gfx950 trace
// kernels of rox_device.hpp, plus the two small kernels that are not part of
// the per-ray trace (pupil axes, fp64 self-test).
//
//   rox_trace_rays / rox_trace_pupil_grid / rox_trace_pupil_list
//       -> trace_kernel<OUT_MODE, GEN, PER_RAY_WVL, FEAT>  (csrc/inst_*.hip)
//   rox_aim_chief_rays -> aim_kernel                          (csrc/rox_search.hpp, search_*.hip)
//   rayoptics/raytr/trace.py:563-605, 537-560 grid / fan pupil coordinates
//       -> pupil_axes_kernel (repeated +=)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <mutex>
#include <new>
#include <vector>

#include "rox_device.hpp"
#include "rox_host.hpp"
#include "../../include/roxtrace_diag.h"

#pragma clang fp contract(off)

using namespace rox;

namespace {

// trace.py:563-605 / 537-560: pupil coordinates by repeated `+=` of the step.
// lane 0 walks the x axis, lane 1 the y axis (both are sequential by
// definition: k-th value = start after k separately rounded additions).
__global__ void pupil_axes_kernel(double x0, double y0, double sx, double sy, int num,
                                  double *px, double *py)
{
    if (threadIdx.x > 1)
        return;
    double v = threadIdx.x == 0 ? x0 : y0;
    const double step = threadIdx.x == 0 ? sx : sy;
    double *out = threadIdx.x == 0 ? px : py;
    for (int k = 0; k < num; ++k) {
        out[k] = v;
        v += step;
    }
}

// ... the axes of several grid definitions at once (rox_trace_through_focus[_grids]): thread 2 s
// walks slot s's x axis and thread 2 s + 1 its y axis, prm[s] = (x0, y0, sx, sy), into
// axes[s][2][num] -- each value the same repeated `+=` as pupil_axes_kernel's
__global__ void pupil_axes_slots_kernel(const double *prm, int n_slots, int num, double *axes)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * n_slots)
        return;
    const int s = t >> 1, ax = t & 1;
    double v = prm[4 * s + ax];
    const double step = prm[4 * s + 2 + ax];
    double *out = axes + ((size_t)s * 2 + ax) * num;
    for (int k = 0; k < num; ++k) {
        out[k] = v;
        v += step;
    }
}

// Diagnostic: the slim fp64 paths against the plain operators on pseudo-random
// operands spanning the whole exponent range (zeros, denormals, band edges,
// inf and nan included).  counts[0] = sqrt mismatches, counts[1] = division
// mismatches, counts[2] = operand sets that took a slim path, counts[3] = the
// same for the band-edge classes.
__device__ __forceinline__ uint64_t mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ double with_exponent(uint64_t bits, uint64_t e)
{
    return __longlong_as_double((long long)((bits & 0x800fffffffffffffull) | (e << 52)));
}

// operand `slot` (0..2 numerators, 3 divisor) of class `kind`; every class is
// wave-uniform, so that the wave-uniform slim branch is decided by the class
__device__ __forceinline__ double test_operand(uint64_t bits, int kind, int slot)
{
    switch (kind) {
    case 0:                                         // any bit pattern
        return __longlong_as_double((long long)bits);
    case 1:                                         // 2^-40 .. 2^40 (the common case)
        return with_exponent(bits, 1023 - 40 + (bits >> 52) % 80);
    case 2: {                                       // specials
        const double sp[] = {0.0, -0.0, 1.0, -1.0, 4.9e-324, 2.2250738585072014e-308,
                             0x1p-383, 0x1.fffffffffffffp-384, 0x1p385, 0x1.fffffffffffffp384,
                             1.7976931348623157e308, __builtin_inf(), -__builtin_inf(),
                             __builtin_nan(""), 0x1p-767, 3.0};
        return sp[bits % 16];
    }
    case 3:                                         // every lane at the band's edges
        return with_exponent(bits, (bits >> 52) & 1 ? ((bits >> 53) & 1 ? 640 : 641)
                                                    : ((bits >> 53) & 1 ? 1406 : 1407));
    case 4:                                         // exponent spread 767: numerators at the
        if (slot < 3)                               // bottom, divisor at the top (and +-0 mixed in)
            return (bits >> 60) == 0 ? ((bits >> 59) & 1 ? -0.0 : 0.0) : with_exponent(bits, 640);
        return with_exponent(bits, 1407);
    case 5:                                         // the other way round
        if (slot < 3)
            return (bits >> 60) == 0 ? ((bits >> 59) & 1 ? -0.0 : 0.0) : with_exponent(bits, 1407);
        return with_exponent(bits, 640);
    default:                                        // one step outside the band: must fall back
        return with_exponent(bits, (bits >> 52) & 1 ? 639 : 1408);
    }
}

__device__ __forceinline__ bool same_bits(double a, double b)
{
    return __double_as_longlong(a) == __double_as_longlong(b) || (a != a && b != b);
}

__global__ void __launch_bounds__(kBlock) selftest_kernel(uint64_t n, uint64_t seed,
                                                           unsigned long long *counts)
{
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * kBlock) {
        // one operand class per wave: half the waves the common case, the rest
        // cycling through the other classes
        const uint64_t wv = i / 64;
        const int kind = (wv & 1) ? 1 : (int)((wv >> 1) % 7);
        const uint64_t k = i * 4 + seed * 0x9e3779b97f4a7c15ull;
        const double a0 = test_operand(mix64(k), kind, 0), a1 = test_operand(mix64(k + 1), kind, 1);
        const double a2 = test_operand(mix64(k + 2), kind, 2), b = test_operand(mix64(k + 3), kind, 3);
        const double x = fabs(a0);
        if (!same_bits(slim_sqrt(x), sqrt(x)))
            atomicAdd(&counts[0], 1ull);
        const v3 q = slim_div3(v3{a0, a1, a2}, b);
        if (!same_bits(q.x, a0 / b) || !same_bits(q.y, a1 / b) || !same_bits(q.z, a2 / b))
            atomicAdd(&counts[1], 1ull);
        if (!same_bits(slim_div(a1, b), a1 / b))
            atomicAdd(&counts[1], 1ull);
        if (__all(in_band(b) && in_band_or_zero(a0) && in_band_or_zero(a1) && in_band_or_zero(a2))) {
            atomicAdd(&counts[2], 1ull);
            if (kind >= 3)
                atomicAdd(&counts[3], 1ull);
        }
        // unit(): one decision for its sqrt and quotients (the numerators' upper edge is
        // implied by |v_i| <= |v|).  Components of very different magnitudes, some scaled
        // down to the band's lower edge and below, zeros included.
        {
            const double sc[4] = {1.0, 0x1p-200, 0x1p-381, 0x1p-390};
            // (scales are wave-uniform so that whole waves sit on either side of the edge)
            const double k0 = sc[(wv >> 4) & 3], k1 = sc[(wv >> 6) & 3], k2 = sc[(wv >> 8) & 3];
            const v3 w{a0 * k0, (mix64(k + 9) & 7) == 0 ? 0.0 : a1 * k1, a2 * k2};
            const v3 u = unit(w);
            const double len = sqrt(dot3(w, w));
            const v3 r = (len == 0.0) ? w : v3{w.x / len, w.y / len, w.z / len};
            if (!same_bits(u.x, r.x) || !same_bits(u.y, r.y) || !same_bits(u.z, r.z))
                atomicAdd(&counts[1], 1ull);
        }
        // the sqrt-free aperture test: (sqrt(s) <= t) == (s <= sqrt_le_threshold(t)) for s
        // within a few ulps of t*t and far from it (mismatches are counted as sqrt mismatches)
        {
            const double t = (kind == 2) ? a1 : fabs(a1);
            const double thr = sqrt_le_threshold(t);
            const long long k9 = (long long)(mix64(k + 7) % 9) - 4;
            double s2 = t * t;
            if (s2 > 0 && s2 < 1e300)
                s2 = __longlong_as_double(__double_as_longlong(s2) + k9);
            const double cand[3] = {s2, fabs(a2), fabs(a0) * fabs(a0)};
            for (int q = 0; q < 3; ++q)
                if ((sqrt(cand[q]) <= t) != (cand[q] <= thr))
                    atomicAdd(&counts[0], 1ull);
        }
    }
}

// ------------------------------------------------------------------ host side
thread_local char g_err[512] = "";
constexpr char kHipWhere[] = "";        // (HIP_TRY: the messages of the trace entries name no entry)
int (&fail)(int code, const char *fmt, ...) = rox::host_fail;

// Per-stream launch scratch.  Launches on one stream run in stream order, so
// they may share it; two streams (or two host threads on two streams) get two
// contexts, looked up under rox_system::mu.
struct StreamCtx {
    hipStream_t stream = nullptr;
    // pupil axes [2][axes_cap] + the grid definition they currently hold (spot
    // diagrams reuse one grid definition for every field and wavelength: the
    // serial accumulate is skipped when unchanged)
    double *d_axes = nullptr;
    int32_t axes_cap = 0;
    double axes_key[4] = {0, 0, 0, 0};
    int32_t axes_num = 0;
    // HITS_COMPACT: tile states of the decoupled look-back, ticket, running base
    uint64_t *d_tiles = nullptr;
    int64_t tiles_cap = 0;
    uint32_t *d_ticket = nullptr;       // [0] ticket, [1] workgroups done
    int64_t *d_hits_base = nullptr;     // [2] running totals between launches (ping-pong)
    uint32_t epoch = 0;
    // two-pass packed hits: the plain HITS launch's (x, y)[2][pack_cap] and status[pack_cap]
    // (grow-only; launches on one stream run in order, so they share it)
    double *d_pack_xy = nullptr;
    uint8_t *d_pack_status = nullptr;
    int64_t pack_cap = 0;
    // ROX_HOST_POINTERS staging: HBM arena for big batches, device-mapped pinned
    // block for small ones (grow-only)
    char *d_stage = nullptr, *h_stage = nullptr;
    size_t d_stage_cap = 0, h_stage_cap = 0;
    // rox_trace_pupil_grids: the launch items of a batch of MORE than kInlineItems items (smaller
    // batches travel in the kernel argument, rox_device.hpp BatchArgs).  Written into one of kItemSlots
    // pinned slots (a slot is reused only after the copy that read it has completed),
    // copied to d_items in stream order, read by the kernel through scalar loads.
    static constexpr int kItemSlots = 4;
    rox::TraceArgs *d_items = nullptr, *h_items = nullptr;
    int32_t items_cap = 0;
    std::vector<char> items_last;       // the bytes d_items holds (or is about to, in stream order)
    hipEvent_t item_ev[kItemSlots] = {nullptr, nullptr, nullptr, nullptr};
    bool item_ev_live[kItemSlots] = {false, false, false, false};
    uint32_t item_slot = 0;
    uint32_t *d_btickets = nullptr;     // HITS_COMPACT in a batch: [items][2] tickets
    uint64_t *d_btiles = nullptr;       // ... and [items][tiles] look-back states
    int64_t btickets_cap = 0, btiles_cap = 0;
    uint32_t bepoch = 0;
    // rox_trace_through_focus[_grids] (grow-only): the device block -- the pupil axes, then items,
    // planes and axis parameters (copied in one transfer from the pinned block h_focus: the
    // caller's arrays may be pageable and are free to go when the call returns), the statistics
    // and the partial records of one launch
    char *d_focus = nullptr;
    size_t focus_cap = 0;
    Staging h_focus;
    // ... the axis parameters and num of the axes at the head of the block (none after a regrow):
    // a call that repeats them byte for byte does not walk the axes again
    std::vector<double> focus_prm;
    int32_t focus_num = 0;
    // Everything a pupil-grid call does between reading / rewriting the cached axes
    // (prepare_grid) and handing its launches to the stream is one critical section per
    // stream: two host threads enqueueing on the SAME stream take turns (their launches run
    // in stream order anyway); different streams have different contexts and do not meet.
    std::mutex enqueue_mu;
    std::mutex batch_mu;                // one batch enqueue at a time per stream
    std::mutex stage_mu;                // one ROX_HOST_POINTERS call at a time per stream
    std::mutex compact_mu;              // epoch / ticket state: one HITS_COMPACT enqueue at a time
    std::mutex ticket_mu;               // first allocation of d_ticket / d_hits_base
};

}  // namespace

int rox::host_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

struct rox_system {
    int device = 0;
    int32_t n_ifcs = 0, n_wvls = 0;
    std::vector<rox_surface> rows;      // host copy (immutable)
    double *d_rows = nullptr;
    double *d_ntab = nullptr;
    double *d_phc = nullptr;            // [W][N][kPhaseConsts]
    double *d_wvls = nullptr;
    int32_t *d_slots[2] = {nullptr, nullptr};   // [0]: no phantom filtering, [1]: filtered
    int32_t n_seg[2] = {0, 0};
    int num_cus = 256;
    int features = 0;                   // F_* of the table
    int n_newton = 0;                   // interfaces intersected by Newton iteration
    std::mutex mu;                      // guards ctxs
    std::vector<StreamCtx *> ctxs;
    // the small synchronous search entries (aiming, pupil search, vignetting, pupil
    // iterations): one device-mapped pinned block the kernel reads its problems from and
    // writes its answers to -- no allocation, no copy-engine transfer per call (round 4; a
    // call used to be hipMalloc + three hipMemcpyAsync + hipFree around a 10-300 us kernel)
    char *h_search = nullptr;
    size_t h_search_cap = 0;
    std::mutex search_mu;
};

namespace {

StreamCtx *ctx_for(rox_system *sys, hipStream_t st)
{
    std::lock_guard<std::mutex> lock(sys->mu);
    for (StreamCtx *c : sys->ctxs)
        if (c->stream == st)
            return c;
    StreamCtx *c = new (std::nothrow) StreamCtx;
    if (c) {
        c->stream = st;
        sys->ctxs.push_back(c);
    }
    return c;
}

// the per-stream enqueue lock of a pupil-grid call (StreamCtx::enqueue_mu); empty when the
// context cannot be made (the call then fails in prepare_grid with the same condition)
std::unique_lock<std::mutex> enqueue_lock(rox_system *sys, hipStream_t st)
{
    StreamCtx *cx = ctx_for(sys, st);
    return cx ? std::unique_lock<std::mutex>(cx->enqueue_mu) : std::unique_lock<std::mutex>();
}

// room for `bytes` in the system's search block; the caller holds search_mu until its results
// are copied out
int search_block(rox_system *sys, size_t bytes, char *&base)
{
    if (sys->h_search_cap < bytes) {
        size_t cap = size_t(16) << 10;
        while (cap < bytes)
            cap *= 2;
        HIP_TRY(regrow(sys->h_search, sys->h_search_cap, cap, cap, hipHostMallocMapped));
    }
    base = sys->h_search;
    return 0;
}

void slot_map(const rox_system *s, bool filter, std::vector<int32_t> &m, int32_t &n_seg)
{
    const int N = s->n_ifcs;
    m.assign(2 * N, 0);
    int next = 0;
    for (int i = 0; i < N; ++i) {
        // a phantom's segment is dropped when the *following* surface sees
        // b4_interact_mode == 'phantom' (raytrace.py:185-188); the last
        // interface has no follower, and the object is 'dummy' unless
        // intersect_obj reads its own mode
        const bool filtered = filter && s->rows[i].mode == ROX_PHANTOM && i > 0 && i < N - 1;
        m[N + i] = next;                // nslots_before[i]
        m[i] = filtered ? -1 : next++;
    }
    n_seg = next;
}

// (rox_device.hpp trace_tiles: the LDS layout of a workgroup; gtab = the table and the phase
// constants stay in global memory, the circular clear-aperture thresholds get an array)
size_t lds_bytes(const rox_system *s, bool per_ray_wvl, bool phase, bool fast, bool gtab = false,
                 bool aplist = false)
{
    const size_t N = s->n_ifcs, Wn = per_ray_wvl ? (size_t)s->n_wvls : 1;
    size_t b = (gtab ? 0 : N * sizeof(dev_surface)) + Wn * N * sizeof(double) +
               ((phase && !gtab) ? Wn * N * kPhaseConsts * sizeof(double) : 0) +
               ((gtab && aplist) ? N * ROX_MAX_AP * sizeof(double) : 0) +
               ((size_t)s->n_wvls + N) * sizeof(double) + 2 * N * sizeof(int32_t);
    if (fast)       // (mu, mu^2, sg) per (wavelength row, interface) behind the slot map
        b += Wn * 3 * N * sizeof(double);
    return (b + 15) & ~size_t(15);
}

// ROX_FAST_FP64 is a permission, taken where it buys something: the reduced-output modes (bound
// by VALU issue) always, FULL packets where the system makes them VALU-bound too (below).
// ROX_FAST_FP64_DISABLE=1 (read once) ignores the flag everywhere: an A/B switch for callers
// that set it by default.
bool use_fast(const rox_system *sys, const rox_opts &o)
{
    static const bool off = [] {
        const char *e = getenv("ROX_FAST_FP64_DISABLE");
        return e && *e && atoi(e) != 0;
    }();
    // FULL packets: the tolerance-mode kernels write them too (trace_ray_fast), and the host sends
    // a launch there where that pays -- systems whose interfaces are mostly aspheres (the same
    // test that picks their FULL workgroup, want_small()): there the FULL kernel is bound by the
    // Spencer-Murty arithmetic (phone lens, 8 aspheres in 12: 265 -> 208-212 us per 2^20 rays).
    // Everywhere else FULL is bound by its stores, which the shorter arithmetic only bunches up
    // (double Gauss 190.9 -> 200.1, .zmx zoom 191.9 -> 197.3; Nikkor 447.7 -> 440.6, lithography
    // lens 675.6 -> 670.2): those launches keep the exact kernels -- bit-exact is within any
    // tolerance.  Never under ROX_FILTER_PHANTOMS (the late append of a filtered segment is not
    // in trace_ray_fast).  ROX_FAST_FP64_FULL=0 / 1 (read once): never / wherever possible (A/B).
    static const int full_env = [] {
        const char *e = getenv("ROX_FAST_FP64_FULL");
        return (e && *e) ? (atoi(e) != 0 ? 1 : 0) : -1;
    }();
    if (!(o.flags & ROX_FAST_FP64) || off)
        return false;
    if (o.out_mode != ROX_OUT_FULL)
        return true;
    if ((o.flags & ROX_FILTER_PHANTOMS) || full_env == 0)
        return false;
    return full_env == 1 || sys->n_newton * 4 > sys->n_ifcs - 1;
}

int check_opts(const rox_system *sys, const rox_opts *o, const rox_out *out, int64_t n_rays)
{
    if (!sys || !o || !out)
        return fail(ROX_E_ARG, "null argument");
    if (o->out_mode < ROX_OUT_FULL || o->out_mode > ROX_OUT_FAN)
        return fail(ROX_E_ARG, "bad out_mode %d", o->out_mode);
    if (o->out_mode == ROX_OUT_OPD || o->out_mode == ROX_OUT_FAN) {
        if (sys->n_ifcs < 3)
            return fail(ROX_E_ARG, "OPD output needs at least 3 interfaces");
        if ((o->flags & ROX_FILTER_PHANTOMS) && sys->n_seg[1] != sys->n_seg[0])
            return fail(ROX_E_UNSUPPORTED, "OPD output with filter_out_phantoms");
        if (!(o->wf.ref_radius != 0.0))
            return fail(ROX_E_ARG, "OPD output needs rox_opts.wf (ref_radius is 0)");
        if (o->wf.kind < ROX_WF_FINITE || o->wf.kind > ROX_WF_INF_SPLIT)
            return fail(ROX_E_ARG, "bad rox_wavefront.kind %d", o->wf.kind);
    }
    if (o->out_mode == ROX_OUT_HITS_COMPACT) {
        if (!out->n_hits)
            return fail(ROX_E_ARG, "HITS_COMPACT output needs rox_out.n_hits");
        if (o->flags & ROX_HOST_POINTERS)
            return fail(ROX_E_ARG, "HITS_COMPACT writes device or device-mapped pinned host "
                                   "memory directly: do not set ROX_HOST_POINTERS");
        // rox_out.ld = capacity of seg in (x, y) pairs.  A call that does not append can need
        // up to n_rays of them; an appending call is clamped by the kernel (n_hits < 0)
        if (!(o->flags & ROX_HITS_APPEND) && out->ld < n_rays)
            return fail(ROX_E_ARG, "HITS_COMPACT: out.ld (%lld pairs of room) < n_rays (%lld)",
                        (long long)out->ld, (long long)n_rays);
        if (out->ld < 0)
            return fail(ROX_E_ARG, "HITS_COMPACT: negative out.ld");
    } else if (out->ld < n_rays) {
        return fail(ROX_E_ARG, "out.ld (%lld) < n_rays (%lld)", (long long)out->ld, (long long)n_rays);
    } else if (o->flags & ROX_HITS_APPEND) {
        return fail(ROX_E_ARG, "ROX_HITS_APPEND goes with ROX_OUT_HITS_COMPACT only");
    }
    if (!out->seg && n_rays > 0)
        return fail(ROX_E_ARG, "out.seg is null");
    if ((o->flags & ROX_FILTER_PHANTOMS) && sys->rows[0].mode == ROX_PHANTOM)
        return fail(ROX_E_UNSUPPORTED, "phantom object surface with filter_out_phantoms");
    return 0;
}

// workgroups per CU of a launch of `bs`-thread workgroups (the rest of the batch is
// grid-strided).  ROX_BLOCKS_PER_CU overrides it for experiments.
int blocks_per_cu(int bs)
{
    static const int v = [] {
        const char *e = getenv("ROX_BLOCKS_PER_CU");
        return e ? atoi(e) : 0;
    }();
    return v > 0 ? v : 32 * 256 / bs;      // measured: FULL 238 us at 8/CU, 228 us at 32/CU (256 threads)
}

// HITS_COMPACT: workgroups per CU.  Tiles are drawn by ticket, so any number of workgroups
// finishes the launch; a CU holds exactly one 1024-thread workgroup of these instances, and one
// persistent workgroup per CU that draws its four tiles in turn (table staged once, no
// workgroup start-up between tiles) measured 146 us per 2^20 rays into HBM against 159 us
// for one workgroup per tile (nine appended grids: 1.36 vs 1.49 ms; two per CU 1.40).
// ROX_COMPACT_BLOCKS_PER_CU overrides it for experiments.
int compact_blocks_per_cu()
{
    static const int v = [] {
        const char *e = getenv("ROX_COMPACT_BLOCKS_PER_CU");
        return e ? atoi(e) : 0;
    }();
    return v > 0 ? v : 1;
}

// rays per kernel launch (lane byte offsets are 32-bit: at most 2^28).
// ROX_RAYS_PER_LAUNCH overrides it (tests exercise the chunked path with it).
// HITS_COMPACT: how many first tickets take small tiles (rox_device.hpp compact_tiles).
// A launch that small tiles spread over no more workgroups than the chip has CUs (a
// 256 x 256 grid: 256 tiles of 256 rays instead of 64 of 1024) runs all of it that way:
// 30 vs 40 us into HBM, 41 vs 53 us into pinned memory.  Larger launches take full tiles
// throughout: small first tiles measured slower there (1024 x 1024: 178 vs 158 us into HBM,
// 319 vs 301 us into pinned memory; 45 x 1M rays of config 5: 26.3 vs 23.1 ms).
// ROX_COMPACT_SMALL_TILES overrides the count for experiments.
int32_t compact_small_want(const rox_system *sys, int64_t n_rays)
{
    static const int v = [] {
        const char *e = getenv("ROX_COMPACT_SMALL_TILES");
        return e ? atoi(e) : -1;
    }();
    if (v >= 0)
        return v;
    return n_rays <= (int64_t)sys->num_cus * kSmallTile ? sys->num_cus : 0;
}

int64_t rays_per_launch()
{
    static const int64_t v = [] {
        const char *e = getenv("ROX_RAYS_PER_LAUNCH");
        const long long n = e ? atoll(e) : 0;
        return (n > 0 && n <= (1LL << 28)) ? (int64_t)n : (int64_t(1) << 28);
    }();
    return v;
}

// the leanest compiled instance that covers `need` (index into kInstances).
// ROX_FORCE_INSTANCE=<index> (experiments: what a richer instance costs on a plain table) is
// honoured when that instance covers the need.
int pick_instance(int need)
{
    const int n = (int)(sizeof kInstances / sizeof kInstances[0]);
    static const int forced = [] {
        const char *e = getenv("ROX_FORCE_INSTANCE");
        return (e && *e) ? atoi(e) : -1;
    }();
    if (forced >= 0 && forced < n && (need & ~kInstances[forced]) == 0)
        return forced;
    for (int i = 0; i < n; ++i)
        if ((need & ~kInstances[i]) == 0)
            return i;
    return n - 1;
}

// Workgroup size of a launch (rox_device.hpp block_of()), measured rule
// (profiles/r05_block_rule.jsonl, tools/block_rule_sweep.py):
//  * FULL packets (1024-thread workgroups, one per CU, whose waves write packet rows in step
//    -- worth 13-23 % of the store rate on launches that fill the chip): a launch of at most
//    four rounds of such workgroups that would leave >= 30 % of its CU-rounds idle -- 64
//    workgroups (256^2 rays: 75 %), BASELINE configs[3]'s 320 on 256 CUs (two rounds, 37.5 %)
//    -- runs in ROX_BLOCK_SMALL-thread workgroups instead,
//    five of which fit a CU (256^2: 49 -> 29 us, configs[3]: 43.6 -> 34.0 us per pass);
//  * the reduced-output modes (512-thread workgroups): small workgroups up to kSmallWavesPerCu
//    waves per CU (configs[3]: 25.8 -> 23.9 us, 3 x 256^2: 43 -> 37 us), equal beyond, 3 % worse
//    at 2^20 rays.
// ROX_SMALL_BLOCKS=0 / 1 forces one form, ROX_SMALL_WAVES_PER_CU moves the second threshold.
constexpr int kSmallWavesPerCu = 24;
bool want_small(const rox_system *sys, int64_t total_rays, int out_mode, int feat, int64_t n_items = 1)
{
    static const int forced = [] {
        const char *e = getenv("ROX_SMALL_BLOCKS");
        return (e && *e) ? atoi(e) : -1;
    }();
    static const int per_cu = [] {
        const char *e = getenv("ROX_SMALL_WAVES_PER_CU");
        return (e && *e && atoi(e) > 0) ? atoi(e) : kSmallWavesPerCu;
    }();
    if (forced == 0 || forced == 1)
        return forced == 1;
    if (out_mode == ROX_OUT_FULL) {
        const int64_t big = block_of(ROX_OUT_FULL, feat, false);
        if (big <= ROX_BLOCK_SMALL)
            return false;
        // Newton instances: a workgroup waits at every surface for its slowest wave, and the
        // iteration counts differ per wave.  Where aspheres are a minority of the interfaces
        // the large workgroup's packet rows still win (the .zmx zoom, one asphere in 12: 209
        // -> 192 us per 2^20 rays; Nikkor, 4 in 28: 471 -> 445); where they are most of the
        // system small workgroups out of step with each other do (phone lens, 8 in 12: 263
        // against 288 us).  profiles/r05_full_block_newton.txt.
        if ((feat & kFeatNewton) && sys->n_newton * 4 > sys->n_ifcs - 1)
            return true;
        const int64_t per_item = (total_rays / n_items + big - 1) / big;
        const int64_t wgs = per_item * n_items, cus = sys->num_cus;
        const int64_t rounds = (wgs + cus - 1) / cus;
        const int64_t idle = rounds * cus - wgs;
        return rounds <= 4 && idle * 10 >= 3 * rounds * cus;
    }
    return (total_rays + 63) / 64 <= (int64_t)sys->num_cus * per_cu;
}

// ---- the search kernels (csrc/rox_search.hpp): the leanest instance of kSearchInstances that
// covers the system's features -- their trial rays never filter phantoms
int pick_search_instance(const rox_system *sys)
{
    const int n = (int)(sizeof kSearchInstances / sizeof kSearchInstances[0]);
    for (int i = 0; i < n; ++i)
        if ((sys->features & ~kSearchInstances[i]) == 0)
            return i;
    return n - 1;
}

// surface table + index table + phase constants + wavelengths + slot map + the vignetting
// search's aperture thresholds
constexpr size_t kLdsLimit = 160 * 1024 - 64;
// (rox_search.hpp search_ctx(); gtab: the table and the phase constants stay in global memory,
// the circular clear-aperture thresholds of the checked trace get an array)
size_t search_lds_bytes(size_t N, size_t W, bool gtab = false)
{
    return ((gtab ? N * ROX_MAX_AP * sizeof(double)
                  : N * sizeof(dev_surface) + W * N * sizeof(double) * kPhaseConsts) +
            W * N * sizeof(double) + W * sizeof(double) + 2 * N * sizeof(int32_t) + N * sizeof(double) + 15) &
           ~size_t(15);
}

// the LDS need of a search launch; gtab = the system's table does not fit the LDS of a
// workgroup: the general instance over the table in global memory (search_general_gtab.hip)
int search_lds(const rox_system *sys, size_t &lds, bool &gtab)
{
    const size_t N = sys->n_ifcs, W = sys->n_wvls;
    static const bool force_gtab = [] {
        const char *e = getenv("ROX_FORCE_GTAB");
        return e && *e && atoi(e) != 0;
    }();
    lds = search_lds_bytes(N, W);
    gtab = lds > kLdsLimit || force_gtab;
    if (gtab) {
        lds = search_lds_bytes(N, W, true);
        if (lds > kLdsLimit)
            return fail(ROX_E_UNSUPPORTED, "%zu interfaces x %zu wavelengths need %zu B of LDS for their "
                                           "indices and thresholds alone (max %zu)", N, W, lds, kLdsLimit);
    }
    return 0;
}

// the entry points of the search instance a launch takes (gtab: search_lds found the table too
// large for the LDS)
const SearchInstanceFns &search_fns(const rox_system *sys, bool gtab)
{
#define ROX_SEARCH_FNS(name, FEAT) &search_##name,
    static const SearchInstanceFns *const fns[] = {ROX_SEARCH_INSTANCES(ROX_SEARCH_FNS)};
#undef ROX_SEARCH_FNS
    return gtab ? search_general_gtab : *fns[pick_search_instance(sys)];
}

// the entry points of trace instance kInstances[inst] -- or of its tolerance-mode twin, or of the
// general instance over a table in global memory -- as launch_setup chose in k
const TraceInstanceFns &trace_fns(int inst, const LaunchCfg &k)
{
#define ROX_TRACE_FNS(name, FEAT) &trace_##name,
#define ROX_TRACE_FAST_FNS(name, FEAT) &trace_##name##_fast,
    static const TraceInstanceFns *const fns[] = {ROX_TRACE_INSTANCES(ROX_TRACE_FNS)};
    static const TraceInstanceFns *const fast[] = {ROX_TRACE_INSTANCES(ROX_TRACE_FAST_FNS)};
#undef ROX_TRACE_FNS
#undef ROX_TRACE_FAST_FNS
    return k.gtab ? trace_general_gtab : *(k.fast ? fast : fns)[inst];
}

// (initialisations are enqueued on the launch stream itself: a stream created with
// hipStreamNonBlocking is not ordered after NULL-stream memsets)
// the stream context's ticket words (HITS_COMPACT tiles and the pack pass: launches of one
// stream run in order and each leaves them zero)
int ensure_ticket(StreamCtx *cx, hipStream_t st)
{
    std::lock_guard<std::mutex> g(cx->ticket_mu);
    if (!cx->d_ticket) {
        uint32_t *t = nullptr;
        int64_t *b = nullptr;
        HIP_TRY(hipMalloc(&t, 2 * sizeof(uint32_t)));
        HIP_TRY(hipMemsetAsync(t, 0, 2 * sizeof(uint32_t), st));
        HIP_TRY(hipMalloc(&b, 2 * sizeof(int64_t)));
        HIP_TRY(hipMemsetAsync(b, 0, 2 * sizeof(int64_t), st));
        cx->d_hits_base = b;
        cx->d_ticket = t;
    }
    return 0;
}

int ensure_compact(StreamCtx *cx, int64_t tiles, hipStream_t st)
{
    int rc = ensure_ticket(cx, st);
    if (rc)
        return rc;
    if (tiles > cx->tiles_cap) {
        HIP_TRY(regrow_zeroed(cx->d_tiles, cx->tiles_cap, tiles, sizeof(uint64_t) * (size_t)tiles, st));
        cx->epoch = 0;
    }
    return 0;
}

// Packed hits in two passes -- the unsynchronised HITS instance into a scratch, then the
// streaming pack kernel (csrc/pack.hip) -- instead of the fused tile-synchronous instance.
// The fused instance pays three workgroup barriers and a look-back per 1024-ray tile with
// one workgroup per CU; that is the cheaper form while a tile's waves finish together
// (shallow spherical systems) and while the destination sits behind PCIe (the pairs cross
// the link while later tiles are traced).  On deep tables and Newton instances the waves
// finish far apart and the plain HITS launch + a ~17 B/ray pack pass wins: measured
// crossover in profiles/r04_pack_crossover.jsonl (tools/pack_bench.py).
// ROX_PACK_TWO_PASS=0 / 1 forces one form (experiments, tests).
std::atomic<uint64_t> g_two_pass_launches{0}, g_fused_pack_launches{0};
constexpr int64_t kTwoPassMinRays = 1 << 16;
constexpr int64_t kTwoPassChunk = int64_t(1) << 24;     // rays per launch of the two-pass form
bool want_two_pass(const rox_system *sys, int inst, int64_t n_rays, const void *dst)
{
    const char *e = getenv("ROX_PACK_TWO_PASS");        // (read per call: tests flip it)
    const int forced = (e && *e) ? atoi(e) : -1;
    if (forced == 0 || forced == 1)
        return forced == 1;
    (void)sys;
    (void)inst;
    return n_rays >= kTwoPassMinRays && is_device(dst);
}

int ensure_pack_scratch(StreamCtx *cx, int64_t rays, bool need_status)
{
    const int64_t want = (rays + 511) & ~int64_t(511);
    if (want > cx->pack_cap) {
        HIP_TRY(release(cx->d_pack_status, cx->pack_cap));      // (made again below, on demand)
        HIP_TRY(regrow(cx->d_pack_xy, cx->pack_cap, want, sizeof(double) * 2 * (size_t)want));
    }
    if (need_status && !cx->d_pack_status)
        HIP_TRY(hipMalloc(&cx->d_pack_status, (size_t)cx->pack_cap));
    return 0;
}

// the table pointers of a launch, the leanest kernel instance that covers this system and
// these options, and its LDS need
int launch_setup(rox_system *sys, TraceArgs &a, int gen, bool prw, hipStream_t st, LaunchCfg &k,
                 int &inst)
{
    a.rows = sys->d_rows;
    a.n_table = sys->d_ntab;
    a.ph_consts = sys->d_phc;
    a.wvls = sys->d_wvls;
    a.slots = sys->d_slots[(a.opts.flags & ROX_FILTER_PHANTOMS) ? 1 : 0];
    a.n_ifcs = sys->n_ifcs;
    a.n_wvls = sys->n_wvls;
    int need = sys->features;
    if ((a.opts.flags & ROX_FILTER_PHANTOMS) && sys->n_seg[1] != sys->n_seg[0])
        need |= F_PHFILT;
    k.gen = gen;
    k.per_ray_wvl = prw;
    k.small = false;
    k.n_inline = 0;
    k.fast = use_fast(sys, a.opts);
    k.out_mode = a.opts.out_mode;
    k.stream = st;
    inst = pick_instance(need);
    // (an instance compiled with F_PHASE stages the phase constants, needed or not)
    const size_t stash = a.opts.out_mode == ROX_OUT_HITS_COMPACT    // two tiles of packed pairs (rox_device.hpp)
                             ? 16 + 2 * 16 * (size_t)block_of(ROX_OUT_HITS_COMPACT, kInstances[inst]) : 0;
    const bool fast_gtab = gtab_of(kInstances[inst], k.fast, a.opts.out_mode) != 0;   // (this kernel's own table source)
    k.gtab = false;
    k.lds = lds_bytes(sys, prw, (kInstances[inst] & F_PHASE) != 0, k.fast, fast_gtab,
                      (kInstances[inst] & F_APLIST) != 0) + stash;
    // A table that does not fit the LDS of a workgroup (~220 interfaces at 736 B a row) is traced
    // by the general instance that leaves it in global memory and reads it with scalar loads
    // (F_GTAB; bit-identical, every output mode): SequentialModel has no size limit either.
    // ROX_FORCE_GTAB=1 sends every launch there (tests; read once).
    static const bool force_gtab = [] {
        const char *e = getenv("ROX_FORCE_GTAB");
        return e && *e && atoi(e) != 0;
    }();
    if (k.lds > kLdsLimit || force_gtab) {
        inst = (int)(sizeof kInstances / sizeof kInstances[0]) - 1;
        k.fast = false;
        k.gtab = true;
        k.lds = lds_bytes(sys, prw, true, false, true, true) +
                (a.opts.out_mode == ROX_OUT_HITS_COMPACT
                     ? 16 + 2 * 16 * (size_t)block_of(ROX_OUT_HITS_COMPACT, kInstances[inst]) : 0);
        if (k.lds > kLdsLimit)
            return fail(ROX_E_UNSUPPORTED, "%d interfaces x %d wavelengths need %zu B of LDS for their "
                                           "indices and thresholds alone (max %zu)",
                        sys->n_ifcs, prw ? sys->n_wvls : 1, k.lds, kLdsLimit);
    }
    return 0;
}

int launch(rox_system *sys, TraceArgs &a, int gen, hipStream_t st)
{
    if (a.opts.out_mode == ROX_OUT_HITS_COMPACT && a.n_rays == 0) {
        // nothing to trace: the count is still owed (appending nothing leaves it as it is)
        if (!(a.opts.flags & ROX_HITS_APPEND))
            HIP_TRY(hipMemsetAsync(a.out.n_hits, 0, sizeof(int64_t), st));
        return 0;
    }
    if (a.n_rays == 0)
        return 0;
    const bool prw = a.wvl_idx != nullptr;
    LaunchCfg k;
    int inst;
    int rc0 = launch_setup(sys, a, gen, prw, st, k, inst);
    if (rc0)
        return rc0;
    // lane byte offsets are 32-bit: at most 2^28 rays per launch
    const int64_t total = a.n_rays;
    int64_t chunk_max = rays_per_launch();
    k.small = !prw && want_small(sys, total, a.opts.out_mode, kInstances[inst]);   // (per-ray-wavelength lists keep the regular kernels)
    const bool compact = a.opts.out_mode == ROX_OUT_HITS_COMPACT;
    StreamCtx *cx = nullptr;
    bool two_pass = false;
    // two host threads enqueueing HITS_COMPACT launches on one stream take turns with the
    // stream's epoch / ticket / tile-state words (the launches themselves run in stream order)
    std::unique_lock<std::mutex> compact_lock;
    if (compact) {
        cx = ctx_for(sys, st);
        if (!cx)
            return fail(ROX_E_NOMEM, "out of host memory");
        compact_lock = std::unique_lock<std::mutex>(cx->compact_mu);
        const int tb = block_of(ROX_OUT_HITS_COMPACT, kInstances[inst]);
        two_pass = want_two_pass(sys, inst, total, a.out.seg);
        if (two_pass) {
            // the scratch of the two passes is 17 B per ray of one launch: launches of at most
            // kTwoPassChunk rays bound it (272 MiB) whatever the call's size; the running base
            // carries the packed order across the launches exactly as it does across 2^28-ray
            // chunks.  Should the scratch still not be had, the fused instance -- which needs
            // none -- takes the call.
            if (chunk_max > kTwoPassChunk)
                chunk_max = kTwoPassChunk;
            const int64_t per2 = total < chunk_max ? total : chunk_max;
            if (ensure_pack_scratch(cx, per2, a.out.status == nullptr) != 0) {
                (void)hipGetLastError();
                two_pass = false;
                chunk_max = rays_per_launch();
            }
        }
        const int64_t per = total < chunk_max ? total : chunk_max;
        a.small_tiles = two_pass ? 0 : compact_small_want(sys, per);
        int rc = ensure_compact(cx, two_pass ? (per + kPackTile - 1) / kPackTile
                                             : compact_tiles(per, a.small_tiles, tb), st);
        if (rc)
            return rc;
    }
    const rox_out out0 = a.out;
    a.in_ld = total;
    // HITS_COMPACT: launch c reads its base from slot[(c + 1) & 1] and leaves the running total
    // in slot[c & 1]; the first launch starts from zero, or -- ROX_HITS_APPEND -- from the
    // caller's count, copied into slot[1] first (device or device-mapped host memory)
    const bool append = compact && (a.opts.flags & ROX_HITS_APPEND);
    if (append)
        HIP_TRY(hipMemcpyAsync(cx->d_hits_base + 1, out0.n_hits, sizeof(int64_t), hipMemcpyDefault, st));
    int64_t n_launch = 0;
    for (int64_t base = 0; base < total; base += chunk_max, ++n_launch) {
        a.ray_base = base;
        a.n_rays = total - base < chunk_max ? total - base : chunk_max;
        if (compact) {
            a.tile_state = cx->d_tiles;
            a.ticket = cx->d_ticket;
            a.hits_base_in = (n_launch == 0 && !append) ? nullptr : cx->d_hits_base + ((n_launch + 1) & 1);
            a.hits_total_out = (base + chunk_max >= total) ? out0.n_hits : cx->d_hits_base + (n_launch & 1);
            a.epoch = ++cx->epoch;
            a.out.status = out0.status ? out0.status + base : nullptr;
        } else {
            a.out.seg = out0.seg + base;
            a.out.op = out0.op ? out0.op + base : nullptr;
            a.out.status = out0.status ? out0.status + base : nullptr;
            a.out.fail_surf = out0.fail_surf ? out0.fail_surf + base : nullptr;
            a.out.pupil = out0.pupil ? out0.pupil + base : nullptr;
        }
        if (compact)
            (two_pass ? g_two_pass_launches : g_fused_pack_launches).fetch_add(1, std::memory_order_relaxed);
        if (two_pass) {
            // pass 1: the plain HITS instance of the same rays into the scratch rows
            TraceArgs h = a;
            h.opts.out_mode = ROX_OUT_HITS;
            h.opts.flags &= ~(uint32_t)ROX_HITS_APPEND;
            h.out.seg = cx->d_pack_xy;
            h.out.ld = cx->pack_cap;
            h.out.op = nullptr;
            h.out.fail_surf = nullptr;
            h.out.pupil = nullptr;
            h.out.n_hits = nullptr;
            h.out.status = out0.status ? out0.status + base : cx->d_pack_status;
            LaunchCfg kh = k;
            kh.out_mode = ROX_OUT_HITS;
            kh.lds = k.gtab ? lds_bytes(sys, prw, true, false, true, true)
                            : lds_bytes(sys, prw, (kInstances[inst] & F_PHASE) != 0, kh.fast,
                                        gtab_of(kInstances[inst], kh.fast, ROX_OUT_HITS) != 0,
                                        (kInstances[inst] & F_APLIST) != 0);
            const int hb = block_of(ROX_OUT_HITS, kInstances[inst], kh.small);
            int64_t hblocks = (a.n_rays + hb - 1) / hb;
            const int64_t hcap = (int64_t)sys->num_cus * blocks_per_cu(hb);
            kh.grid = dim3((unsigned)(hblocks > hcap ? hcap : hblocks));
            trace_fns(inst, kh).launch(kh, h);
            // pass 2: survivors to their final place, in ray order
            PackArgs p;
            p.status = h.out.status;
            p.xy = cx->d_pack_xy;
            p.ld = cx->pack_cap;
            p.n_rays = a.n_rays;
            p.tile_state = a.tile_state;
            p.ticket = a.ticket;
            p.hits_base_in = a.hits_base_in;
            p.hits_total_out = a.hits_total_out;
            p.epoch = a.epoch;
            p.dst = out0.seg;
            p.ld_dst = out0.ld;
            int64_t pblocks = (a.n_rays + kPackTile - 1) / kPackTile;
            const int64_t pcap = (int64_t)sys->num_cus * 2;
            launch_pack(p, (unsigned)(pblocks > pcap ? pcap : pblocks), st);
            continue;
        }
        // enough workgroups to fill 256 CUs several times over, grid-stride the rest
        const int bs = block_of(a.opts.out_mode, kInstances[inst], k.small);
        int64_t blocks = compact ? compact_tiles(a.n_rays, a.small_tiles, bs) : (a.n_rays + bs - 1) / bs;
        const int64_t cap = (int64_t)sys->num_cus * (compact ? compact_blocks_per_cu() : blocks_per_cu(bs));
        if (blocks > cap)
            blocks = cap;
        k.grid = dim3((unsigned)blocks);
        trace_fns(inst, k).launch(k, a);
    }
    a.n_rays = total;
    a.out = out0;
    HIP_TRY(hipGetLastError());
    return 0;
}

int64_t seg_rows(const rox_system *sys, const rox_opts *o)
{
    if (o->out_mode == ROX_OUT_FULL)
        return (int64_t)sys->n_seg[(o->flags & ROX_FILTER_PHANTOMS) ? 1 : 0] * ROX_SEG_DOUBLES;
    if (o->out_mode == ROX_OUT_OPD)
        return 1;
    if (o->out_mode == ROX_OUT_FAN)
        return 3;
    return o->out_mode == ROX_OUT_LAST ? ROX_SEG_DOUBLES : 2;
}

// ROX_HOST_POINTERS.  The caller's buffers are ordinary host memory; they are
// staged through an arena the stream context keeps (grow-only: no allocation per
// call).  Batches of up to kBounceBytes never touch the copy engine: inputs are
// copied into, and results out of, one device-mapped pinned block that the
// kernel reads and writes directly (one launch, one synchronise).  Larger
// batches go through HBM and the runtime's pageable copies.  seg slots the trace
// does not produce come back as NaN (include/roxtrace.h, ROX_HOST_POINTERS).
constexpr size_t kBounceBytes = size_t(4) << 20;

__global__ void fill_nan_kernel(double *p, size_t n)
{
    const double q = __longlong_as_double(0x7ff8000000000000ll);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (size_t)gridDim.x * blockDim.x)
        p[i] = q;
}

struct Staged {
    std::unique_lock<std::mutex> lock;  // holds the stream's staging arena until the call returns
    rox_out dev{};          // staging buffers (device-visible)
    rox_out host{};         // caller's host buffers
    int64_t n = 0, rows = 0;
    bool bounce = false;    // staging lives in the pinned block
    char *in = nullptr;     // room for the staged inputs
};

inline size_t up16(size_t b) { return (b + 15) & ~size_t(15); }

// ROX_HOST_POINTERS calls are synchronous; two host threads on one stream (typically the
// NULL stream of ctypes callers) take turns with the stream's scratch -- the cached pupil
// axes as well as the staging arena -- from before the launch is prepared until the
// results are in place
int stage_lock(Staged &s, rox_system *sys, hipStream_t st)
{
    StreamCtx *cx = ctx_for(sys, st);
    if (!cx)
        return fail(ROX_E_NOMEM, "out of host memory");
    s.lock = std::unique_lock<std::mutex>(cx->stage_mu);
    return 0;
}

int stage_out(Staged &s, rox_system *sys, hipStream_t st, const rox_opts *o, const rox_out *out,
              int64_t n, size_t in_bytes)
{
    StreamCtx *cx = ctx_for(sys, st);
    if (!cx)
        return fail(ROX_E_HIP, "out of host memory");
    s.host = *out;
    s.n = n;
    s.rows = seg_rows(sys, o);
    const size_t N = (size_t)n;
    const size_t b_seg = up16(sizeof(double) * (size_t)s.rows * N), b_in = up16(in_bytes),
                 b_op = out->op ? up16(sizeof(double) * N) : 0,
                 b_st = out->status ? up16(N) : 0,
                 b_fs = out->fail_surf ? up16(sizeof(int16_t) * N) : 0,
                 b_pu = out->pupil ? up16(sizeof(double) * 2 * N) : 0;
    const size_t total = b_seg + b_in + b_op + b_st + b_fs + b_pu + 16;
    s.bounce = total <= kBounceBytes;
    char *base;
    if (s.bounce) {
        if (cx->h_stage_cap < total) {
            size_t cap = size_t(64) << 10;
            while (cap < total)
                cap *= 2;
            HIP_TRY(regrow(cx->h_stage, cx->h_stage_cap, cap, cap, hipHostMallocMapped));
        }
        base = cx->h_stage;
    } else {
        if (cx->d_stage_cap < total) {
            const size_t cap = total + total / 8;
            HIP_TRY(regrow(cx->d_stage, cx->d_stage_cap, cap, cap));
        }
        base = cx->d_stage;
    }
    s.dev.ld = n;
    s.dev.seg = (double *)base;             base += b_seg;
    s.in = base;                            base += b_in;
    if (out->op) { s.dev.op = (double *)base; base += b_op; }
    if (out->status) { s.dev.status = (uint8_t *)base; base += b_st; }
    if (out->fail_surf) { s.dev.fail_surf = (int16_t *)base; base += b_fs; }
    if (out->pupil) { s.dev.pupil = (double *)base; base += b_pu; }
    const size_t n_seg = (size_t)s.rows * N;
    if (s.bounce) {
        std::fill_n(s.dev.seg, n_seg, __builtin_nan(""));
    } else if (n_seg) {
        hipLaunchKernelGGL(fill_nan_kernel, dim3(1024), dim3(256), 0, st, s.dev.seg, n_seg);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// inputs of a ROX_HOST_POINTERS call -> s.in + off
int stage_in(Staged &s, size_t off, const void *src, size_t bytes, hipStream_t st)
{
    if (!bytes)
        return 0;
    if (s.bounce)
        memcpy(s.in + off, src, bytes);
    else
        HIP_TRY(hipMemcpyAsync(s.in + off, src, bytes, hipMemcpyHostToDevice, st));
    return 0;
}

int unstage_out(Staged &s, hipStream_t st)
{
    HIP_TRY(hipStreamSynchronize(st));
    const size_t N = (size_t)s.n;
    if (s.bounce) {
        for (int64_t r = 0; r < s.rows; ++r)
            memcpy(s.host.seg + r * s.host.ld, s.dev.seg + r * s.n, sizeof(double) * N);
        if (s.host.op)
            memcpy(s.host.op, s.dev.op, sizeof(double) * N);
        if (s.host.status)
            memcpy(s.host.status, s.dev.status, N);
        if (s.host.fail_surf)
            memcpy(s.host.fail_surf, s.dev.fail_surf, sizeof(int16_t) * N);
        if (s.host.pupil)
            for (int r = 0; r < 2; ++r)
                memcpy(s.host.pupil + r * s.host.ld, s.dev.pupil + r * s.n, sizeof(double) * N);
        return 0;
    }
    HIP_TRY(hipMemcpy2D(s.host.seg, sizeof(double) * s.host.ld, s.dev.seg, sizeof(double) * s.n,
                        sizeof(double) * s.n, s.rows, hipMemcpyDeviceToHost));
    if (s.host.op)
        HIP_TRY(hipMemcpy(s.host.op, s.dev.op, sizeof(double) * s.n, hipMemcpyDeviceToHost));
    if (s.host.status)
        HIP_TRY(hipMemcpy(s.host.status, s.dev.status, s.n, hipMemcpyDeviceToHost));
    if (s.host.fail_surf)
        HIP_TRY(hipMemcpy(s.host.fail_surf, s.dev.fail_surf, sizeof(int16_t) * s.n,
                          hipMemcpyDeviceToHost));
    if (s.host.pupil)
        HIP_TRY(hipMemcpy2D(s.host.pupil, sizeof(double) * s.host.ld, s.dev.pupil,
                            sizeof(double) * s.n, sizeof(double) * s.n, 2, hipMemcpyDeviceToHost));
    return 0;
}

int ensure_axes(StreamCtx *cx, int32_t num)
{
    if (num <= cx->axes_cap)
        return 0;
    cx->axes_num = 0;
    HIP_TRY(regrow(cx->d_axes, cx->axes_cap, num, sizeof(double) * 2 * (size_t)num));
    return 0;
}

int check_field(const rox_field *fld)
{
    if (!fld)
        return fail(ROX_E_ARG, "null argument");
    if (fld->kind < ROX_FLD_EPD || fld->kind > ROX_FLD_AIM_DIR)
        return fail(ROX_E_ARG, "bad rox_field.kind %d", fld->kind);
    return 0;
}

// the checks of a pupil-grid launch and its arguments, the pupil axes aside (nothing enqueued)
int grid_args(rox_system *sys, const rox_field *fld, const rox_grid *grid, int32_t wvl_idx,
              const rox_opts *opts, const rox_out *out, TraceArgs &a)
{
    if (!grid)
        return fail(ROX_E_ARG, "null argument");
    int rc = check_field(fld);
    if (rc)
        return rc;
    if (grid->num < 1)
        return fail(ROX_E_ARG, "grid.num must be >= 1");
    if (wvl_idx < 0 || wvl_idx >= sys->n_wvls)
        return fail(ROX_E_ARG, "wvl_idx %d out of range", wvl_idx);
    int32_t rows = grid->num, row0 = 0;
    if (grid->kind != ROX_GRID_FAN && grid->row_count > 0) {
        rows = grid->row_count;
        row0 = grid->row_begin;
    }
    if (row0 < 0 || row0 + rows > grid->num)
        return fail(ROX_E_ARG, "grid row block [%d, %d) outside [0, %d)", row0, row0 + rows, grid->num);
    const int64_t R = grid->kind == ROX_GRID_FAN ? grid->num : (int64_t)rows * grid->num;
    rc = check_opts(sys, opts, out, R);
    if (rc)
        return rc;
    a = TraceArgs{};
    a.n_rays = R;
    a.axis_kind = grid->kind == ROX_GRID_FAN ? AXIS_LIST : AXIS_PRODUCT;
    a.axis_num = grid->num;
    a.row_begin = row0;
    a.wvl_idx_all = wvl_idx;
    a.fld = *fld;
    a.opts = *opts;
    a.out = *out;
    return 0;
}

int prepare_grid(rox_system *sys, const rox_field *fld, const rox_grid *grid, int32_t wvl_idx,
                 const rox_opts *opts, const rox_out *out, hipStream_t st, TraceArgs &a)
{
    int rc = grid_args(sys, fld, grid, wvl_idx, opts, out, a);
    if (rc)
        return rc;
    StreamCtx *cx = ctx_for(sys, st);
    if (!cx)
        return fail(ROX_E_NOMEM, "out of host memory");
    rc = ensure_axes(cx, grid->num);
    if (rc)
        return rc;
    // trace.py:566-570 step = (stop - start)/(num - 1)
    const double sx = (grid->stop[0] - grid->start[0]) / (grid->num - 1);
    const double sy = (grid->stop[1] - grid->start[1]) / (grid->num - 1);
    double *px = cx->d_axes, *py = cx->d_axes + cx->axes_cap;
    const double key[4] = {grid->start[0], grid->start[1], sx, sy};
    if (cx->axes_num != grid->num || memcmp(key, cx->axes_key, sizeof key) != 0) {
        hipLaunchKernelGGL(pupil_axes_kernel, dim3(1), dim3(64), 0, st, grid->start[0],
                           grid->start[1], sx, sy, grid->num, px, py);
        HIP_TRY(hipGetLastError());
        memcpy(cx->axes_key, key, sizeof key);
        cx->axes_num = grid->num;
    }
    a.px = px;
    a.py = py;
    return 0;
}

// ---- rox_trace_through_focus
// Workgroups per CU of a through-focus launch: its 512-thread workgroups hold 4 waves per SIMD
// (two per CU) and grid-stride over the tiles, so that the partial records -- one per
// (wave, plane) -- stay few: 2 x 256 x 8 x 72 B = 288 KiB per plane on 256 CUs.
constexpr int kFocusBlocksPerCu = 2;
constexpr int kFocusFinishBlock = 256;

// the finishing pass: a block merges one plane's partial records -- thread t the records t, t + 256,
// ... in turn, then the lanes pairwise (the lower lane's first), then the four waves in order --
// and forms its statistics
__device__ inline FocusAcc shfl_xor_acc(const FocusAcc &a, int o)
{
    FocusAcc r;
    const double *s = &a.n;
    double *d = &r.n;
    for (int j = 0; j < kFocusStat; ++j)
        d[j] = __shfl_xor(s[j], o);
    return r;
}

// Block (k, i) merges plane k of item i = blockIdx.y, whose n_rec x n_planes records follow item
// i - 1's and whose statistics go to out[i][n_planes]: an item's merges do not depend on the items
// beside it
__global__ void __launch_bounds__(kFocusFinishBlock)
focus_finish_kernel(const FocusAcc *partial, int64_t n_rec, int32_t n_planes, rox_focus_stats *out)
{
    partial += (size_t)blockIdx.y * n_rec * n_planes;
    out += (size_t)blockIdx.y * n_planes;
    const int k = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    FocusAcc v{};
    for (int64_t i = threadIdx.x; i < n_rec; i += kFocusFinishBlock)
        v = focus_merge(v, partial[(size_t)i * n_planes + k]);
    for (int o = 1; o < 64; o <<= 1) {
        const FocusAcc p = shfl_xor_acc(v, o);
        v = (lane & o) ? focus_merge(p, v) : focus_merge(v, p);
    }
    __shared__ FocusAcc s[kFocusFinishBlock / 64];
    if (lane == 0)
        s[wave] = v;
    __syncthreads();
    if (threadIdx.x != 0)
        return;
    for (int w = 1; w < kFocusFinishBlock / 64; ++w)
        v = focus_merge(v, s[w]);
    rox_focus_stats r;
    r.n = (int64_t)v.n;
    if (v.n > 0) {
        r.cx = v.mx;
        r.cy = v.my;
        r.rms_spot = sqrt(v.m2xy / v.n);
        r.rms_spot_image_pt = sqrt(v.sr2 / v.n);
        r.opd_mean = v.mw;
        r.opd_rms = sqrt(v.m2w / v.n);
        r.opd_min = v.wmin;
        r.opd_max = v.wmax;
    } else {
        const double q = __builtin_nan("");
        r.cx = r.cy = r.rms_spot = r.rms_spot_image_pt = q;
        r.opd_mean = r.opd_rms = r.opd_min = r.opd_max = q;
    }
    out[k] = r;
}

// DiffractionGrating constants per (wavelength, interface), doe.py:138-143,
// with libm pow() for `mu**2` and `T**2` as CPython / NumPy scalars evaluate them.
// (Called through a volatile pointer: the compiler folds a direct pow(x, 2.0) into x * x,
// which is not what libm returns for about one argument in a thousand.)
double (*volatile libm_pow)(double, double) = pow;

void phase_consts(const rox_surface *rows, int N, const double *n_table, const double *wvls,
                  int W, std::vector<double> &pc)
{
    pc.assign((size_t)W * N * kPhaseConsts, 0.0);
    for (int w = 0; w < W; ++w)
        for (int i = 1; i < N; ++i) {
            const rox_phase &ph = rows[i].ph;
            if (ph.kind != ROX_PH_GRATING)
                continue;
            const double n_in = n_table[(size_t)w * N + i - 1], n_out = n_table[(size_t)w * N + i];
            const double refl = rows[i].mode == ROX_REFLECT ? -1.0 : 1.0;
            const double mu = n_in / n_out;
            const double T = refl * (wvls[w] * ph.order) / (ph.spacing_nm * n_out);
            double *o = &pc[((size_t)w * N + i) * kPhaseConsts];
            o[0] = mu;
            o[1] = libm_pow(mu, 2.0);
            o[2] = T;
            o[3] = libm_pow(T, 2.0);
        }
}

}  // namespace

// ---------------------------------------------------------------------- C ABI
const rox_surface *rox::system_rows(const rox_system *sys, int32_t *n_ifcs)
{
    *n_ifcs = sys->n_ifcs;
    return sys->rows.data();
}

void rox::system_slot_map(const rox_system *sys, bool filter, std::vector<int32_t> &m, int32_t &n_seg)
{
    slot_map(sys, filter, m, n_seg);
}

extern "C" {

int rox_abi_version(void) { return ROX_ABI_VERSION; }

const char *rox_last_error(void) { return g_err; }

int rox_device_count(int *count)
{
    if (!count)
        return fail(ROX_E_ARG, "null argument");
    *count = 0;
    hipError_t e = hipGetDeviceCount(count);
    if (e != hipSuccess) {
        *count = 0;
        return fail(ROX_E_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    return 0;
}

int rox_set_device(int device)
{
    HIP_TRY(hipSetDevice(device));
    return 0;
}

int rox_pin_host_memory(void *p, size_t bytes, void **device_ptr)
{
    if (!p || !bytes || !device_ptr)
        return fail(ROX_E_ARG, "rox_pin_host_memory: bad argument");
    HIP_TRY(hipHostRegister(p, bytes, hipHostRegisterMapped | hipHostRegisterPortable));
    hipError_t e = hipHostGetDevicePointer(device_ptr, p, 0);
    if (e != hipSuccess) {
        (void)hipHostUnregister(p);
        return fail(ROX_E_HIP, "hipHostGetDevicePointer: %s", hipGetErrorString(e));
    }
    return 0;
}

int rox_unpin_host_memory(void *p)
{
    if (!p)
        return fail(ROX_E_ARG, "rox_unpin_host_memory: null pointer");
    HIP_TRY(hipHostUnregister(p));
    return 0;
}

int rox_copy_async(void *dst, const void *src, size_t bytes, void *stream)
{
    if (bytes == 0)
        return 0;
    if (!dst || !src)
        return fail(ROX_E_ARG, "rox_copy_async: null pointer");
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, (hipStream_t)stream));
    return 0;
}

int rox_synchronize(void *stream)
{
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

int rox_system_create(const rox_surface *rows, int32_t n_ifcs, const double *n_table,
                      const double *wvls, int32_t n_wvls, rox_system **out_sys)
{
    if (!rows || !n_table || !out_sys || n_ifcs < 2 || n_wvls < 1)
        return fail(ROX_E_ARG, "rox_system_create: bad argument");
    int features = 0, n_newton = 0;
    for (int i = 0; i < n_ifcs; ++i) {
        const rox_surface &s = rows[i];
        if (s.profile >= ROX_EVENPOLY && s.profile <= ROX_XTOROID)
            ++n_newton;
        if (s.mode < ROX_TRANSMIT || s.mode > ROX_PHANTOM || s.profile < ROX_SPHERICAL ||
            s.profile > ROX_THINLENS || s.ncoef < 0 || s.ncoef > ROX_MAX_COEF || s.n_ap < 0 ||
            s.n_ap > ROX_MAX_AP || s.ph.kind < ROX_PH_NONE || s.ph.kind > ROX_PH_HOLOGRAM ||
            s.ph.ncoef < 0 || s.ph.ncoef > ROX_MAX_COEF)
            return fail(ROX_E_ARG, "rox_system_create: row %d is malformed", i);
        // rox_surface.flags: ROX_SURF_CV_INT_ZERO says "the curvature is the INTEGER 0" (its
        // only effect: the zero signs of Spherical / Conic df).  It means nothing on any other
        // row, and a caller that left the field uninitialised must not get flat normals on a
        // curved surface: refused, as are bits this version does not define.
        if ((s.flags & ~ROX_SURF_CV_INT_ZERO) != 0)
            return fail(ROX_E_ARG, "rox_system_create: row %d: unknown bits in rox_surface.flags (%#x)", i,
                        (unsigned)s.flags);
        if ((s.flags & ROX_SURF_CV_INT_ZERO) && !(s.profile <= ROX_CONIC && s.cv == 0.0))
            return fail(ROX_E_ARG, "rox_system_create: row %d: ROX_SURF_CV_INT_ZERO on a surface that is not "
                                   "a Spherical / Conic of zero curvature", i);
        if (s.profile == ROX_EVENPOLY)
            features |= F_EVEN;
        else if (s.profile == ROX_RADIALPOLY)
            features |= F_RADIAL;
        else if (s.profile == ROX_YTOROID || s.profile == ROX_XTOROID)
            features |= F_TOROID;
        else if (s.profile == ROX_THINLENS)
            features |= F_PHASE;
        if (s.n_ap > 0)
            features |= F_APLIST;
        if (s.ph.kind != ROX_PH_NONE)
            features |= F_PHASE;
    }
    if ((features & F_PHASE) && !wvls)
        return fail(ROX_E_ARG, "rox_system_create: phase elements need the wavelengths (wvls)");
    rox_system *sys = new (std::nothrow) rox_system;
    if (!sys)
        return fail(ROX_E_NOMEM, "out of host memory");
    sys->n_ifcs = n_ifcs;
    sys->n_wvls = n_wvls;
    sys->features = features;
    sys->n_newton = n_newton;
    sys->rows.assign(rows, rows + n_ifcs);
    hipError_t e = hipGetDevice(&sys->device);
    if (e != hipSuccess) {
        delete sys;
        return fail(ROX_E_NO_DEVICE, "hipGetDevice: %s", hipGetErrorString(e));
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, sys->device) == hipSuccess && prop.multiProcessorCount > 0)
        sys->num_cus = prop.multiProcessorCount;
    int rc = 0;
    do {
        std::vector<dev_surface> drows(n_ifcs);
        for (int i = 0; i < n_ifcs; ++i) {
            drows[i].pub = rows[i];
            // device copy only: rt is exactly the identity (every centred interface) -- the
            // kernels then transform with `v + 0.0` instead of the dgemv chain (rox_device.hpp)
            {
                static const double eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
                bool ident = true;
                for (int k = 0; k < 9; ++k)
                    ident = ident && rows[i].rt[k] == eye[k] && !std::signbit(rows[i].rt[k]);
                // device copy of flags: bit 1 = identity rotation (bit 0 = ROX_SURF_CV_INT_ZERO)
                drows[i].pub.flags = (rows[i].flags & ROX_SURF_CV_INT_ZERO) | (ident ? 2 : 0);
            }
            // device copy only: `-self.cv` as Spherical/Conic.df forms it (rox_device.hpp reads
            // it from the cR slot, which only toroids use): +0.0 for an integer-zero curvature
            if (rows[i].profile <= ROX_CONIC)
                drows[i].pub.cR = (rows[i].flags & ROX_SURF_CV_INT_ZERO) ? 0.0 : -rows[i].cv;
            const double c0 = rows[i].profile == ROX_RADIALPOLY ? 1.0 : 2.0;
            double c_coef = c0;                 // profiles.py:877-882, 1104-1109, 1364-1369
            for (int k = 0; k < ROX_MAX_COEF; ++k) {
                drows[i].cd[2 * k] = rows[i].coefs[k];
                drows[i].cd[2 * k + 1] = c_coef * rows[i].coefs[k];
                c_coef += c0;
            }
        }
        std::vector<double> wv(n_wvls, 0.0), pc;
        if (wvls)
            wv.assign(wvls, wvls + n_wvls);
        phase_consts(rows, n_ifcs, n_table, wv.data(), n_wvls, pc);
        const size_t rb = sizeof(dev_surface) * n_ifcs, nb = sizeof(double) * n_wvls * n_ifcs;
        if (hipMalloc(&sys->d_rows, rb) != hipSuccess || hipMalloc(&sys->d_ntab, nb) != hipSuccess ||
            hipMalloc(&sys->d_phc, nb * kPhaseConsts) != hipSuccess ||
            hipMalloc(&sys->d_wvls, sizeof(double) * n_wvls) != hipSuccess) {
            rc = fail(ROX_E_HIP, "hipMalloc failed for the surface table");
            break;
        }
        if (hipMemcpy(sys->d_rows, drows.data(), rb, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(sys->d_ntab, n_table, nb, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(sys->d_phc, pc.data(), nb * kPhaseConsts, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(sys->d_wvls, wv.data(), sizeof(double) * n_wvls, hipMemcpyHostToDevice) !=
                hipSuccess) {
            rc = fail(ROX_E_HIP, "hipMemcpy failed for the surface table");
            break;
        }
        for (int f = 0; f < 2 && !rc; ++f) {
            std::vector<int32_t> m;
            slot_map(sys, f == 1, m, sys->n_seg[f]);
            if (hipMalloc(&sys->d_slots[f], sizeof(int32_t) * m.size()) != hipSuccess ||
                hipMemcpy(sys->d_slots[f], m.data(), sizeof(int32_t) * m.size(),
                          hipMemcpyHostToDevice) != hipSuccess)
                rc = fail(ROX_E_HIP, "slot map upload failed");
        }
    } while (0);
    if (rc) {
        rox_system_destroy(sys);
        return rc;
    }
    *out_sys = sys;
    return 0;
}

int rox_system_destroy(rox_system *sys)
{
    if (!sys)
        return 0;
    (void)hipFree(sys->d_rows);
    (void)hipFree(sys->d_ntab);
    (void)hipFree(sys->d_phc);
    (void)hipFree(sys->d_wvls);
    (void)hipFree(sys->d_slots[0]);
    (void)hipFree(sys->d_slots[1]);
    for (StreamCtx *c : sys->ctxs) {
        (void)hipFree(c->d_axes);
        (void)hipFree(c->d_tiles);
        (void)hipFree(c->d_ticket);
        (void)hipFree(c->d_hits_base);
        (void)hipFree(c->d_pack_xy);
        (void)hipFree(c->d_pack_status);
        (void)hipFree(c->d_stage);
        (void)hipHostFree(c->h_stage);
        (void)hipFree(c->d_items);
        (void)hipHostFree(c->h_items);
        (void)hipFree(c->d_btickets);
        (void)hipFree(c->d_btiles);
        (void)hipFree(c->d_focus);
        (void)hipHostFree(c->h_focus.h);
        if (c->h_focus.ev)
            (void)hipEventDestroy(c->h_focus.ev);
        for (hipEvent_t ev : c->item_ev)
            if (ev)
                (void)hipEventDestroy(ev);
        delete c;
    }
    (void)hipHostFree(sys->h_search);
    delete sys;
    return 0;
}

int rox_system_num_segments(const rox_system *sys, uint32_t flags, int32_t *n_seg)
{
    if (!sys || !n_seg)
        return fail(ROX_E_ARG, "null argument");
    *n_seg = sys->n_seg[(flags & ROX_FILTER_PHANTOMS) ? 1 : 0];
    return 0;
}

int rox_trace_rays(rox_system *sys, int64_t n_rays, const double *pt0, const double *dir0,
                   const int32_t *wvl_idx, int32_t wvl_idx_all, const rox_opts *opts,
                   const rox_out *out, void *stream)
{
    int rc = check_opts(sys, opts, out, n_rays);
    if (rc)
        return rc;
    if (n_rays < 0 || (n_rays > 0 && (!pt0 || !dir0)))
        return fail(ROX_E_ARG, "rox_trace_rays: bad ray buffers");
    if (!wvl_idx && (wvl_idx_all < 0 || wvl_idx_all >= sys->n_wvls))
        return fail(ROX_E_ARG, "wvl_idx %d out of range", wvl_idx_all);
    hipStream_t st = (hipStream_t)stream;
    TraceArgs a{};
    a.n_rays = n_rays;
    a.wvl_idx_all = wvl_idx_all;
    a.opts = *opts;
    if (!(opts->flags & ROX_HOST_POINTERS)) {
        a.pt0 = pt0; a.dir0 = dir0; a.wvl_idx = wvl_idx; a.out = *out;
        return launch(sys, a, GEN_RAYS, st);
    }
    if (wvl_idx)
        for (int64_t i = 0; i < n_rays; ++i)
            if (wvl_idx[i] < 0 || wvl_idx[i] >= sys->n_wvls)
                return fail(ROX_E_ARG, "wvl_idx[%lld] = %d out of range", (long long)i, wvl_idx[i]);
    Staged s;
    if ((rc = stage_lock(s, sys, st)))
        return rc;
    const size_t vb = sizeof(double) * 3 * (size_t)n_rays;
    const size_t wb = wvl_idx ? sizeof(int32_t) * (size_t)n_rays : 0;
    rc = stage_out(s, sys, st, opts, out, n_rays, 2 * vb + wb);
    if (rc)
        return rc;
    if ((rc = stage_in(s, 0, pt0, vb, st)) || (rc = stage_in(s, vb, dir0, vb, st)) ||
        (rc = stage_in(s, 2 * vb, wvl_idx, wb, st)))
        return rc;
    a.pt0 = (const double *)s.in;
    a.dir0 = (const double *)(s.in + vb);
    a.wvl_idx = wvl_idx ? (const int32_t *)(s.in + 2 * vb) : nullptr;
    a.out = s.dev;
    rc = launch(sys, a, GEN_RAYS, st);
    return rc ? rc : unstage_out(s, st);
}

int rox_trace_pupil_grid(rox_system *sys, const rox_field *fld, const rox_grid *grid,
                         int32_t wvl_idx, const rox_opts *opts, const rox_out *out, void *stream)
{
    if (!sys)
        return fail(ROX_E_ARG, "null system");
    hipStream_t st = (hipStream_t)stream;
    TraceArgs a;
    Staged s;
    int rc;
    if (opts && (opts->flags & ROX_HOST_POINTERS) && (rc = stage_lock(s, sys, st)))
        return rc;
    auto enq = enqueue_lock(sys, st);
    rc = prepare_grid(sys, fld, grid, wvl_idx, opts, out, st, a);
    if (rc)
        return rc;
    if (!(opts->flags & ROX_HOST_POINTERS))
        return launch(sys, a, GEN_PUPIL, st);
    rc = stage_out(s, sys, st, opts, out, a.n_rays, 0);
    if (rc)
        return rc;
    a.out = s.dev;
    rc = launch(sys, a, GEN_PUPIL, st);
    return rc ? rc : unstage_out(s, st);
}

}  // extern "C"

namespace {

// Partial records of one through-focus launch stay under this many bytes: an item of a
// large grid at K = 256 holds 512 workgroups x 8 waves x 256 planes x 72 B = 75 MB of them, so
// the host splits a batch into consecutive launches of whole items (each item's workgroups,
// records and merges are the same either way).
constexpr size_t kFocusBatchPartialBytes = size_t(256) << 20;

// rays of one through-focus item (grid.num >= 1; grid_args checks the row block)
int64_t focus_rays(const rox_grid &g)
{
    return g.kind == ROX_GRID_FAN ? g.num : (int64_t)(g.row_count > 0 ? g.row_count : g.num) * g.num;
}

// What both through-focus entries do once their own argument checks have passed: n_items scans
// (grids of one kind, num and row block, R rays each) in one launch, or in a few launches of
// whole items.  A per-item failure of grid_args is returned as it stands, or behind
// "<item_prefix>: item %d: " where the entry gives a prefix.
int trace_focus_items(rox_system *sys, int32_t n_items, const rox_field *flds, const int32_t *wvl_idx,
                      const rox_grid *grids, const rox_opts *opts, int32_t n_planes,
                      const rox_focus_plane *planes, double *rows, int64_t ld, uint8_t *status,
                      rox_focus_stats *stats, hipStream_t st, const char *item_prefix)
{
    // the items, validated one by one as a FAN launch's arguments are (plane 0 in rox_opts; the
    // kernel reads planes[]); a stats-only item names a dummy seg, which the kernel never writes
    const rox_grid &g0 = grids[0];
    const int64_t R = focus_rays(g0);
    std::vector<FocusArgs> items((size_t)n_items);
    double dummy = 0.0;
    for (int32_t i = 0; i < n_items; ++i) {
        const rox_focus_plane &p0 = planes[(size_t)i * n_planes];
        rox_opts o = opts[i];
        o.foc = p0.foc;
        o.image_pt[0] = p0.image_pt[0];
        o.image_pt[1] = p0.image_pt[1];
        o.wf = p0.wf;
        rox_out out{};
        out.seg = rows ? rows + (size_t)i * n_planes * 3 * ld : &dummy;
        out.ld = rows ? ld : R;
        out.status = status ? status + (size_t)i * ld : nullptr;
        const int rc = grid_args(sys, &flds[i], &grids[i], wvl_idx[i], &o, &out, items[i]);
        if (rc) {
            if (!item_prefix)
                return rc;
            char msg[sizeof g_err];
            memcpy(msg, g_err, sizeof msg);
            return fail(rc, "%s: item %d: %s", item_prefix, i, msg);
        }
    }

    auto enq = enqueue_lock(sys, st);
    StreamCtx *cx = ctx_for(sys, st);
    if (!cx)
        return fail(ROX_E_NOMEM, "out of host memory");
    LaunchCfg k;
    int inst = 0;
    for (int32_t i = 0; i < n_items; ++i) {     // (the same instance for every item: same flags)
        const int rc = launch_setup(sys, items[i], GEN_PUPIL, false, st, k, inst);
        if (rc)
            return rc;
    }
    const int bs = block_of(MODE_FOCUS, kInstances[inst]);
    const int64_t blocks = std::min<int64_t>((R + bs - 1) / bs, (int64_t)sys->num_cus * kFocusBlocksPerCu);
    const int64_t n_rec = blocks * (bs / 64);                   // partial records per (item, plane)
    const size_t item_part = stats ? (size_t)n_rec * n_planes * sizeof(FocusAcc) : 0;
    const int32_t per_launch = item_part ? (int32_t)std::max<size_t>(
                                               1, std::min<size_t>(n_items, kFocusBatchPartialBytes / item_part))
                                         : n_items;

    // pupil axes: one slot per distinct (start, step) -- trace.py:566-570 step = (stop - start)/(num - 1)
    std::vector<double> prm;
    std::vector<int32_t> slot_of((size_t)n_items);
    for (int32_t i = 0; i < n_items; ++i) {
        const rox_grid &g = grids[i];
        const double key[4] = {g.start[0], g.start[1], (g.stop[0] - g.start[0]) / (g.num - 1),
                               (g.stop[1] - g.start[1]) / (g.num - 1)};
        size_t s = 0;
        while (s < prm.size() / 4 && memcmp(&prm[4 * s], key, sizeof key) != 0)
            ++s;
        if (s == prm.size() / 4)
            prm.insert(prm.end(), key, key + 4);
        slot_of[i] = (int32_t)s;
    }
    const int32_t n_slots = (int32_t)(prm.size() / 4);

    // device block: [axes] [items][planes][axis parameters] (staged) [statistics][partial records]
    // -- the axes in front, where the same axis parameters and num put them again
    const size_t b_axes = up256(sizeof(double) * 2 * (size_t)n_slots * g0.num);
    const size_t b_items = up256(sizeof(FocusArgs) * (size_t)n_items);
    const size_t b_planes = up256(sizeof(rox_focus_plane) * (size_t)n_items * n_planes);
    const size_t b_prm = up256(sizeof(double) * prm.size());
    const size_t b_stats = stats ? up256(sizeof(rox_focus_stats) * (size_t)n_items * n_planes) : 0;
    const size_t staged = b_items + b_planes + b_prm;
    const size_t need = b_axes + staged + b_stats + item_part * (size_t)per_launch;
    if (need > cx->focus_cap) {
        cx->focus_prm.clear();                  // the new block holds no axes
        HIP_TRY(regrow(cx->d_focus, cx->focus_cap, need, need));
    }
    double *d_axes = (double *)cx->d_focus;
    char *d_staged = cx->d_focus + b_axes;
    FocusArgs *d_items = (FocusArgs *)d_staged;
    rox_focus_plane *d_planes = (rox_focus_plane *)(d_staged + b_items);
    double *d_prm = (double *)(d_staged + b_items + b_planes);
    rox_focus_stats *d_stats = (rox_focus_stats *)(d_staged + staged);
    char *d_part = d_staged + staged + b_stats;

    for (int32_t i = 0; i < n_items; ++i) {
        FocusArgs &f = items[i];
        f.px = d_axes + (size_t)slot_of[i] * 2 * g0.num;
        f.py = f.px + g0.num;
        f.out.seg = nullptr;
        f.ray_base = 0;
        f.in_ld = R;
        f.planes = d_planes + (size_t)i * n_planes;
        f.n_planes = n_planes;
        f.focus_rows = rows ? rows + (size_t)i * n_planes * 3 * ld : nullptr;
        f.partial = stats ? (double *)(d_part + (size_t)(i % per_launch) * item_part) : nullptr;
    }

    // stage through the pinned block (once the previous call's copy has read it), one copy
    HIP_TRY(cx->h_focus.acquire(staged));
    char *h = cx->h_focus.h;
    memcpy(h, items.data(), sizeof(FocusArgs) * (size_t)n_items);
    memcpy(h + b_items, planes, sizeof(rox_focus_plane) * (size_t)n_items * n_planes);
    memcpy(h + b_items + b_planes, prm.data(), sizeof(double) * prm.size());
    HIP_TRY(hipMemcpyAsync(d_staged, h, staged, hipMemcpyHostToDevice, st));
    HIP_TRY(cx->h_focus.record(st));
    // the axes, unless the block holds them from the previous call on this context
    if (cx->focus_num != g0.num || cx->focus_prm.size() != prm.size() ||
        memcmp(cx->focus_prm.data(), prm.data(), sizeof(double) * prm.size()) != 0) {
        cx->focus_prm.clear();
        hipLaunchKernelGGL(pupil_axes_slots_kernel, dim3((unsigned)((2 * n_slots + 63) / 64)), dim3(64), 0,
                           st, (const double *)d_prm, n_slots, g0.num, d_axes);
        HIP_TRY(hipGetLastError());
        cx->focus_prm = prm;
        cx->focus_num = g0.num;
    }

    const bool dev_dst = stats && is_device(stats);
    for (int32_t i0 = 0; i0 < n_items; i0 += per_launch) {
        const int32_t n = std::min(per_launch, n_items - i0);
        if (stats)      // every wave merges into its records: they start at n = 0
            HIP_TRY(hipMemsetAsync(d_part, 0, item_part * (size_t)n, st));
        k.grid = dim3((unsigned)blocks, (unsigned)n);
        trace_fns(inst, k).focus(k, d_items + i0);
        HIP_TRY(hipGetLastError());
        if (!stats)
            continue;
        hipLaunchKernelGGL(focus_finish_kernel, dim3((unsigned)n_planes, (unsigned)n),
                           dim3(kFocusFinishBlock), 0, st, (const FocusAcc *)d_part, n_rec, n_planes,
                           (dev_dst ? stats : d_stats) + (size_t)i0 * n_planes);
        HIP_TRY(hipGetLastError());
    }
    if (!stats || dev_dst)
        return 0;
    HIP_TRY(hipMemcpyAsync(stats, d_stats, sizeof(rox_focus_stats) * (size_t)n_items * n_planes,
                           hipMemcpyDeviceToHost, st));
    enq.unlock();
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

}  // namespace

extern "C" {

// One trace of a pupil grid, evaluated at n_planes focus positions (include/roxtrace.h).
int rox_trace_through_focus(rox_system *sys, const rox_field *fld, const rox_grid *grid,
                            int32_t wvl_idx, const rox_opts *opts, int32_t n_planes,
                            const rox_focus_plane *planes, double *rows, int64_t ld, uint8_t *status,
                            rox_focus_stats *stats, void *stream)
{
    // every argument check comes before anything touches a device
    if (!fld || !grid || !opts)
        return fail(ROX_E_ARG, "rox_trace_through_focus: null argument");
    ROX_TRY(check_range("rox_trace_through_focus", "n_planes", n_planes, 1, ROX_MAX_FOCUS_PLANES));
    if (!planes)
        return fail(ROX_E_ARG, "rox_trace_through_focus: planes is null");
    if (!rows && !stats)
        return fail(ROX_E_ARG, "rox_trace_through_focus: rows and stats are both null");
    if (opts->out_mode != ROX_OUT_FAN)
        return fail(ROX_E_ARG, "rox_trace_through_focus: out_mode must be ROX_OUT_FAN (got %d)", opts->out_mode);
    if (opts->flags & (ROX_HOST_POINTERS | ROX_HITS_APPEND))
        return fail(ROX_E_ARG, "rox_trace_through_focus: device pointers only, no ROX_HOST_POINTERS / "
                               "ROX_HITS_APPEND");
    if (grid->num < 1)
        return fail(ROX_E_ARG, "rox_trace_through_focus: grid.num must be >= 1");
    const int64_t R = focus_rays(*grid);
    if (rows && ld < R)
        return fail(ROX_E_ARG, "rox_trace_through_focus: ld (%lld) < rays (%lld)", (long long)ld, (long long)R);
    if (R > (int64_t(1) << 28))
        return fail(ROX_E_UNSUPPORTED, "rox_trace_through_focus: %lld rays (max 2^28 per call)", (long long)R);
    for (int32_t p = 0; p < n_planes; ++p) {
        const rox_wavefront &w = planes[p].wf;
        if (!(w.ref_radius != 0.0) || w.kind < ROX_WF_FINITE || w.kind > ROX_WF_INF_SPLIT)
            return fail(ROX_E_ARG, "rox_trace_through_focus: plane %d: bad wf (ref_radius %g, kind %d)", p,
                        w.ref_radius, w.kind);
    }
    if (!sys)
        return fail(ROX_E_ARG, "rox_trace_through_focus: null system");
    if (wvl_idx < 0 || wvl_idx >= sys->n_wvls)
        return fail(ROX_E_ARG, "rox_trace_through_focus: wvl_idx %d out of range", wvl_idx);

    return trace_focus_items(sys, 1, fld, &wvl_idx, grid, opts, n_planes, planes, rows, ld, status, stats,
                             (hipStream_t)stream, nullptr);
}

// n_items through-focus scans in one launch (include/roxtrace.h): item i is rox_trace_through_focus
// with flds[i], grids[i], wvl_idx[i], opts[i] and planes[i][n_planes] -- which is this with one item.
int rox_trace_through_focus_grids(rox_system *sys, int32_t n_items, const rox_field *flds,
                                  const int32_t *wvl_idx, const rox_grid *grids, const rox_opts *opts,
                                  int32_t n_planes, const rox_focus_plane *planes, double *rows,
                                  int64_t ld, uint8_t *status, rox_focus_stats *stats, void *stream)
{
    static const char kE[] = "rox_trace_through_focus_grids";
    // every argument check comes before anything touches a device
    ROX_TRY(check_range(kE, "n_items", n_items, 1, ROX_MAX_FOCUS_ITEMS));
    ROX_TRY(check_range(kE, "n_planes", n_planes, 1, ROX_MAX_FOCUS_PLANES));
    if (!flds || !wvl_idx || !grids || !opts || !planes)
        return fail(ROX_E_ARG, "%s: null array (flds, wvl_idx, grids, opts or planes)", kE);
    if (!rows && !stats)
        return fail(ROX_E_ARG, "%s: rows and stats are both null", kE);
    const rox_grid &g0 = grids[0];
    if (g0.num < 1)
        return fail(ROX_E_ARG, "%s: item 0: grid.num must be >= 1", kE);
    const bool fan = g0.kind == ROX_GRID_FAN;
    const int64_t R = focus_rays(g0);
    if ((rows || status) && ld < R)
        return fail(ROX_E_ARG, "%s: ld (%lld) < rays (%lld)", kE, (long long)ld, (long long)R);
    if (R > (int64_t(1) << 28))
        return fail(ROX_E_UNSUPPORTED, "%s: %lld rays (max 2^28 per item)", kE, (long long)R);
    const rox_opts &o0 = opts[0];
    for (int32_t i = 0; i < n_items; ++i) {
        const rox_grid &g = grids[i];
        if (g.kind != g0.kind || g.num != g0.num ||
            (!fan && (g.row_begin != g0.row_begin || g.row_count != g0.row_count)))
            return fail(ROX_E_ARG, "%s: item %d: grid kind, num and row block must match item 0's", kE, i);
        const rox_opts &o = opts[i];
        if (o.out_mode != ROX_OUT_FAN)
            return fail(ROX_E_ARG, "%s: item %d: out_mode must be ROX_OUT_FAN (got %d)", kE, i, o.out_mode);
        if (o.flags & (ROX_HOST_POINTERS | ROX_HITS_APPEND))
            return fail(ROX_E_ARG, "%s: item %d: device pointers only, no ROX_HOST_POINTERS / "
                                   "ROX_HITS_APPEND", kE, i);
        if (((o.flags ^ o0.flags) & (ROX_FILTER_PHANTOMS | ROX_FAST_FP64)) ||
            o.first_surf != o0.first_surf || o.last_surf != o0.last_surf)
            return fail(ROX_E_ARG, "%s: item %d: ROX_FILTER_PHANTOMS, ROX_FAST_FP64, first_surf and "
                                   "last_surf must match item 0's", kE, i);
        for (int32_t p = 0; p < n_planes; ++p) {
            const rox_wavefront &w = planes[(size_t)i * n_planes + p].wf;
            if (!(w.ref_radius != 0.0) || w.kind < ROX_WF_FINITE || w.kind > ROX_WF_INF_SPLIT)
                return fail(ROX_E_ARG, "%s: item %d plane %d: bad wf (ref_radius %g, kind %d)", kE, i, p,
                            w.ref_radius, w.kind);
        }
    }
    if (!sys)
        return fail(ROX_E_ARG, "%s: null system", kE);
    for (int32_t i = 0; i < n_items; ++i)
        if (wvl_idx[i] < 0 || wvl_idx[i] >= sys->n_wvls)
            return fail(ROX_E_ARG, "%s: item %d: wvl_idx %d out of range", kE, i, wvl_idx[i]);

    return trace_focus_items(sys, n_items, flds, wvl_idx, grids, opts, n_planes, planes, rows, ld, status,
                             stats, (hipStream_t)stream, kE);
}

// Several pupil grids of one system in ONE launch: item i traces `grid` for field flds[i]
// at wavelength wvl_idx[i] with opts[i] into outs[i].  blockIdx.y = item, so a spot diagram's
// 3 fields x 3 wavelengths x 64^2 rays fills the chip as one launch instead of idling on
// nine small ones, and nine 512^2 grids lose eight launch tails.
int rox_trace_pupil_grids(rox_system *sys, int32_t n_grids, const rox_field *flds,
                          const int32_t *wvl_idx, const rox_grid *grid, const rox_opts *opts,
                          const rox_out *outs, void *stream)
{
    if (!sys)
        return fail(ROX_E_ARG, "null system");
    if (n_grids < 0 || (n_grids > 0 && (!flds || !wvl_idx || !opts || !outs)))
        return fail(ROX_E_ARG, "null argument");
    if (n_grids == 0)
        return 0;
    hipStream_t st = (hipStream_t)stream;
    for (int32_t i = 0; i < n_grids; ++i) {
        if (opts[i].flags & (ROX_HOST_POINTERS | ROX_HITS_APPEND))
            return fail(ROX_E_UNSUPPORTED, "rox_trace_pupil_grids: device pointers only, no ROX_HITS_APPEND "
                                           "(item %d)", i);
        if (opts[i].out_mode != opts[0].out_mode ||
            ((opts[i].flags ^ opts[0].flags) & (ROX_FILTER_PHANTOMS | ROX_FAST_FP64)))
            return fail(ROX_E_ARG, "rox_trace_pupil_grids: out_mode, ROX_FILTER_PHANTOMS and ROX_FAST_FP64 "
                                   "must be the same for every item (item %d)", i);
    }
    // the items, validated one by one exactly as single launches are
    auto enq = enqueue_lock(sys, st);
    std::vector<TraceArgs> items((size_t)n_grids);
    int rc;
    for (int32_t i = 0; i < n_grids; ++i)
        if ((rc = prepare_grid(sys, &flds[i], grid, wvl_idx[i], &opts[i], &outs[i], st, items[i])))
            return rc;
    const int64_t R = items[0].n_rays;
    const bool compact = opts[0].out_mode == ROX_OUT_HITS_COMPACT;
    if (n_grids == 1 || n_grids > 65535 || R > rays_per_launch() || R == 0) {
        // nothing to batch (or more than one launch each): the plain path, item by item
        for (int32_t i = 0; i < n_grids; ++i)
            if ((rc = launch(sys, items[i], GEN_PUPIL, st)))
                return rc;
        return 0;
    }
    LaunchCfg k;
    int inst = 0;
    for (int32_t i = 0; i < n_grids; ++i) {
        if ((rc = launch_setup(sys, items[i], GEN_PUPIL, false, st, k, inst)))
            return rc;
        items[i].in_ld = R;
        items[i].ray_base = 0;
    }
    StreamCtx *cx = ctx_for(sys, st);
    if (!cx)
        return fail(ROX_E_NOMEM, "out of host memory");
    std::lock_guard<std::mutex> lock(cx->batch_mu);
    k.small = want_small(sys, (int64_t)n_grids * R, opts[0].out_mode, kInstances[inst], n_grids);
    const int bs = block_of(opts[0].out_mode, kInstances[inst], k.small);
    int64_t blocks = (R + bs - 1) / bs;
    if (compact) {
        // per-item tickets
        if ((int64_t)n_grids > cx->btickets_cap)
            HIP_TRY(regrow_zeroed(cx->d_btickets, cx->btickets_cap, n_grids,
                                  sizeof(uint32_t) * 2 * (size_t)n_grids, st));
        // per-item look-back states; small tiles when the whole batch is small
        const int32_t small = ((int64_t)n_grids * R <= (int64_t)sys->num_cus * kSmallTile)
                                  ? compact_small_want(sys, R) : 0;
        const int64_t tiles = compact_tiles(R, small, bs);
        blocks = tiles;
        if ((int64_t)n_grids * tiles > cx->btiles_cap) {
            HIP_TRY(regrow_zeroed(cx->d_btiles, cx->btiles_cap, n_grids * tiles,
                                  sizeof(uint64_t) * (size_t)(n_grids * tiles), st));
            cx->bepoch = 0;
        }
        ++cx->bepoch;
        for (int32_t i = 0; i < n_grids; ++i) {
            items[i].small_tiles = small;
            items[i].tile_state = cx->d_btiles + (size_t)i * tiles;
            items[i].ticket = cx->d_btickets + 2 * (size_t)i;
            items[i].hits_base_in = nullptr;
            items[i].hits_total_out = outs[i].n_hits;
            items[i].epoch = cx->bepoch;
        }
    }
    // Per item as many workgroups as a launch of its own would get: items differ in work
    // (vignetting, Newton counts), and it is the hardware dispatcher handing out many more
    // workgroups than fit that evens them out.  (Splitting one launch's worth between the
    // items -- all resident at once, each striding over its item -- measured 6 % slower on
    // config 5's 45 grids of 2048 x 2048.)  HITS_COMPACT draws tiles by ticket: any number
    // of workgroups per item will do.
    const int64_t cap = (int64_t)sys->num_cus * (compact ? compact_blocks_per_cu() : blocks_per_cu(bs));
    if (blocks > cap)
        blocks = cap;
    k.grid = dim3((unsigned)blocks, (unsigned)n_grids);
    // a few items: in the kernel argument itself (rox_device.hpp BatchArgs) -- nothing to upload
    static const bool no_inline = [] {
        const char *e = getenv("ROX_BATCH_NO_INLINE");      // (the A/B switch of tools/ab_bench.py)
        return e && *e && atoi(e) != 0;
    }();
    if (n_grids <= kInlineItems && !no_inline) {
        k.n_inline = n_grids;
        trace_fns(inst, k).batch(k, items.data());
        HIP_TRY(hipGetLastError());
        return 0;
    }
    // items -> pinned slot -> device, in stream order
    if (n_grids > cx->items_cap) {
        const int32_t want = n_grids < 64 ? 64 : n_grids;
        HIP_TRY(release(cx->d_items, cx->items_cap));   // synchronises: the copies from h_items are done
        HIP_TRY(regrow(cx->h_items, cx->items_cap, want,
                       sizeof(TraceArgs) * (size_t)want * StreamCtx::kItemSlots, hipHostMallocDefault));
        HIP_TRY(regrow(cx->d_items, cx->items_cap, want, sizeof(TraceArgs) * (size_t)want));
        cx->items_last.clear();
        for (bool &live : cx->item_ev_live)
            live = false;
    }
    // The items of a batch that repeats the previous one of this stream byte for byte (a figure
    // refreshed with unchanged arguments, a timing loop) are already in d_items: the upload -- a
    // copy-engine transfer in front of the kernel, ~6 us -- is skipped.
    const size_t items_bytes = sizeof(TraceArgs) * (size_t)n_grids;
    // ROX_BATCH_ALWAYS_UPLOAD=1 (read once) switches the short cut off: bench.py times the
    // BASELINE configurations that way, so that its figures are those of a call whose fields or
    // outputs changed.  (TraceArgs is value-initialised, padding included, before it is filled.)
    static const bool always_upload = [] {
        const char *e = getenv("ROX_BATCH_ALWAYS_UPLOAD");
        return e && *e && atoi(e) != 0;
    }();
    const bool same_items = !always_upload && cx->items_last.size() == items_bytes &&
                            memcmp(cx->items_last.data(), items.data(), items_bytes) == 0;
    if (!same_items) {
        const uint32_t slot = cx->item_slot++ % StreamCtx::kItemSlots;
        if (!cx->item_ev[slot])
            HIP_TRY(hipEventCreateWithFlags(&cx->item_ev[slot], hipEventDisableTiming));
        if (cx->item_ev_live[slot])
            HIP_TRY(hipEventSynchronize(cx->item_ev[slot]));
        TraceArgs *h = cx->h_items + (size_t)slot * cx->items_cap;
        memcpy(h, items.data(), items_bytes);
        cx->items_last.clear();                     // (not valid until the copy is enqueued)
        HIP_TRY(hipMemcpyAsync(cx->d_items, h, items_bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipEventRecord(cx->item_ev[slot], st));
        cx->item_ev_live[slot] = true;
        cx->items_last.assign(reinterpret_cast<const char *>(items.data()),
                              reinterpret_cast<const char *>(items.data()) + items_bytes);
    }
    trace_fns(inst, k).batch(k, cx->d_items);
    HIP_TRY(hipGetLastError());
    return 0;
}

int rox_trace_pupil_list(rox_system *sys, const rox_field *fld, int64_t n_rays, const double *px,
                         const double *py, int32_t wvl_idx, const rox_opts *opts,
                         const rox_out *out, void *stream)
{
    int rc = check_opts(sys, opts, out, n_rays);
    if (rc)
        return rc;
    rc = check_field(fld);
    if (rc)
        return rc;
    if (n_rays < 0 || (n_rays > 0 && (!px || !py)))
        return fail(ROX_E_ARG, "rox_trace_pupil_list: bad argument");
    if (wvl_idx < 0 || wvl_idx >= sys->n_wvls)
        return fail(ROX_E_ARG, "wvl_idx %d out of range", wvl_idx);
    hipStream_t st = (hipStream_t)stream;
    TraceArgs a{};
    a.n_rays = n_rays;
    a.axis_kind = AXIS_LIST;
    a.axis_num = 1;
    a.wvl_idx_all = wvl_idx;
    a.fld = *fld;
    a.opts = *opts;
    if (!(opts->flags & ROX_HOST_POINTERS)) {
        a.px = px; a.py = py; a.out = *out;
        return launch(sys, a, GEN_PUPIL, st);
    }
    Staged s;
    if ((rc = stage_lock(s, sys, st)))
        return rc;
    const size_t pb = sizeof(double) * (size_t)n_rays;
    rc = stage_out(s, sys, st, opts, out, n_rays, 2 * pb);
    if (rc)
        return rc;
    if ((rc = stage_in(s, 0, px, pb, st)) || (rc = stage_in(s, pb, py, pb, st)))
        return rc;
    a.px = (const double *)s.in;
    a.py = (const double *)(s.in + pb);
    a.out = s.dev;
    rc = launch(sys, a, GEN_PUPIL, st);
    return rc ? rc : unstage_out(s, st);
}

// the iterated single-ray searches (aiming, vignetting, pupil iterations): up to this many
// problems per call get a wave each (latency: a model's fields, run side by side); larger
// batches keep a lane per problem (throughput: soaks, sweeps)
constexpr int32_t kWavePerProblemMax = 1024;

int rox_iterate_ray_raw(rox_system *sys, int32_t n, const rox_aim *probs, double eps,
                        double *aim_xy, int32_t *result, double *last_xy, int32_t *last_status,
                        void *stream)
{
    if (!sys || n < 0 || (n > 0 && (!probs || !aim_xy || !result)) || (!last_xy != !last_status))
        return fail(ROX_E_ARG, "rox_iterate_ray_raw: bad argument");
    if (n == 0)
        return 0;
    for (int i = 0; i < n; ++i) {
        if (probs[i].wvl_idx < 0 || probs[i].wvl_idx >= sys->n_wvls)
            return fail(ROX_E_ARG, "probs[%d].wvl_idx %d out of range", i, probs[i].wvl_idx);
        if (probs[i].surf < 0 || probs[i].surf >= sys->n_ifcs)
            return fail(ROX_E_ARG, "probs[%d].surf %d out of range", i, probs[i].surf);
        if (probs[i].two_d && !(probs[i].epsfcn >= 0.0))
            return fail(ROX_E_ARG, "probs[%d].epsfcn %g", i, probs[i].epsfcn);
    }
    hipStream_t st = (hipStream_t)stream;
    size_t lds;
    bool gtab;
    if (int rcl = search_lds(sys, lds, gtab))
        return rcl;
    const size_t pb = up16(sizeof(rox_aim) * n), yb = up16(sizeof(double) * 2 * n), rb = up16(sizeof(int32_t) * n);
    std::lock_guard<std::mutex> lock(sys->search_mu);
    char *d = nullptr;
    int rc = search_block(sys, pb + 2 * yb + 2 * rb, d);
    if (rc)
        return rc;
    memcpy(d, probs, sizeof(rox_aim) * n);
    AimArgs a{};
    a.rows = sys->d_rows; a.n_table = sys->d_ntab; a.ph_consts = sys->d_phc; a.wvls = sys->d_wvls;
    a.slots = sys->d_slots[0];
    a.n_ifcs = sys->n_ifcs; a.n_wvls = sys->n_wvls; a.n = n;
    a.probs = (const rox_aim *)d;
    a.aim_xy = (double *)(d + pb);
    a.result = (int32_t *)(d + pb + 2 * yb);
    a.last_xy = last_xy ? (double *)(d + pb + yb) : nullptr;
    a.last_status = last_xy ? (int32_t *)(d + pb + 2 * yb + rb) : nullptr;
    a.eps = eps;
    a.wave_per_problem = n <= kWavePerProblemMax;
    search_fns(sys, gtab).aim(a, lds, st);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = hipStreamSynchronize(st);
    if (e == hipSuccess) {
        memcpy(aim_xy, a.aim_xy, sizeof(double) * 2 * n);
        memcpy(result, a.result, sizeof(int32_t) * n);
        if (last_xy) {
            memcpy(last_xy, a.last_xy, sizeof(double) * 2 * n);
            memcpy(last_status, a.last_status, sizeof(int32_t) * n);
        }
    }
    if (e != hipSuccess)
        return fail(ROX_E_HIP, "rox_iterate_ray_raw: %s", hipGetErrorString(e));
    return 0;
}

int rox_aim_chief_rays(rox_system *sys, int32_t n, const rox_aim *probs, double eps,
                       double *aim_xy, int32_t *result, void *stream)
{
    return rox_iterate_ray_raw(sys, n, probs, eps, aim_xy, result, nullptr, nullptr, stream);
}

int rox_find_real_enp(rox_system *sys, int32_t n, const rox_enp *probs, double eps,
                      double *z_out, int32_t *result, void *stream)
{
    if (!sys || n < 0 || (n > 0 && (!probs || !z_out || !result)))
        return fail(ROX_E_ARG, "rox_find_real_enp: bad argument");
    if (n == 0)
        return 0;
    for (int i = 0; i < n; ++i) {
        if (probs[i].wvl_idx < 0 || probs[i].wvl_idx >= sys->n_wvls)
            return fail(ROX_E_ARG, "probs[%d].wvl_idx %d out of range", i, probs[i].wvl_idx);
        if (probs[i].surf < 0 || probs[i].surf >= sys->n_ifcs)
            return fail(ROX_E_ARG, "probs[%d].surf %d out of range", i, probs[i].surf);
    }
    hipStream_t st = (hipStream_t)stream;
    size_t lds;
    bool gtab;
    if (int rcl = search_lds(sys, lds, gtab))
        return rcl;
    const size_t pb = up16(sizeof(rox_enp) * n), zb = up16(sizeof(double) * 2 * n);
    std::lock_guard<std::mutex> lock(sys->search_mu);
    char *d = nullptr;
    int rc = search_block(sys, pb + zb + sizeof(int32_t) * n, d);
    if (rc)
        return rc;
    memcpy(d, probs, sizeof(rox_enp) * n);
    EnpArgs a{};
    a.rows = sys->d_rows; a.n_table = sys->d_ntab; a.ph_consts = sys->d_phc; a.wvls = sys->d_wvls;
    a.slots = sys->d_slots[0];
    a.n_ifcs = sys->n_ifcs; a.n_wvls = sys->n_wvls; a.n = n;
    a.probs = (const rox_enp *)d;
    a.z_out = (double *)(d + pb);
    a.result = (int32_t *)(d + pb + zb);
    a.eps = eps;
    search_fns(sys, gtab).enp(a, lds, st);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = hipStreamSynchronize(st);
    if (e == hipSuccess) {
        memcpy(z_out, a.z_out, sizeof(double) * 2 * n);
        memcpy(result, a.result, sizeof(int32_t) * n);
    }
    if (e != hipSuccess)
        return fail(ROX_E_HIP, "rox_find_real_enp: %s", hipGetErrorString(e));
    return 0;
}

int rox_iterate_pupil_rays(rox_system *sys, int32_t n, const rox_pupil_iter *probs, double eps,
                           double *start_r, void *stream)
{
    if (!sys || n < 0 || (n > 0 && (!probs || !start_r)))
        return fail(ROX_E_ARG, "rox_iterate_pupil_rays: bad argument");
    if (n == 0)
        return 0;
    for (int i = 0; i < n; ++i) {
        const rox_pupil_iter &p = probs[i];
        if (p.wvl_idx < 0 || p.wvl_idx >= sys->n_wvls)
            return fail(ROX_E_ARG, "probs[%d].wvl_idx %d out of range", i, p.wvl_idx);
        if (p.indx < 0 || p.indx >= sys->n_ifcs || (p.xy != 0 && p.xy != 1))
            return fail(ROX_E_ARG, "probs[%d] is malformed", i);
        int rc = check_field(&p.fld);
        if (rc)
            return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    size_t lds;
    bool gtab;
    if (int rcl = search_lds(sys, lds, gtab))
        return rcl;
    const size_t pb = up16(sizeof(rox_pupil_iter) * n);
    std::lock_guard<std::mutex> lock(sys->search_mu);
    char *d = nullptr;
    int rc = search_block(sys, pb + sizeof(double) * n, d);
    if (rc)
        return rc;
    memcpy(d, probs, sizeof(rox_pupil_iter) * n);
    VigArgs a{};
    a.rows = sys->d_rows; a.n_table = sys->d_ntab; a.ph_consts = sys->d_phc; a.wvls = sys->d_wvls;
    a.slots = sys->d_slots[0];
    a.n_ifcs = sys->n_ifcs; a.n_wvls = sys->n_wvls; a.n = n;
    a.iters = (const rox_pupil_iter *)d;
    a.vig = (double *)(d + pb);
    a.eps = eps;
    a.wave_per_problem = n <= kWavePerProblemMax;
    search_fns(sys, gtab).vig(a, lds, st);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = hipStreamSynchronize(st);
    if (e == hipSuccess)
        memcpy(start_r, a.vig, sizeof(double) * n);
    if (e != hipSuccess)
        return fail(ROX_E_HIP, "rox_iterate_pupil_rays: %s", hipGetErrorString(e));
    return 0;
}

int rox_calc_vignetting(rox_system *sys, int32_t n, const rox_vig *probs, double eps,
                        double *vig, int32_t *clip_surf, void *stream)
{
    if (!sys || n < 0 || (n > 0 && (!probs || !vig || !clip_surf)))
        return fail(ROX_E_ARG, "rox_calc_vignetting: bad argument");
    if (n == 0)
        return 0;
    for (int i = 0; i < n; ++i) {
        const rox_vig &p = probs[i];
        if (p.wvl_idx < 0 || p.wvl_idx >= sys->n_wvls)
            return fail(ROX_E_ARG, "probs[%d].wvl_idx %d out of range", i, p.wvl_idx);
        if (p.stop_surf >= sys->n_ifcs || (p.xy != 0 && p.xy != 1) || p.max_iter < 0)
            return fail(ROX_E_ARG, "probs[%d] is malformed", i);
        int rc = check_field(&p.fld);
        if (rc)
            return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    size_t lds;
    bool gtab;
    if (int rcl = search_lds(sys, lds, gtab))
        return rcl;
    const size_t pb = up16(sizeof(rox_vig) * n), vb = up16(sizeof(double) * n);
    std::lock_guard<std::mutex> lock(sys->search_mu);
    char *d = nullptr;
    int rc = search_block(sys, pb + vb + sizeof(int32_t) * n, d);
    if (rc)
        return rc;
    memcpy(d, probs, sizeof(rox_vig) * n);
    VigArgs a{};
    a.rows = sys->d_rows; a.n_table = sys->d_ntab; a.ph_consts = sys->d_phc; a.wvls = sys->d_wvls;
    a.slots = sys->d_slots[0];
    a.n_ifcs = sys->n_ifcs; a.n_wvls = sys->n_wvls; a.n = n;
    a.probs = (const rox_vig *)d;
    a.vig = (double *)(d + pb);
    a.clip = (int32_t *)(d + pb + vb);
    a.eps = eps;
    a.wave_per_problem = n <= kWavePerProblemMax;
    search_fns(sys, gtab).vig(a, lds, st);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = hipStreamSynchronize(st);
    if (e == hipSuccess) {
        memcpy(vig, a.vig, sizeof(double) * n);
        memcpy(clip_surf, a.clip, sizeof(int32_t) * n);
    }
    if (e != hipSuccess)
        return fail(ROX_E_HIP, "rox_calc_vignetting: %s", hipGetErrorString(e));
    return 0;
}

// ---- include/roxtrace_diag.h ------------------------------------------------
int rox_diag_pack_launches(uint64_t counts[2])
{
    if (!counts)
        return fail(ROX_E_ARG, "null argument");
    counts[0] = g_fused_pack_launches.load();
    counts[1] = g_two_pass_launches.load();
    return 0;
}

int rox_selftest_fp64(uint64_t n, uint64_t seed, uint64_t counts[4])
{
    if (!counts)
        return fail(ROX_E_ARG, "null argument");
    unsigned long long *d = nullptr;
    HIP_TRY(hipMalloc(&d, 4 * sizeof(unsigned long long)));
    HIP_TRY(hipMemset(d, 0, 4 * sizeof(unsigned long long)));
    hipLaunchKernelGGL(selftest_kernel, dim3(2048), dim3(kBlock), 0, nullptr, n, seed, d);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = hipMemcpy(counts, d, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess)
        return fail(ROX_E_HIP, "selftest: %s", hipGetErrorString(e));
    return 0;
}

int rox_time_pupil_grid(rox_system *sys, const rox_field *fld, const rox_grid *grid,
                        int32_t wvl_idx, const rox_opts *opts, const rox_out *out, void *stream,
                        int32_t launches, double *mean_ms)
{
    if (!sys || !mean_ms || launches < 1)
        return fail(ROX_E_ARG, "rox_time_pupil_grid: bad argument");
    if (opts && (opts->flags & ROX_HOST_POINTERS))
        return fail(ROX_E_ARG, "rox_time_pupil_grid needs device buffers");
    hipStream_t st = (hipStream_t)stream;
    TraceArgs a;
    auto enq = enqueue_lock(sys, st);
    int rc = prepare_grid(sys, fld, grid, wvl_idx, opts, out, st, a);
    if (rc)
        return rc;
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    HIP_TRY(hipEventRecord(e0, st));
    for (int i = 0; i < launches && !rc; ++i)
        rc = launch(sys, a, GEN_PUPIL, st);
    HIP_TRY(hipEventRecord(e1, st));
    HIP_TRY(hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *mean_ms = (double)ms / launches;
    return rc;
}

}  // extern "C"
