// trace_entries.hip -- the entries that trace a batch of rays (include/roxtrace.h): explicit
// rays, a pupil grid / fan, a pupil list, several grids in one launch; the ROX_HOST_POINTERS
// staging of the first three; the timing entry of include/roxtrace_diag.h.
#include <algorithm>
#include <cstring>

#include "rox_system.hpp"
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
    StageArena *arena = nullptr;
    rox_out dev{};          // staging buffers (device-visible)
    rox_out host{};         // caller's host buffers
    int64_t n = 0, rows = 0;
    bool bounce = false;    // staging lives in the pinned block
    char *in = nullptr;     // room for the staged inputs
};

// ROX_HOST_POINTERS calls are synchronous; two host threads on one stream (typically the
// NULL stream of ctypes callers) take turns with the stream's scratch -- the cached pupil
// axes as well as the staging arena -- from before the launch is prepared until the
// results are in place
int stage_lock(Staged &s, rox_system *sys, hipStream_t st)
{
    StreamCtx *cx;
    ROX_TRY(stream_ctx(sys, st, cx));
    s.lock = std::unique_lock<std::mutex>(cx->stage_mu);
    s.arena = &cx->stage;
    return 0;
}

struct HostIn { const void *src; size_t bytes; };     // one host input of a staged call

// room in the stream's arena for the results of `out` (s.dev; seg full of NaN) and, one behind
// the other from s.in on, copies of the n_in inputs `in`
int stage(Staged &s, rox_system *sys, hipStream_t st, const rox_opts *o, const rox_out *out, int64_t n,
          const HostIn *in = nullptr, int n_in = 0)
{
    s.host = *out;
    s.n = n;
    s.rows = seg_rows(sys, o);
    size_t in_bytes = 0;
    for (int i = 0; i < n_in; ++i)
        in_bytes += in[i].bytes;
    const size_t N = (size_t)n, n_seg = (size_t)s.rows * N;
    Layout lay;
    lay.add(s.dev.seg, up16(sizeof(double) * n_seg)).add(s.in, up16(in_bytes));
    if (out->op)
        lay.add(s.dev.op, up16(sizeof(double) * N));
    if (out->status)
        lay.add(s.dev.status, up16(N));
    if (out->fail_surf)
        lay.add(s.dev.fail_surf, up16(sizeof(int16_t) * N));
    if (out->pupil)
        lay.add(s.dev.pupil, up16(sizeof(double) * 2 * N));
    const size_t total = lay.size() + 16;
    s.bounce = total <= kBounceBytes;
    StageArena &ar = *s.arena;
    if (s.bounce && ar.h_cap < total) {
        size_t cap = size_t(64) << 10;
        while (cap < total)
            cap *= 2;
        HIP_TRY(regrow(ar.h, ar.h_cap, cap, cap, hipHostMallocMapped));
    } else if (!s.bounce && ar.d_cap < total) {
        HIP_TRY(regrow(ar.d, ar.d_cap, total + total / 8, total + total / 8));
    }
    lay.carve(s.bounce ? ar.h : ar.d);
    s.dev.ld = n;
    if (s.bounce) {
        std::fill_n(s.dev.seg, n_seg, __builtin_nan(""));
    } else if (n_seg) {
        hipLaunchKernelGGL(fill_nan_kernel, dim3(1024), dim3(256), 0, st, s.dev.seg, n_seg);
        HIP_TRY(hipGetLastError());
    }
    char *dst = s.in;
    for (int i = 0; i < n_in; ++i) {
        if (in[i].bytes && s.bounce) {
            memcpy(dst, in[i].src, in[i].bytes);
        } else if (in[i].bytes) {
            HIP_TRY(hipMemcpyAsync(dst, in[i].src, in[i].bytes, hipMemcpyHostToDevice, st));
        }
        dst += in[i].bytes;
    }
    return 0;
}

// the staged launch `a` (its inputs point into s.in): launch, synchronise, results to the caller
int launch_staged(Staged &s, rox_system *sys, TraceArgs &a, int gen, hipStream_t st)
{
    a.out = s.dev;
    ROX_TRY(launch(sys, a, gen, st));
    HIP_TRY(hipStreamSynchronize(st));
    // `rows` rows of s.n elements of `size` bytes each to the caller's rows, s.host.ld elements
    // apart (rows = 0: one row as a flat copy)
    auto rows_out = [&s](void *dst, const void *src, size_t size, int64_t rows) -> hipError_t {
        const size_t bytes = size * (size_t)s.n, pitch = size * (size_t)s.host.ld;
        if (!s.bounce)
            return rows ? hipMemcpy2D(dst, pitch, src, bytes, bytes, rows, hipMemcpyDeviceToHost)
                        : hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
        for (int64_t r = 0; r < (rows ? rows : 1); ++r)
            memcpy((char *)dst + r * pitch, (const char *)src + r * bytes, bytes);
        return hipSuccess;
    };
    HIP_TRY(rows_out(s.host.seg, s.dev.seg, sizeof(double), s.rows));
    if (s.host.op)
        HIP_TRY(rows_out(s.host.op, s.dev.op, sizeof(double), 0));
    if (s.host.status)
        HIP_TRY(rows_out(s.host.status, s.dev.status, 1, 0));
    if (s.host.fail_surf)
        HIP_TRY(rows_out(s.host.fail_surf, s.dev.fail_surf, sizeof(int16_t), 0));
    if (s.host.pupil)
        HIP_TRY(rows_out(s.host.pupil, s.dev.pupil, sizeof(double), 2));
    return 0;
}

}  // namespace

int rox::grid_args(rox_system *sys, const rox_field *fld, const rox_grid *grid, int32_t wvl_idx,
                   const rox_opts *opts, const rox_out *out, TraceArgs &a)
{
    if (!grid)
        return fail(ROX_E_ARG, "null argument");
    ROX_TRY(check_field(fld));
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
    ROX_TRY(check_opts(sys, opts, out, R));
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

namespace {

int prepare_grid(rox_system *sys, const rox_field *fld, const rox_grid *grid, int32_t wvl_idx,
                 const rox_opts *opts, const rox_out *out, hipStream_t st, TraceArgs &a)
{
    ROX_TRY(grid_args(sys, fld, grid, wvl_idx, opts, out, a));
    StreamCtx *cx;
    ROX_TRY(stream_ctx(sys, st, cx));
    if (grid->num > cx->axes.cap) {
        cx->axes.num = 0;
        HIP_TRY(regrow(cx->axes.d, cx->axes.cap, grid->num, sizeof(double) * 2 * (size_t)grid->num));
    }
    // trace.py:566-570 step = (stop - start)/(num - 1)
    const double sx = (grid->stop[0] - grid->start[0]) / (grid->num - 1);
    const double sy = (grid->stop[1] - grid->start[1]) / (grid->num - 1);
    double *px = cx->axes.d, *py = cx->axes.d + cx->axes.cap;
    const double key[4] = {grid->start[0], grid->start[1], sx, sy};
    if (cx->axes.num != grid->num || memcmp(key, cx->axes.key, sizeof key) != 0) {
        hipLaunchKernelGGL(pupil_axes_kernel, dim3(1), dim3(64), 0, st, grid->start[0],
                           grid->start[1], sx, sy, grid->num, px, py);
        HIP_TRY(hipGetLastError());
        memcpy(cx->axes.key, key, sizeof key);
        cx->axes.num = grid->num;
    }
    a.px = px;
    a.py = py;
    return 0;
}

}  // namespace

extern "C" {

int rox_trace_rays(rox_system *sys, int64_t n_rays, const double *pt0, const double *dir0,
                   const int32_t *wvl_idx, int32_t wvl_idx_all, const rox_opts *opts,
                   const rox_out *out, void *stream)
{
    ROX_TRY(check_opts(sys, opts, out, n_rays));
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
    ROX_TRY(stage_lock(s, sys, st));
    const size_t vb = sizeof(double) * 3 * (size_t)n_rays;
    const HostIn in[] = {{pt0, vb}, {dir0, vb}, {wvl_idx, wvl_idx ? sizeof(int32_t) * (size_t)n_rays : 0}};
    ROX_TRY(stage(s, sys, st, opts, out, n_rays, in, 3));
    a.pt0 = (const double *)s.in;
    a.dir0 = (const double *)(s.in + vb);
    a.wvl_idx = wvl_idx ? (const int32_t *)(s.in + 2 * vb) : nullptr;
    return launch_staged(s, sys, a, GEN_RAYS, st);
}

int rox_trace_pupil_grid(rox_system *sys, const rox_field *fld, const rox_grid *grid,
                         int32_t wvl_idx, const rox_opts *opts, const rox_out *out, void *stream)
{
    if (!sys)
        return fail(ROX_E_ARG, "null system");
    hipStream_t st = (hipStream_t)stream;
    TraceArgs a;
    Staged s;
    if (opts && (opts->flags & ROX_HOST_POINTERS))
        ROX_TRY(stage_lock(s, sys, st));
    auto enq = enqueue_lock(sys, st);
    ROX_TRY(prepare_grid(sys, fld, grid, wvl_idx, opts, out, st, a));
    if (!(opts->flags & ROX_HOST_POINTERS))
        return launch(sys, a, GEN_PUPIL, st);
    ROX_TRY(stage(s, sys, st, opts, out, a.n_rays));
    return launch_staged(s, sys, a, GEN_PUPIL, st);
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
    for (int32_t i = 0; i < n_grids; ++i)
        ROX_TRY(prepare_grid(sys, &flds[i], grid, wvl_idx[i], &opts[i], &outs[i], st, items[i]));
    const int64_t R = items[0].n_rays;
    const bool compact = opts[0].out_mode == ROX_OUT_HITS_COMPACT;
    if (n_grids == 1 || n_grids > 65535 || R > rays_per_launch() || R == 0) {
        // nothing to batch (or more than one launch each): the plain path, item by item
        for (int32_t i = 0; i < n_grids; ++i)
            ROX_TRY(launch(sys, items[i], GEN_PUPIL, st));
        return 0;
    }
    LaunchCfg k;
    int inst = 0;
    for (int32_t i = 0; i < n_grids; ++i) {
        ROX_TRY(launch_setup(sys, items[i], GEN_PUPIL, false, st, k, inst));
        items[i].in_ld = R;
        items[i].ray_base = 0;
    }
    StreamCtx *cx;
    ROX_TRY(stream_ctx(sys, st, cx));
    std::lock_guard<std::mutex> lock(cx->batch_mu);
    BatchItems &b = cx->batch;
    k.small = want_small(sys, (int64_t)n_grids * R, opts[0].out_mode, kInstances[inst], n_grids);
    const int bs = block_of(opts[0].out_mode, kInstances[inst], k.small);
    int64_t blocks = (R + bs - 1) / bs;
    if (opts[0].out_mode == ROX_OUT_FULL)
        for (int32_t i = 0; i < n_grids; ++i)
            items[i].tile_group = full_tile_group(k.small);
    if (compact) {
        // per-item tickets
        if ((int64_t)n_grids > b.tickets_cap)
            HIP_TRY(regrow_zeroed(b.d_tickets, b.tickets_cap, n_grids,
                                  sizeof(uint32_t) * 2 * (size_t)n_grids, st));
        // per-item look-back states; small tiles when the whole batch is small
        const int32_t small = ((int64_t)n_grids * R <= (int64_t)sys->num_cus * kSmallTile)
                                  ? compact_small_want(sys, R) : 0;
        const int64_t tiles = compact_tiles(R, small, bs);
        blocks = tiles;
        if ((int64_t)n_grids * tiles > b.tiles_cap) {
            HIP_TRY(regrow_zeroed(b.d_tiles, b.tiles_cap, n_grids * tiles,
                                  sizeof(uint64_t) * (size_t)(n_grids * tiles), st));
            b.epoch = 0;
        }
        ++b.epoch;
        for (int32_t i = 0; i < n_grids; ++i) {
            items[i].small_tiles = small;
            items[i].tile_state = b.d_tiles + (size_t)i * tiles;
            items[i].ticket = b.d_tickets + 2 * (size_t)i;
            items[i].hits_base_in = nullptr;
            items[i].hits_total_out = outs[i].n_hits;
            items[i].epoch = b.epoch;
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
    // a few items: in the kernel argument itself (rox_args.hpp BatchArgs) -- nothing to upload
    static const bool no_inline = env_flag("ROX_BATCH_NO_INLINE");  // (the A/B switch of tools/ab_bench.py)
    if (n_grids <= kInlineItems && !no_inline) {
        k.n_inline = n_grids;
        trace_fns(inst, k).batch(k, items.data());
        HIP_TRY(hipGetLastError());
        return 0;
    }
    // items -> pinned slot -> device, in stream order
    if (n_grids > b.cap) {
        const int32_t want = n_grids < 64 ? 64 : n_grids;
        HIP_TRY(release(b.d_items, b.cap));   // synchronises: the copies from h_items are done
        HIP_TRY(regrow(b.h_items, b.cap, want,
                       sizeof(TraceArgs) * (size_t)want * BatchItems::kSlots, hipHostMallocDefault));
        HIP_TRY(regrow(b.d_items, b.cap, want, sizeof(TraceArgs) * (size_t)want));
        b.last.clear();
        for (bool &live : b.ev_live)
            live = false;
    }
    // The items of a batch that repeats the previous one of this stream byte for byte (a figure
    // refreshed with unchanged arguments, a timing loop) are already in d_items: the upload -- a
    // copy-engine transfer in front of the kernel, ~6 us -- is skipped.
    const size_t items_bytes = sizeof(TraceArgs) * (size_t)n_grids;
    // ROX_BATCH_ALWAYS_UPLOAD=1 (read once) switches the short cut off: bench.py times the
    // BASELINE configurations that way, so that its figures are those of a call whose fields or
    // outputs changed.  (TraceArgs is value-initialised, padding included, before it is filled.)
    static const bool always_upload = env_flag("ROX_BATCH_ALWAYS_UPLOAD");
    const bool same_items = !always_upload && b.last.size() == items_bytes &&
                            memcmp(b.last.data(), items.data(), items_bytes) == 0;
    if (!same_items) {
        const uint32_t slot = b.slot++ % BatchItems::kSlots;
        if (!b.ev[slot])
            HIP_TRY(hipEventCreateWithFlags(&b.ev[slot], hipEventDisableTiming));
        if (b.ev_live[slot])
            HIP_TRY(hipEventSynchronize(b.ev[slot]));
        TraceArgs *h = b.h_items + (size_t)slot * b.cap;
        memcpy(h, items.data(), items_bytes);
        b.last.clear();                     // (not valid until the copy is enqueued)
        HIP_TRY(hipMemcpyAsync(b.d_items, h, items_bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipEventRecord(b.ev[slot], st));
        b.ev_live[slot] = true;
        b.last.assign(reinterpret_cast<const char *>(items.data()),
                              reinterpret_cast<const char *>(items.data()) + items_bytes);
    }
    trace_fns(inst, k).batch(k, b.d_items);
    HIP_TRY(hipGetLastError());
    return 0;
}

int rox_trace_pupil_list(rox_system *sys, const rox_field *fld, int64_t n_rays, const double *px,
                         const double *py, int32_t wvl_idx, const rox_opts *opts,
                         const rox_out *out, void *stream)
{
    ROX_TRY(check_opts(sys, opts, out, n_rays));
    ROX_TRY(check_field(fld));
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
    ROX_TRY(stage_lock(s, sys, st));
    const size_t pb = sizeof(double) * (size_t)n_rays;
    const HostIn in[] = {{px, pb}, {py, pb}};
    ROX_TRY(stage(s, sys, st, opts, out, n_rays, in, 2));
    a.px = (const double *)s.in;
    a.py = (const double *)(s.in + pb);
    return launch_staged(s, sys, a, GEN_PUPIL, st);
}

// ---- include/roxtrace_diag.h
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
    ROX_TRY(prepare_grid(sys, fld, grid, wvl_idx, opts, out, st, a));
    // (the events are destroyed on every path)
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const int rc = [&]() -> int {
        HIP_TRY(hipEventCreate(&e0));
        HIP_TRY(hipEventCreate(&e1));
        HIP_TRY(hipEventRecord(e0, st));
        int rcl = 0;
        for (int i = 0; i < launches && !rcl; ++i)
            rcl = launch(sys, a, GEN_PUPIL, st);
        HIP_TRY(hipEventRecord(e1, st));
        HIP_TRY(hipEventSynchronize(e1));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        *mean_ms = (double)ms / launches;
        return rcl;
    }();
    if (e0)
        (void)hipEventDestroy(e0);
    if (e1)
        (void)hipEventDestroy(e1);
    return rc;
}

}  // extern "C"
