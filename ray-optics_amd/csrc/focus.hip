// focus.hip -- rox_trace_through_focus and rox_trace_through_focus_grids (include/roxtrace.h): one
// trace of a pupil grid evaluated at many focus positions, the host side and its two small
// kernels (the pupil axes of several grid definitions, the finishing merge of the statistics).
// The trace itself is trace_tiles<MODE_FOCUS> of rox_kernel.hpp.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "rox_system.hpp"

#pragma clang fp contract(off)

using namespace rox;

namespace {

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
            char msg[512];
            snprintf(msg, sizeof msg, "%s", rox_last_error());
            return fail(rc, "%s: item %d: %s", item_prefix, i, msg);
        }
    }

    auto enq = enqueue_lock(sys, st);
    StreamCtx *cx;
    ROX_TRY(stream_ctx(sys, st, cx));
    LaunchCfg k;
    int inst = 0;
    for (int32_t i = 0; i < n_items; ++i)       // (the same instance for every item: same flags)
        ROX_TRY(launch_setup(sys, items[i], GEN_PUPIL, false, st, k, inst));
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
    const size_t b_items = up256(sizeof(FocusArgs) * (size_t)n_items);
    const size_t b_planes = up256(sizeof(rox_focus_plane) * (size_t)n_items * n_planes);
    const size_t b_prm = up256(sizeof(double) * prm.size()), staged = b_items + b_planes + b_prm;
    double *d_axes, *d_prm;
    FocusArgs *d_items;
    rox_focus_plane *d_planes;
    rox_focus_stats *d_stats;
    char *d_part;
    Layout dev;
    dev.add(d_axes, up256(sizeof(double) * 2 * (size_t)n_slots * g0.num))
        .add(d_items, b_items).add(d_planes, b_planes).add(d_prm, b_prm)
        .add(d_stats, stats ? up256(sizeof(rox_focus_stats) * (size_t)n_items * n_planes) : 0)
        .add(d_part, item_part * (size_t)per_launch);
    if (dev.size() > cx->focus.cap) {
        cx->focus.prm.clear();                  // the new block holds no axes
        HIP_TRY(regrow(cx->focus.d, cx->focus.cap, dev.size(), dev.size()));
    }
    dev.carve(cx->focus.d);

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
    HIP_TRY(cx->focus.h.acquire(staged));
    char *h = cx->focus.h.h;
    memcpy(h, items.data(), sizeof(FocusArgs) * (size_t)n_items);
    memcpy(h + b_items, planes, sizeof(rox_focus_plane) * (size_t)n_items * n_planes);
    memcpy(h + b_items + b_planes, prm.data(), sizeof(double) * prm.size());
    HIP_TRY(hipMemcpyAsync(d_items, h, staged, hipMemcpyHostToDevice, st));
    HIP_TRY(cx->focus.h.record(st));
    // the axes, unless the block holds them from the previous call on this context
    if (cx->focus.num != g0.num || cx->focus.prm.size() != prm.size() ||
        memcmp(cx->focus.prm.data(), prm.data(), sizeof(double) * prm.size()) != 0) {
        cx->focus.prm.clear();
        hipLaunchKernelGGL(pupil_axes_slots_kernel, dim3((unsigned)((2 * n_slots + 63) / 64)), dim3(64), 0,
                           st, (const double *)d_prm, n_slots, g0.num, d_axes);
        HIP_TRY(hipGetLastError());
        cx->focus.prm = prm;
        cx->focus.num = g0.num;
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

}  // extern "C"
