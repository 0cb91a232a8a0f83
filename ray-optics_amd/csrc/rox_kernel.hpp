// rox_kernel.hpp -- the trace kernels: the work of a workgroup on its tiles, the three __global__
// templates and the host launchers that an instance unit turns into its table entry.
#pragma once
#include <cstring>
#include <type_traits>

#include "rox_args.hpp"
#include "rox_compact.hpp"
#include "rox_math.hpp"
#include "rox_math_fast.hpp"
#include "rox_opd.hpp"
#include "rox_profiles.hpp"
#include "rox_ray.hpp"

namespace rox {

// ------------------------------------------------------------------ through focus
// rox_trace_through_focus: a lane has traced its ray once (as for ROX_OUT_FAN) and evaluates it
// at every focus plane with the very expressions of the FAN epilogue in trace_tiles() -- the
// same helpers, the same IEEE operations, a plane's foc / image_pt / wf in place of rox_opts':
// the rows are bit-identical to one FAN launch per plane.

typedef const __attribute__((address_space(4))) rox_focus_plane *ConstPlanes;

template <bool FAST, int kB, class ARGS>
__device__ __forceinline__ void focus_planes(ARGS &a, const RayEnd &e, const v3 &dir0, bool ok,
                                             uint32_t voff)
{
    const ConstPlanes planes = (ConstPlanes)a.planes;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row_bytes = a.out.ld * 8;
    const double op = e.phs + e.opl;
    const double n_ok = (double)__popcll(__ballot(ok));
    for (int k = 0; k < a.n_planes; ++k) {
        const auto &pl = planes[k];
        double x = 0.0, y = 0.0, w = 0.0;
        if (ok) {                                   // trace_tiles, ROX_OUT_FAN (analyses.py:258-262)
            w = pl.wf.kind == ROX_WF_FINITE         // (wave-uniform)
                ? wave_abr_finite_pup<FAST>(pl.wf, e.ray1_p, dir0, e.rayk_p, e.rayk_d, op)
                : wave_abr_inf_ref<FAST>(pl.wf, e.ray1_p, dir0, e.rayk_p, e.rayk_d, e.inc, e.ad, op);
            const double dist = FAST ? pl.foc * rcp_f(e.ad.z) : pl.foc / e.ad.z;
            x = (e.inc.x + dist * e.ad.x) - pl.image_pt[0];
            y = (e.inc.y + dist * e.ad.y) - pl.image_pt[1];
            if (a.focus_rows) {
                const SegOut so{reinterpret_cast<char *>(a.focus_rows) + (int64_t)k * 3 * row_bytes,
                                row_bytes, voff};
                so.put(0, 0, x);
                so.put(0, 1, y);
                so.put(0, 2, w);
            }
        }
        if (a.partial && n_ok > 0) {                // (wave-uniform)
            FocusAcc s;
            s.n = n_ok;
            s.mx = wave_sum(x) / n_ok;
            s.my = wave_sum(y) / n_ok;
            s.mw = wave_sum(w) / n_ok;
            s.sr2 = wave_sum(x * x + y * y);
            const double dx = ok ? x - s.mx : 0.0, dy = ok ? y - s.my : 0.0, dw = ok ? w - s.mw : 0.0;
            s.m2xy = wave_sum(dx * dx + dy * dy);
            s.m2w = wave_sum(dw * dw);
            double lo = ok ? w : __builtin_inf(), hi = ok ? w : -__builtin_inf();
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                lo = fmin(lo, __shfl_xor(lo, o));
                hi = fmax(hi, __shfl_xor(hi, o));
            }
            s.wmin = lo;
            s.wmax = hi;
            if (lane == 0) {
                FocusAcc *rec = reinterpret_cast<FocusAcc *>(a.partial) +
                                ((size_t)blockIdx.x * (kB / 64) + wave) * a.n_planes + k;
                *rec = focus_merge(*rec, s);        // (the host zeroes the records: n = 0)
            }
        }
    }
}

// ------------------------------------------------------------------ the kernel
// the work of one workgroup on one launch item: its share of the item's ray tiles
template <int OUT_MODE, int GEN, bool PER_RAY_WVL, int FEAT, bool SMALL, class ARGS>
__device__ __forceinline__ void trace_tiles(ARGS &a)
{
    constexpr bool kCompact = (OUT_MODE == ROX_OUT_HITS_COMPACT);
    constexpr int kB = block_of(OUT_MODE, FEAT, SMALL);     // threads per workgroup = rays per tile
    constexpr int kTrace = OUT_MODE == MODE_FOCUS ? ROX_OUT_FAN : OUT_MODE;     // what the trace keeps

    const int N = a.n_ifcs;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    // LDS of a workgroup: [the table: N rows]  the indices  [phase constants]  wavelengths
    // max-aperture thresholds  [clear-aperture thresholds]  slot map  [mu, mu^2]  [stash].
    // F_GTAB leaves the table and the phase constants in global memory and keeps the circular
    // clear-aperture thresholds, which the LDS instances write into their copy of the table,
    // in an array of their own.
    constexpr bool kGtab = (FEAT & F_GTAB) != 0;
    constexpr bool kFast = (FEAT & F_FAST) != 0;
    typedef typename std::conditional<kGtab, ctblp, tblp>::type TP;
    double *tbl_w = lds;                               // [N][kRowDoubles]
    const int nw_rows = PER_RAY_WVL ? a.n_wvls : 1;
    double *ntab_w = tbl_w + (kGtab ? 0 : (size_t)N * kRowDoubles);    // [W][N] (or [N] for one wavelength)
    double *phc_w = ntab_w + (size_t)nw_rows * N;      // [W][N][4] (F_PHASE only)
    double *wvls_w = phc_w + (((FEAT & F_PHASE) && !kGtab) ? (size_t)nw_rows * N * kPhaseConsts : 0);
    double *apthr_w = wvls_w + a.n_wvls;                // [N]
    double *aplthr_w = apthr_w + N;                     // [N][ROX_MAX_AP] (F_GTAB with F_APLIST)
    int32_t *slot_w = reinterpret_cast<int32_t *>(
        aplthr_w + ((kGtab && (FEAT & F_APLIST)) ? (size_t)N * ROX_MAX_AP : 0));
    // F_FAST: (mu, mu^2, sg) of interact_f per (wavelength row, interface), behind the slot map
    // (2 N int32 = 8 N bytes behind an 8-byte aligned start: aligned as it stands -- a pointer
    // rounded through an integer loses its LDS address space and is read with flat loads)
    double *mu_w = reinterpret_cast<double *>(slot_w + 2 * N);
    // HITS_COMPACT: two tiles' worth of packed (x, y) pairs behind them, 16-byte aligned: the
    // offset is rounded in doubles (lds is 16-byte aligned, every region before is whole doubles)
    double *end_w = mu_w + (kFast ? (size_t)nw_rows * 3 * N : 0);
    d2 *stash_w = reinterpret_cast<d2 *>(lds + (((size_t)(end_w - lds) + 1) & ~size_t(1)));

    // stage the surface table once per workgroup
    if (!kGtab)
        for (int i = threadIdx.x; i < N * kRowDoubles; i += kB)
            tbl_w[i] = a.rows[i];
    const size_t w0 = PER_RAY_WVL ? 0 : (size_t)a.wvl_idx_all * N;
    {
        for (int i = threadIdx.x; i < nw_rows * N; i += kB)
            ntab_w[i] = a.n_table[w0 + i];
        if (kFast)
            for (int i = threadIdx.x; i < nw_rows * N; i += kB) {
                const int w = i / N, sf = i - w * N;
                // (mode of the interface: rox_surface.mode is the row's first word)
                const int md = reinterpret_cast<const int32_t *>(a.rows + (size_t)sf * kRowDoubles)[0];
                const double m = (sf > 0 && md == ROX_TRANSMIT) ? a.n_table[w0 + i - 1] / a.n_table[w0 + i] : 1.0;
                mu_w[(size_t)w * 3 * N + sf] = m;
                mu_w[(size_t)w * 3 * N + N + sf] = m * m;
                mu_w[(size_t)w * 3 * N + 2 * N + sf] = (md == ROX_REFLECT) ? -1.0 : 1.0;
            }
        if ((FEAT & F_PHASE) && !kGtab)
            for (int i = threadIdx.x; i < nw_rows * N * kPhaseConsts; i += kB)
                phc_w[i] = a.ph_consts[w0 * kPhaseConsts + i];
    }
    for (int i = threadIdx.x; i < a.n_wvls; i += kB)
        wvls_w[i] = a.wvls[i];
    for (int i = threadIdx.x; i < 2 * N; i += kB)
        slot_w[i] = a.slots[i];
    for (int i = threadIdx.x; i < N; i += kB)
        apthr_w[i] = sqrt_le_threshold(
            a.rows[(size_t)i * kRowDoubles + offsetof(rox_surface, max_aperture) / 8] + a.opts.fuzz);
    if (kGtab && (FEAT & F_APLIST))
        for (int i = threadIdx.x; i < N * ROX_MAX_AP; i += kB) {
            const double *row = a.rows + (size_t)(i / ROX_MAX_AP) * kRowDoubles;
            const int k = i % ROX_MAX_AP;
            double t = 0.0;
            if (k < reinterpret_cast<const int32_t *>(row)[3]) {
                const double *ap = row + offsetof(rox_surface, ap) / sizeof(double) +
                                   (size_t)k * (sizeof(rox_aperture) / sizeof(double));
                if (reinterpret_cast<const int32_t *>(ap)[0] == ROX_AP_CIRCULAR)
                    t = sqrt_le_threshold(ap[3] + a.opts.fuzz);
            }
            aplthr_w[i] = t;
        }
    __syncthreads();
    if ((FEAT & F_APLIST) && !kGtab) {
        stage_aperture_thresholds<FEAT>(tbl_w, N, a.opts.fuzz, threadIdx.x, kB);
        __syncthreads();
    }

    CtxT<TP> c;
    if constexpr (kGtab) {
        c.tbl = (ctblp)a.rows;
        c.phc = (ctblp)a.ph_consts + w0 * kPhaseConsts;
        c.aplthr = (FEAT & F_APLIST) ? aplthr_w : nullptr;
    } else {
        c.tbl = tbl_w;
        c.phc = phc_w;
        c.aplthr = nullptr;
    }
    c.ntab = ntab_w; c.wvls = wvls_w; c.apthr = apthr_w;
    c.slot = slot_w; c.nslots_before = slot_w + N;
    c.mu = mu_w;
    c.N = N;
    const uint32_t flags = a.opts.flags;
    c.check_ap = flags & ROX_CHECK_APERTURES;
    c.intersect_obj = flags & ROX_INTERSECT_OBJ;
    c.filter_ph = (FEAT & F_PHFILT) && (flags & ROX_FILTER_PHANTOMS);
    c.first_surf = a.opts.first_surf; c.last_surf = a.opts.last_surf;
    c.eps = a.opts.eps; c.fuzz = a.opts.fuzz;
    c.probe_surf = -1;
    const int64_t ld = a.out.ld;
    const int64_t n_small = kCompact ? compact_small_tiles(a.n_rays, a.small_tiles) : 0;
    const int64_t n_tiles = kCompact ? compact_tiles(a.n_rays, a.small_tiles, kB)
                          : (a.n_rays + kB - 1) / kB;

    // HITS_COMPACT: tiles are handed out by ticket, so that the tile a workgroup
    // waits for in the look-back is always held by a running workgroup
    __shared__ int64_t s_tile;
    __shared__ int32_t s_wcnt[kB / 64];
    __shared__ uint32_t s_excl;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    for (int64_t it = 0;; ++it) {
        int64_t tile;
        if (kCompact) {
            if (threadIdx.x == 0)
                s_tile = (int64_t)atomicAdd(&a.ticket[0], 1u);
            __syncthreads();
            // (wave-uniform by construction: keep it in scalar registers across the trace)
            tile = (int64_t)__builtin_amdgcn_readfirstlane((int)s_tile);
        } else {
            tile = (int64_t)blockIdx.x + it * gridDim.x;
            if constexpr (OUT_MODE == ROX_OUT_FULL)     // (blockIdx.y: the item of a batched launch)
                tile = full_tile_map(tile, n_tiles, a.tile_group, blockIdx.y * gridDim.x % kXcds);
        }
        if (tile >= n_tiles)
            break;
        int64_t r = tile * kB + threadIdx.x;
        bool active = r < a.n_rays;
        if (kCompact) {
            const bool small = tile < n_small;
            r = (small ? tile * kSmallTile : n_small * kSmallTile + (tile - n_small) * kB) + threadIdx.x;
            active = r < a.n_rays && (!small || threadIdx.x < kSmallTile);
        }
        RayEnd e;
        SegOut so;
        so.base = reinterpret_cast<char *>(a.out.seg);
        so.row_bytes = ld * 8;
        so.voff = (uint32_t)r * 8u;
        v3 pt0{0, 0, 0}, dir0{0, 0, 1};
        int wi = a.wvl_idx_all;
        bool wi_ok = true;
        if (active) {
            // ---- ray start ---------------------------------------------------
            const int64_t rg = a.ray_base + r;
            if (GEN == GEN_PUPIL) {
                double px, py;
                if (a.axis_kind == AXIS_PRODUCT) {
                    px = a.px[a.row_begin + rg / a.axis_num];
                    py = a.py[rg % a.axis_num];
                } else {
                    px = a.px[rg];
                    py = a.py[rg];
                }
                ray_start(a.fld, flags, px, py, pt0, dir0);
                if (!kCompact && a.out.pupil) {
                    a.out.pupil[r] = px;
                    a.out.pupil[ld + r] = py;
                }
            } else {
                pt0 = v3{a.pt0[rg], a.pt0[a.in_ld + rg], a.pt0[2 * a.in_ld + rg]};
                dir0 = v3{a.dir0[rg], a.dir0[a.in_ld + rg], a.dir0[2 * a.in_ld + rg]};
            }
            if (PER_RAY_WVL) {
                wi = a.wvl_idx[rg];
                wi_ok = (wi >= 0 && wi < a.n_wvls);     // a bad index never reaches the table
                if (!wi_ok)
                    wi = 0;
            }
        }
        if constexpr (kFast)
            trace_ray_fast<kTrace, PER_RAY_WVL, FEAT>(c, so, pt0, dir0, wi, active, e);
        else if constexpr (OUT_MODE != ROX_OUT_FULL)
            trace_ray_reduced<kTrace, PER_RAY_WVL, FEAT>(c, pt0, dir0, wi, active, e);
        else
            trace_ray<kTrace, PER_RAY_WVL, FEAT>(c, so, pt0, dir0, wi, active, e);
        if (active) {
            if (PER_RAY_WVL && !wi_ok) {
                // reported as a miss at the object surface; no packet
                e.status = ROX_MISSED_SURFACE;
                e.fail_surf = 0;
                e.opl = __builtin_nan("");
            }

            // ---- per-ray outputs ---------------------------------------------
            if (e.status == ROX_OK) {
                if (OUT_MODE == ROX_OUT_LAST) {             // trace.py:214-217
                    so.pdn(0, e.inc, e.ad, e.nrm);
                    so.dst(0, 0.0);
                } else if (OUT_MODE == ROX_OUT_OPD || OUT_MODE == ROX_OUT_FAN) {
                    const double op = e.phs + e.opl;
                    so.put(0, OUT_MODE == ROX_OUT_FAN ? 2 : 0,
                           a.opts.wf.kind == ROX_WF_FINITE            // (wave-uniform)
                           ? wave_abr_finite_pup<kFast>(a.opts.wf, e.ray1_p, dir0, e.rayk_p, e.rayk_d, op)
                           : wave_abr_inf_ref<kFast>(a.opts.wf, e.ray1_p, dir0, e.rayk_p, e.rayk_d,
                                                     e.inc, e.ad, op));
                    if (OUT_MODE == ROX_OUT_FAN) {          // analyses.py:258-262
                        const double dist = kFast ? a.opts.foc * rcp_f(e.ad.z) : a.opts.foc / e.ad.z;
                        so.put(0, 0, (e.inc.x + dist * e.ad.x) - a.opts.image_pt[0]);
                        so.put(0, 1, (e.inc.y + dist * e.ad.y) - a.opts.image_pt[1]);
                    }
                } else if (OUT_MODE == ROX_OUT_HITS) {      // axisarrayfigure.py:229-238
                    const double dist = kFast ? a.opts.foc * rcp_f(e.ad.z) : a.opts.foc / e.ad.z;
                    so.put(0, 0, (e.inc.x + dist * e.ad.x) - a.opts.image_pt[0]);
                    so.put(0, 1, (e.inc.y + dist * e.ad.y) - a.opts.image_pt[1]);
                }
            }
            if (!kCompact) {
                if (a.out.op)       // op_delta = phs + opl on success; opl on failure (:236)
                    a.out.op[r] = (e.status == ROX_OK) ? e.phs + e.opl : e.opl;
                if (a.out.fail_surf)
                    a.out.fail_surf[r] = (int16_t)e.fail_surf;
            }
            if (a.out.status)
                a.out.status[r] = (uint8_t)e.status;
        }
        if constexpr (OUT_MODE == MODE_FOCUS)       // (every lane of the workgroup: wave reductions)
            focus_planes<kFast, kB>(a, e, dir0, active && e.status == ROX_OK, so.voff);

        if (kCompact) {
            // ---- stable compaction of the hits: ballot ranks within the wave, wave counts
            // through LDS, the tile's survivors packed into an LDS stash; finish_tile() then
            // finds the tile's place by decoupled look-back and copies the stash there.
            const bool ok = active && e.status == ROX_OK;
            const uint64_t mask = __ballot(ok);
            const int lrank = __popcll(mask & ((1ull << lane) - 1ull));
            if (lane == 0)
                s_wcnt[wave] = __popcll(mask);
            __syncthreads();
            int woff = 0, total = 0;
#pragma unroll
            for (int w = 0; w < kB / 64; ++w) {
                const int cnt = s_wcnt[w];
                if (w < wave)
                    woff += cnt;
                total += cnt;
            }
            woff = __builtin_amdgcn_readfirstlane(woff);        // per-wave / per-workgroup values
            total = __builtin_amdgcn_readfirstlane(total);
            d2 *stash = stash_w + (size_t)(it & 1) * kB;
            if (ok) {
                const double dist = kFast ? a.opts.foc * rcp_f(e.ad.z) : a.opts.foc / e.ad.z;
                d2 xy;
                xy.x = (e.inc.x + dist * e.ad.x) - a.opts.image_pt[0];
                xy.y = (e.inc.y + dist * e.ad.y) - a.opts.image_pt[1];
                stash[woff + lrank] = xy;
            }
            if (threadIdx.x == 0)       // the count is published at once; tile 0's is its prefix
                __hip_atomic_store(&a.tile_state[tile],
                                   ts_pack(a.epoch, tile == 0 ? TS_PREFIX : TS_AGG, (uint32_t)total),
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __syncthreads();            // the stash is complete
            // The tile looks back and copies at once.  (Deferring that until the workgroup has
            // traced its next tile, when every predecessor has long published its count, gained
            // nothing at 1024-ray tiles -- 156 vs 159 us into HBM -- and the output leaves later:
            // 332 vs 301 us into pinned memory)
            finish_tile<kB>(a, tile, total, stash, n_tiles, &s_excl);
        }
    }
    if (kCompact && threadIdx.x == 0) {
        // the last workgroup out re-arms the ticket for the next launch of this
        // stream context (every workgroup leaves exactly once, after its last draw)
        if (atomicAdd(&a.ticket[1], 1u) == gridDim.x - 1) {
            __hip_atomic_store(&a.ticket[0], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&a.ticket[1], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

template <int OUT_MODE, int GEN, bool PER_RAY_WVL, int FEAT, bool SMALL = false>
__global__ void __launch_bounds__(block_of(OUT_MODE, FEAT, SMALL), min_waves_of(OUT_MODE, FEAT, SMALL))
ROX_KERNEL_ALIGNED trace_kernel(const TraceArgs a)
{
    trace_tiles<OUT_MODE, GEN, PER_RAY_WVL, FEAT, SMALL>(a);
}

// One launch for several pupil grids of one system -- the (field x wavelength) loops of
// SequentialModel.trace_grid / trace_wavefront (rayoptics/seq/sequential.py:1058-1114) and of
// the figures that call them per field: blockIdx.y picks the item, blockIdx.x strides over
// that item's tiles.  The items sit in device memory and are read through the constant
// address space, i.e. with the same scalar loads that read a kernel argument -- or, a small
// batch, travel in the kernel argument itself (rox_args.hpp BatchArgs).
typedef const __attribute__((address_space(4))) TraceArgs *ConstTraceArgs;
template <int OUT_MODE, int FEAT, bool SMALL = false>
__global__ void __launch_bounds__(block_of(OUT_MODE, FEAT, SMALL), min_waves_of(OUT_MODE, FEAT, SMALL))
ROX_KERNEL_ALIGNED trace_kernel_batch(const BatchArgs b)
{
    // (the argument block read in place, with a wave-uniform index: scalar loads either way)
    typedef const __attribute__((address_space(4))) char *cbytes;
    const ConstTraceArgs inl =
        (ConstTraceArgs)((cbytes)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(BatchArgs, inl));
    const ConstTraceArgs items = b.items ? (ConstTraceArgs)b.items : inl;
    trace_tiles<OUT_MODE, GEN_PUPIL, false, FEAT, SMALL>(items[blockIdx.y]);
}

// The through-focus kernel (rox_trace_through_focus with one item, rox_trace_through_focus_grids
// with several): pupil grids at one wavelength each, regular workgroups only.  blockIdx.y picks
// the item, blockIdx.x strides over that item's tiles -- the workgroup count per item and the
// partial records, indexed by blockIdx.x, depend on the item's grid alone, so an item's rows and
// statistics are the same whichever items are launched beside it.  The items sit in device
// memory and are read through the constant address space (trace_kernel_batch's scalar loads);
// none travel in the kernel argument: the planes need an upload in front of the kernel anyway,
// and the items ride in the same copy.
typedef const __attribute__((address_space(4))) FocusArgs *ConstFocusArgs;
template <int FEAT>
__global__ void __launch_bounds__(block_of(MODE_FOCUS, FEAT), min_waves_of(MODE_FOCUS, FEAT))
ROX_KERNEL_ALIGNED focus_kernel(const FocusArgs *items)
{
    trace_tiles<MODE_FOCUS, GEN_PUPIL, false, FEAT, false>(((ConstFocusArgs)items)[blockIdx.y]);
}

// ------------------------------------------------------------------ launching
// Tables beyond ~110 interfaces need more than the 64 KiB of dynamic LDS a kernel may
// use by default (gfx950 has 160 KiB per CU): the limit of the instance is raised once.
constexpr size_t kDefaultDynLds = 64 * 1024;
template <class K>
inline void launch_with_lds(K kernel, const dim3 &grid, const dim3 &block, size_t lds,
                            hipStream_t st, const TraceArgs &a)
{
    if (lds > kDefaultDynLds)
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kernel, grid, block, lds, st, a);
}

// the small-workgroup kernels exist for the modes whose regular workgroup is larger
// (per-ray-wavelength lists keep to the regular one)
template <int OUT_MODE, int GEN, bool PRW, int FEAT>
inline void launch_one(const LaunchCfg &k, const TraceArgs &a)
{
    if constexpr (!PRW && has_small(OUT_MODE, FEAT)) {
        if (k.small) {
            constexpr int bs = block_of(OUT_MODE, FEAT, true);
            auto kern = trace_kernel<OUT_MODE, GEN, PRW, FEAT, true>;
            launch_with_lds(kern, k.grid, dim3(bs), k.lds, k.stream, a);
            return;
        }
    }
    constexpr int bs = block_of(OUT_MODE, FEAT);
    auto kern = trace_kernel<OUT_MODE, GEN, PRW, FEAT, false>;
    launch_with_lds(kern, k.grid, dim3(bs), k.lds, k.stream, a);
}

// (FEAT: the instance's feature set | F_FAST for a tolerance-mode instance | F_GTAB for the
// instance of tables beyond the LDS; whether a mode's kernel reads the table through scalar
// loads is gtab_of()'s per-mode decision)
template <int GEN, bool PRW, int FEAT>
inline void launch_mode(const LaunchCfg &k, const TraceArgs &a)
{
    constexpr bool kF = (FEAT & F_FAST) != 0;
    constexpr int FR = FEAT | gtab_of(FEAT, kF, ROX_OUT_HITS), FF = FEAT | gtab_of(FEAT, kF, ROX_OUT_FULL);
    switch (k.out_mode) {
    case ROX_OUT_FULL: launch_one<ROX_OUT_FULL, GEN, PRW, FF>(k, a); break;
    case ROX_OUT_LAST: launch_one<ROX_OUT_LAST, GEN, PRW, FR>(k, a); break;
    case ROX_OUT_OPD: launch_one<ROX_OUT_OPD, GEN, PRW, FR>(k, a); break;
    case ROX_OUT_HITS_COMPACT: launch_one<ROX_OUT_HITS_COMPACT, GEN, PRW, FR>(k, a); break;
    case ROX_OUT_FAN: launch_one<ROX_OUT_FAN, GEN, PRW, FR>(k, a); break;
    default: launch_one<ROX_OUT_HITS, GEN, PRW, FR>(k, a); break;
    }
}

// all (output mode, ray source) variants of one feature instance
template <int FEAT>
inline void launch_instance(const LaunchCfg &k, const TraceArgs &a)
{
    if (k.gen == GEN_PUPIL)
        launch_mode<GEN_PUPIL, false, FEAT>(k, a);
    else if (k.per_ray_wvl)
        launch_mode<GEN_RAYS, true, FEAT>(k, a);
    else
        launch_mode<GEN_RAYS, false, FEAT>(k, a);
}

// the through-focus kernel of one feature instance (the table source of its reduced-output
// modes): `items` is a DEVICE array of k.grid.y FocusArgs
template <int FEAT>
inline void launch_instance_focus(const LaunchCfg &k, const FocusArgs *items)
{
    constexpr int FR = FEAT | gtab_of(FEAT, (FEAT & F_FAST) != 0, ROX_OUT_HITS);
    auto kern = focus_kernel<FR>;
    if (k.lds > kDefaultDynLds)
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.lds);
    hipLaunchKernelGGL(kern, k.grid, dim3(block_of(MODE_FOCUS, FR)), k.lds, k.stream, items);
}

// the batched form (trace_kernel_batch): pupil grids, one wavelength per item
// the host-side argument block of a batched launch: one zero-initialised 16 KB block per host
// thread (the launch copies its argument before it returns; inl beyond n_inline is never read by
// the kernel and keeps what an earlier launch left there)
inline BatchArgs &batch_args_block()
{
    static thread_local BatchArgs b{};
    return b;
}

template <class K>
inline void launch_batch_with_lds(K kernel, const dim3 &grid, const dim3 &block, size_t lds,
                                  hipStream_t st, const TraceArgs *items, int n_inline)
{
    if (lds > kDefaultDynLds)
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    BatchArgs &b = batch_args_block();
    b.items = n_inline > 0 ? nullptr : items;
    if (n_inline > 0)
        memcpy(b.inl, items, sizeof(TraceArgs) * (size_t)n_inline);
    hipLaunchKernelGGL(kernel, grid, block, lds, st, b);
}

template <int OUT_MODE, int FEAT>
inline void launch_one_batch(const LaunchCfg &k, const TraceArgs *items)
{
    if constexpr (has_small(OUT_MODE, FEAT)) {
        if (k.small) {
            constexpr int bs = block_of(OUT_MODE, FEAT, true);
            auto kern = trace_kernel_batch<OUT_MODE, FEAT, true>;
            launch_batch_with_lds(kern, k.grid, dim3(bs), k.lds, k.stream, items, k.n_inline);
            return;
        }
    }
    constexpr int bs = block_of(OUT_MODE, FEAT);
    auto kern = trace_kernel_batch<OUT_MODE, FEAT, false>;
    launch_batch_with_lds(kern, k.grid, dim3(bs), k.lds, k.stream, items, k.n_inline);
}

template <int FEAT>
inline void launch_instance_batch(const LaunchCfg &k, const TraceArgs *items)
{
    constexpr bool kF = (FEAT & F_FAST) != 0;
    constexpr int FR = FEAT | gtab_of(FEAT, kF, ROX_OUT_HITS), FF = FEAT | gtab_of(FEAT, kF, ROX_OUT_FULL);
    switch (k.out_mode) {
    case ROX_OUT_FULL: launch_one_batch<ROX_OUT_FULL, FF>(k, items); break;
    case ROX_OUT_LAST: launch_one_batch<ROX_OUT_LAST, FR>(k, items); break;
    case ROX_OUT_OPD: launch_one_batch<ROX_OUT_OPD, FR>(k, items); break;
    case ROX_OUT_HITS_COMPACT: launch_one_batch<ROX_OUT_HITS_COMPACT, FR>(k, items); break;
    case ROX_OUT_FAN: launch_one_batch<ROX_OUT_FAN, FR>(k, items); break;
    default: launch_one_batch<ROX_OUT_HITS, FR>(k, items); break;
    }
}

// what a translation unit csrc/inst_<name>.hip / fast_<name>.hip defines for its instance
// (rox_args.hpp TraceInstanceFns)
#define ROX_TRACE_INSTANCE(name, FEAT)                                                         \
    TraceInstanceFns trace_##name = {launch_instance<FEAT>, launch_instance_batch<FEAT>, \
                                     launch_instance_focus<FEAT>};

}  // namespace rox
