// footprint.hip -- rox_surface_footprints: per-surface reductions of the ROX_OUT_FULL packets of
// finished launches (include/roxtrace.h): for every (item, slot) the count, bounding box, largest
// radius, centroid and RMS radius of the beam on that interface, the steepest incidence and exit
// angles, the rays lost there by status, and optionally numpy.histogram2d of the landing points.
// What the reference answers with four rim rays per field (vigcalc.max_aperture_at_surf,
// rayoptics/raytr/vigcalc.py:31-42) is answered here from the dense grid that is already in HBM.
//
// A workgroup (rox::PacketTile) owns kTile consecutive rays of one item, kRays per thread, and
// walks the slots in order with the previous slot's direction in registers: of a record's 10 rows
// it reads p.x, p.y, d and nrml once each, coalesced along the ray axis, and never dst or p.z.  A
// slot of a ray is read only where the ray has a record there.  Each wave writes one partial
// record per slot, its counts merged in the same butterfly as its moments (rox::wave_merge); the
// finishing kernel merges a slot's partial records in a fixed order (Chan / Golub / LeVeque for
// the centroid and the second moment, both taken about a pivot ray of the item, footprint_pivot).
// No floating-point atomics; the maps are integer atomics.  (The tile, the merges and the host's
// turn are those of every packet entry: rox_packets.hpp.)
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "rox_bins.hpp"
#include "rox_config.hpp"
#include "rox_packets.hpp"

namespace {

using rox::kRtDoubles;

constexpr char kHipWhere[] = "rox_surface_footprints: ";

using Tile = rox::PacketTile<4>;                // rays per thread
constexpr int kBlock = Tile::kBlock, kWaves = Tile::kWaves, kRays = Tile::kRays;
// Device scratch of one launch (partial records, records and maps bound for host memory): a call
// that needs more per launch runs as consecutive launches over fewer items.
constexpr size_t kFpScratchBytes = size_t(8) << 20;

struct ItemIn {
    const double *seg;
    const uint8_t *status;
    const int16_t *fail_surf;
    int64_t ld;
};

// the floating-point part of a partial record: n records with mean (mx, my) and second moment
// m2 = sum((x - mx)^2 + (y - my)^2) about it, x and y counted from the slot's pivot
struct Acc {
    double n, mx, my, m2;
    double minx, miny, maxx, maxy, r2;
    double cimin, cisum, cemin;
};

struct Part {
    Acc a;
    uint64_t nf;                                // n_fail[1..4] of the wave, 16 bits each
    uint32_t n_inc;
    uint32_t pad;
};                                              // 112 bytes

struct FpArgs {
    const ItemIn *items;                        // the chunk's items
    const double *rt;                           // [n_ifcs][kRtDoubles]
    const int32_t *nb;                          // [n_ifcs] slots before interface s
    const int32_t *slot_ifc;                    // [n_seg] interface of slot k
    const double *hw;                           // [n_seg] or nullptr
    int32_t n_ifcs, n_seg;
    int64_t n_rays;
    uint32_t flags;
    int32_t n_bins;
    int32_t n_waves;                            // per item
    Part *part;                                 // [items][n_waves][n_seg] or nullptr
    const double *pivot;                        // [items][n_seg][2]: the origin of the moments
    uint32_t *maps;                             // [items][n_seg][n_bins][n_bins] or nullptr
};

__device__ __forceinline__ Acc acc_empty()
{
    const double inf = __builtin_inf();
    return Acc{0.0, 0.0, 0.0, 0.0, inf, inf, -inf, -inf, -inf, inf, 0.0, inf};
}

// a <- a merged with b, a's records first
__device__ __forceinline__ void acc_merge(Acc &a, const Acc &b)
{
    if (b.n > 0.0) {
        if (a.n > 0.0) {
            const double nn = a.n + b.n, f = b.n / nn;
            const double dx = b.mx - a.mx, dy = b.my - a.my;
            a.mx = a.mx + dx * f;
            a.my = a.my + dy * f;
            a.m2 = (a.m2 + b.m2) + (dx * dx + dy * dy) * (a.n * f);
            a.n = nn;
        } else {
            a.n = b.n; a.mx = b.mx; a.my = b.my; a.m2 = b.m2;
        }
    }
    a.minx = fmin(a.minx, b.minx); a.miny = fmin(a.miny, b.miny);
    a.maxx = fmax(a.maxx, b.maxx); a.maxy = fmax(a.maxy, b.maxy);
    a.r2 = fmax(a.r2, b.r2);
    a.cimin = fmin(a.cimin, b.cimin);
    a.cisum = a.cisum + b.cisum;
    a.cemin = fmin(a.cemin, b.cemin);
}

// pivot[item][k] = (p.x, p.y) at slot k of one ray of the item that reached the image: the OK ray
// nearest in index to the middle of the grid (of a square product grid: its centre ray), (0, 0)
// when there is none.  The moments are accumulated about it, so that the partial means carry
// the rounding of the beam's extent, not of its distance from the axis -- a small spot far off
// axis keeps its RMS radius.  The choice depends on the item's status row alone.
__global__ __launch_bounds__(kBlock) void footprint_pivot(const ItemIn *__restrict__ items, int64_t n_rays,
                                                          int n_seg, double *__restrict__ pivot)
{
    __shared__ unsigned long long best[kBlock];
    const ItemIn it = items[blockIdx.x];
    int64_t num = (int64_t)sqrt((double)n_rays);
    while (num * num > n_rays)
        --num;
    while ((num + 1) * (num + 1) <= n_rays)
        ++num;
    const int64_t mid = num * num == n_rays ? (num / 2) * num + num / 2 : n_rays / 2;
    unsigned long long key = ~0ull;
    // the centre ray itself when it is OK (the usual case: no scan)
    const bool centre_ok = it.status[mid] == ROX_OK;
    if (centre_ok && threadIdx.x == 0)
        key = (unsigned long long)mid;
    for (int64_t r = threadIdx.x; !centre_ok && r < n_rays; r += kBlock)
        if (it.status[r] == ROX_OK) {
            const unsigned long long d = (unsigned long long)(r > mid ? r - mid : mid - r);
            const unsigned long long cand = (d << 32) | (unsigned long long)r;
            key = cand < key ? cand : key;
        }
    best[threadIdx.x] = key;
    __syncthreads();
    for (int h = kBlock / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h && best[threadIdx.x + h] < best[threadIdx.x])
            best[threadIdx.x] = best[threadIdx.x + h];
        __syncthreads();
    }
    key = best[0];
    for (int k = threadIdx.x; k < n_seg; k += kBlock) {
        double px = 0.0, py = 0.0;
        if (key != ~0ull) {
            const int64_t r = (int64_t)(key & 0xffffffffull);
            const double *rec = it.seg + (size_t)k * ROX_SEG_DOUBLES * it.ld;
            px = rec[r];
            py = rec[it.ld + r];
            if (!(fabs(px) <= DBL_MAX) || !(fabs(py) <= DBL_MAX))
                px = py = 0.0;
        }
        pivot[((size_t)blockIdx.x * n_seg + k) * 2] = px;
        pivot[((size_t)blockIdx.x * n_seg + k) * 2 + 1] = py;
    }
}

__global__ __launch_bounds__(kBlock) void footprint_kernel(const FpArgs a)
{
    const ItemIn it = a.items[blockIdx.y];
    const int lane = threadIdx.x & 63;
    const int n_seg = a.n_seg;
    const bool with_partial = (a.flags & ROX_FP_PARTIAL) != 0, ok_only = (a.flags & ROX_FP_OK_ONLY) != 0;

    // per ray: full segments, the slot of a counted partial record, the slot it failed at
    int64_t r[kRays];
    int nfull[kRays], pslot[kRays], fslot[kRays], fst[kRays];
    double pdx[kRays], pdy[kRays], pdz[kRays];
#pragma unroll
    for (int j = 0; j < kRays; ++j) {
        r[j] = Tile::ray(j);
        nfull[j] = 0; pslot[j] = -1; fslot[j] = -1; fst[j] = 0;
        pdx[j] = pdy[j] = pdz[j] = 0.0;
        if (r[j] < a.n_rays) {
            const int st = it.status[r[j]];
            const int s = it.fail_surf[r[j]];
            if (st == ROX_OK) {
                nfull[j] = n_seg;
            } else {
                const bool known = s >= 0 && s < a.n_ifcs;
                if (known && st <= ROX_EVANESCENT) {
                    fslot[j] = a.nb[s];
                    fst[j] = st;
                }
                if (known && s > 0 && !ok_only) {
                    if (st == ROX_MISSED_SURFACE) {
                        nfull[j] = a.nb[s - 1] + 1;
                    } else {
                        nfull[j] = a.nb[s];
                        pslot[j] = with_partial ? a.nb[s] : -1;
                    }
                }
            }
        }
    }

    Part *out = a.part ? a.part + Tile::part(a.n_waves, n_seg) : nullptr;
    uint32_t *maps = a.maps ? a.maps + (size_t)blockIdx.y * n_seg * a.n_bins * a.n_bins : nullptr;

    for (int k = 0; k < n_seg; ++k) {
        const double *rec = it.seg + (size_t)k * ROX_SEG_DOUBLES * it.ld;
        bool full[kRays], geo[kRays];
        double x[kRays], y[kRays], dx[kRays], dy[kRays], dz[kRays], nx[kRays], ny[kRays], nz[kRays];
#pragma unroll
        for (int j = 0; j < kRays; ++j) {
            full[j] = k < nfull[j];
            geo[j] = full[j] || k == pslot[j];
            x[j] = y[j] = 0.0;
            dx[j] = dy[j] = dz[j] = nx[j] = ny[j] = nz[j] = 0.0;
            if (geo[j]) {
                x[j] = rec[r[j]];
                y[j] = rec[it.ld + r[j]];
            }
            if (full[j] && out) {
                dx[j] = rec[3 * it.ld + r[j]];
                dy[j] = rec[4 * it.ld + r[j]];
                dz[j] = rec[5 * it.ld + r[j]];
                nx[j] = rec[7 * it.ld + r[j]];
                ny[j] = rec[8 * it.ld + r[j]];
                nz[j] = rec[9 * it.ld + r[j]];
            }
        }

        if (maps) {
            const double h = a.hw[k], step = (h + h) / (double)a.n_bins;
            uint32_t *m = maps + (size_t)k * a.n_bins * a.n_bins;
#pragma unroll
            for (int j = 0; j < kRays; ++j) {
                int b = -1;
                if (geo[j]) {
                    const int bx = rox::uniform_bin(x[j], -h, h, step, a.n_bins);
                    const int by = rox::uniform_bin(y[j], -h, h, step, a.n_bins);
                    if (bx >= 0 && by >= 0)
                        b = bx * a.n_bins + by;
                }
                rox::wave_count(m, b);          // (maps is uniform: every lane of the wave is here)
            }
        }
        if (!out)
            continue;

        // the previous slot's direction in this slot's frame: through every interface in between
        if (k >= 1)
            for (int i = a.slot_ifc[k - 1]; i < a.slot_ifc[k]; ++i) {
                const double *rt = a.rt + (size_t)i * kRtDoubles;
                const int order = rt[9] != 0.0 ? ROX_RT_C_ORDER : ROX_RT_F_ORDER;
#pragma unroll
                for (int j = 0; j < kRays; ++j) {
                    const double vx = pdx[j], vy = pdy[j], vz = pdz[j];
                    if (order == ROX_RT_C_ORDER) {
                        pdx[j] = fma(rt[2], vz, fma(rt[0], vx, fma(rt[1], vy, 0.0)));
                        pdy[j] = fma(rt[5], vz, fma(rt[3], vx, fma(rt[4], vy, 0.0)));
                        pdz[j] = fma(rt[8], vz, fma(rt[6], vx, fma(rt[7], vy, 0.0)));
                    } else {
                        pdx[j] = fma(rt[2], vz, fma(rt[1], vy, fma(rt[0], vx, 0.0)));
                        pdy[j] = fma(rt[5], vz, fma(rt[4], vy, fma(rt[3], vx, 0.0)));
                        pdz[j] = fma(rt[8], vz, fma(rt[7], vy, fma(rt[6], vx, 0.0)));
                    }
                }
            }

        // this thread's records, then the wave's by a fixed butterfly
        Acc t = acc_empty();
        uint64_t nf = 0;
        uint32_t n_inc = 0;
        double sx = 0.0, sy = 0.0;
        const double c0x = a.pivot[((size_t)blockIdx.y * n_seg + k) * 2];
        const double c0y = a.pivot[((size_t)blockIdx.y * n_seg + k) * 2 + 1];
#pragma unroll
        for (int j = 0; j < kRays; ++j) {
            if (geo[j]) {
                t.n += 1.0;
                t.minx = fmin(t.minx, x[j]); t.maxx = fmax(t.maxx, x[j]);
                t.miny = fmin(t.miny, y[j]); t.maxy = fmax(t.maxy, y[j]);
                t.r2 = fmax(t.r2, x[j] * x[j] + y[j] * y[j]);    // (-ffp-contract=off: no FMA)
                x[j] -= c0x; y[j] -= c0y;                       // from here on: about the pivot
                sx += x[j]; sy += y[j];
            }
            if (full[j]) {
                t.cemin = fmin(t.cemin, fabs(fma(dz[j], nz[j], fma(dy[j], ny[j], dx[j] * nx[j]))));
                if (k >= 1) {
                    const double ci = fabs(fma(pdz[j], nz[j], fma(pdy[j], ny[j], pdx[j] * nx[j])));
                    t.cimin = fmin(t.cimin, ci);
                    t.cisum += ci;
                    ++n_inc;
                }
                pdx[j] = dx[j]; pdy[j] = dy[j]; pdz[j] = dz[j];
            }
            if (fslot[j] == k)
                nf += uint64_t(1) << (16 * (fst[j] - 1));
        }
        if (t.n > 0.0) {
            t.mx = sx / t.n;
            t.my = sy / t.n;
#pragma unroll
            for (int j = 0; j < kRays; ++j)
                if (geo[j]) {
                    const double ex = x[j] - t.mx, ey = y[j] - t.my;
                    t.m2 += ex * ex + ey * ey;
                }
        }
        Part p{t, nf, n_inc, 0};
        rox::wave_merge(p, [](Part &m, const Part &b) {
            acc_merge(m.a, b.a);
            m.nf += b.nf;
            m.n_inc += b.n_inc;
        });
        if (lane == 0)
            out[k] = p;
    }
}

// what the partial records of an (item, slot) merge into, and its count s as either holds it
struct Sum {
    Acc a;
    int64_t c[5];                               // n_fail[1..4], n_inc
};

__device__ __forceinline__ int64_t count_of(const Sum &b, int s) { return b.c[s]; }
__device__ __forceinline__ int64_t count_of(const Part &q, int s)
{
    return s < 4 ? (int64_t)((q.nf >> (16 * s)) & 0xffff) : (int64_t)q.n_inc;
}

// fp[item][k] from part[item][w][k], w = 0 .. n_waves - 1, in the order of rox::block_merge
__global__ __launch_bounds__(kBlock) void footprint_finish(const Part *__restrict__ part, int n_waves, int n_seg,
                                                           const double *__restrict__ pivot,
                                                           rox_footprint *__restrict__ fp)
{
    __shared__ Sum lds[kBlock];
    const int k = blockIdx.x;
    const auto merge = [](Sum &m, const auto &b) {
        acc_merge(m.a, b.a);
        for (int s = 0; s < 5; ++s)
            m.c[s] += count_of(b, s);
    };
    const Sum sum = rox::block_merge<kBlock>(part + (size_t)blockIdx.y * n_waves * n_seg + k, n_waves, n_seg,
                                             Sum{acc_empty(), {0, 0, 0, 0, 0}}, merge, lds);
    if (threadIdx.x == 0) {
        const Acc m = sum.a;
        const double nan = __builtin_nan("");
        rox_footprint f;
        f.n = (int64_t)m.n;
        f.n_fail[0] = 0;
        for (int s = 0; s < 4; ++s)
            f.n_fail[s + 1] = sum.c[s];
        f.n_inc = sum.c[4];
        f.min[0] = m.minx; f.min[1] = m.miny;
        f.max[0] = m.maxx; f.max[1] = m.maxy;
        f.r2_max = m.r2;
        const bool any = m.n > 0.0;
        f.cx = any ? pivot[((size_t)blockIdx.y * n_seg + k) * 2] + m.mx : nan;
        f.cy = any ? pivot[((size_t)blockIdx.y * n_seg + k) * 2 + 1] + m.my : nan;
        f.rms_r = any ? sqrt(m.m2 / m.n) : nan;
        f.cos_inc_min = f.n_inc > 0 ? m.cimin : nan;
        f.cos_inc_sum = f.n_inc > 0 ? m.cisum : nan;
        f.cos_exit_min = m.cemin < __builtin_inf() ? m.cemin : nan;
        fp[(size_t)blockIdx.y * n_seg + k] = f;
    }
}

rox::PerStream<rox::Workspace> g_fp_ws;

}  // namespace

extern "C" int rox_surface_footprints(rox_system *sys, uint32_t trace_flags, uint32_t fp_flags, int32_t n_items,
                                      const rox_out *outs, int64_t n_rays, rox_footprint *fp,
                                      const double *half_width, int32_t n_bins, uint32_t *maps, void *stream)
{
    static const char kE[] = "rox_surface_footprints";
    // every argument check comes before anything touches a device
    ROX_TRY(rox::check_packet_call(kE, sys, outs, n_items));
    if (fp_flags & ~(ROX_FP_PARTIAL | ROX_FP_OK_ONLY))
        return rox::host_fail(ROX_E_ARG, "%s: unknown fp_flags bits 0x%x", kE,
                              fp_flags & ~(ROX_FP_PARTIAL | ROX_FP_OK_ONLY));
    ROX_TRY(rox::check_packet_rays(kE, n_rays));
    if (!fp && !maps)
        return rox::host_fail(ROX_E_ARG, "%s: null fp and maps", kE);
    for (int32_t i = 0; i < n_items; ++i)
        ROX_TRY(rox::check_packet_item(kE, i, outs[i], n_rays, true));
    const rox::PacketSlots ps(sys, trace_flags);
    const int32_t n_ifcs = ps.n_ifcs, n_seg = ps.n_seg;
    if (maps) {
        if (!half_width)
            return rox::host_fail(ROX_E_ARG, "%s: maps needs half_width", kE);
        ROX_TRY(rox::check_range(kE, "n_bins", n_bins, 1, 512));
        for (int k = 0; k < n_seg; ++k)
            if (!(std::isfinite(half_width[k]) && half_width[k] > 0.0))
                return rox::host_fail(ROX_E_ARG, "%s: half_width[%d] = %g is not finite and > 0", kE, k,
                                      half_width[k]);
    }

    hipStream_t st = (hipStream_t)stream;
    rox::Turn<> ws;
    ROX_TRY(ws.take(g_fp_ws, st, kHipWhere));

    const bool maps_host = maps && !rox::is_device(maps);
    const bool host_dst = (fp && !rox::is_device(fp)) || maps_host;
    const int n_tiles = Tile::tiles(n_rays), n_waves = n_tiles * kWaves;
    const size_t map_item = maps ? sizeof(uint32_t) * (size_t)n_seg * n_bins * n_bins : 0;
    const size_t b_part = fp ? rox::up256(sizeof(Part) * (size_t)n_waves * n_seg) : 0;
    const size_t b_fp = fp ? rox::up256(sizeof(rox_footprint) * (size_t)n_seg) : 0;
    const size_t per_item = b_part + b_fp + (maps_host ? rox::up256(map_item) : 0) + 256;
    const int64_t chunk = rox::chunk_for(n_items, per_item, kFpScratchBytes);

    // the tables, staged as one block: [items][rt][hw][nb][slot_ifc]
    const size_t o_rt = sizeof(ItemIn) * (size_t)n_items, o_hw = o_rt + sizeof(double) * kRtDoubles * n_ifcs;
    const size_t o_nb = o_hw + sizeof(double) * n_seg, o_si = o_nb + sizeof(int32_t) * n_ifcs;
    const size_t b_tab = o_si + sizeof(int32_t) * n_seg;
    char *d_tab;
    Part *d_part;
    rox_footprint *d_fp;
    uint32_t *d_maps;
    double *d_pivot;
    rox::Layout L;
    L.add(d_tab, rox::up256(b_tab));
    L.add(d_part, fp ? rox::up256(sizeof(Part) * (size_t)n_waves * n_seg * chunk) : 0);
    L.add(d_fp, fp ? rox::up256(sizeof(rox_footprint) * (size_t)n_seg * chunk) : 0);
    L.add(d_maps, maps_host ? rox::up256(map_item * chunk) : 0);
    L.add(d_pivot, fp ? rox::up256(sizeof(double) * 2 * (size_t)n_seg * chunk) : 0);
    char *h;
    ROX_TRY(ws.carve(L, b_tab, &h));
    for (int32_t i = 0; i < n_items; ++i)
        ((ItemIn *)h)[i] = ItemIn{outs[i].seg, outs[i].status, outs[i].fail_surf, outs[i].ld};
    ps.stage_rt((double *)(h + o_rt));
    for (int k = 0; k < n_seg; ++k)
        ((double *)(h + o_hw))[k] = maps ? half_width[k] : 0.0;
    for (int32_t i = 0; i < n_ifcs; ++i)
        ((int32_t *)(h + o_nb))[i] = ps.slots[n_ifcs + i];
    ps.stage_slot_ifc((int32_t *)(h + o_si));
    ROX_TRY(ws.upload(d_tab, b_tab));

    FpArgs a{};
    a.rt = (const double *)(d_tab + o_rt);
    a.hw = maps ? (const double *)(d_tab + o_hw) : nullptr;
    a.nb = (const int32_t *)(d_tab + o_nb);
    a.slot_ifc = (const int32_t *)(d_tab + o_si);
    a.n_ifcs = n_ifcs; a.n_seg = n_seg; a.n_rays = n_rays;
    a.flags = fp_flags; a.n_bins = maps ? n_bins : 0; a.n_waves = n_waves;
    a.part = fp ? d_part : nullptr;
    a.pivot = d_pivot;
    for (int64_t i0 = 0; i0 < n_items; i0 += chunk) {
        const int64_t c = std::min<int64_t>(chunk, n_items - i0);
        a.items = (const ItemIn *)d_tab + i0;
        a.maps = maps ? (maps_host ? d_maps : maps + (size_t)i0 * n_seg * n_bins * n_bins) : nullptr;
        if (maps)
            HIP_TRY(hipMemsetAsync(a.maps, 0, map_item * c, st));
        if (fp)
            hipLaunchKernelGGL(footprint_pivot, dim3((unsigned)c), dim3(kBlock), 0, st, a.items, n_rays, n_seg,
                               d_pivot);
        hipLaunchKernelGGL(footprint_kernel, dim3((unsigned)n_tiles, (unsigned)c), dim3(kBlock), 0, st, a);
        if (fp)
            hipLaunchKernelGGL(footprint_finish, dim3((unsigned)n_seg, (unsigned)c), dim3(kBlock), 0, st,
                               (const Part *)d_part, n_waves, n_seg, (const double *)d_pivot, d_fp);
        HIP_TRY(hipGetLastError());
        // this chunk's results, copied before the next chunk reuses the scratch
        if (fp)
            HIP_TRY(hipMemcpyAsync(fp + (size_t)i0 * n_seg, d_fp, sizeof(rox_footprint) * (size_t)n_seg * c,
                                   hipMemcpyDefault, st));
        if (maps_host)
            HIP_TRY(hipMemcpyAsync(maps + (size_t)i0 * n_seg * n_bins * n_bins, d_maps, map_item * c,
                                   hipMemcpyDefault, st));
    }
    if (host_dst)
        HIP_TRY(hipStreamSynchronize(st));
    return 0;
}
