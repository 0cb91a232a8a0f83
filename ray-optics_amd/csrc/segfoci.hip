// segfoci.hip -- rox_segment_foci: per-segment reductions of the ROX_OUT_FULL packets of finished
// launches (include/roxtrace.h): for every (item, slot) the weighted first and second moments of the
// straight lines the rays leave the slot's interface on -- a = where a line meets the plane z = 0
// of the slot's frame, b = its slopes -- from which the host finds where between this interface and
// the next the weighted bundle is smallest (the ghost analysis' internal foci, analyses.ghost_analysis).
//
// The shape of footprint.hip (rox::PacketTile): a workgroup owns kTile consecutive rays of one
// item, kRays per thread, and walks the slots in order; of a record's 10 rows it reads p, d and dst
// once each, coalesced along the ray axis, and only of rays that count.  Each wave writes one
// partial record per slot (rox::wave_merge); the finishing kernel merges a slot's partial records in
// the fixed order of rox::block_merge (Chan / Golub / LeVeque, weighted).  No floating-point
// atomics, no LDS in the walk.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "rox_config.hpp"
#include "rox_packets.hpp"

namespace {

constexpr char kHipWhere[] = "rox_segment_foci: ";

using Tile = rox::PacketTile<4>;                // rays per thread
constexpr int kBlock = Tile::kBlock, kWaves = Tile::kWaves, kRays = Tile::kRays;
// Device scratch of one launch (partial records and records bound for host memory), or what one
// item needs where that is more: a call that needs more per launch runs as consecutive launches
// over fewer items.
constexpr size_t kSfScratchBytes = size_t(32) << 20;

struct ItemIn {
    const double *seg;
    const uint8_t *status;
    const double *weight;                       // or nullptr
    int64_t ld;
};

// a partial record: weight w with the means (ax, ay, bx, by) and the moments about them
struct Acc {
    double w, w_in;
    double ax, ay, bx, by;
    double maa, mab, mbb;
    double zi_min, zi_max, zo_min, zo_max;
    uint32_t n, n_flat, n_bad, n_in;
};                                              // 120 bytes

struct SfArgs {
    const ItemIn *items;                        // the chunk's items
    int32_t n_seg;
    int32_t n_waves;                            // per item
    int64_t n_rays;
    double hx, hy;                              // the window
    int32_t windowed;                           // 0: every counted ray is inside
    Acc *part;                                  // [items][n_waves][n_seg]
};

__device__ __forceinline__ Acc acc_empty()
{
    const double inf = __builtin_inf();
    return Acc{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, inf, -inf, inf, -inf, 0u, 0u, 0u, 0u};
}

// the moments of a <- a merged with b, a's rays first; a partial record of weight 0 has none
template <class A, class B>
__device__ __forceinline__ void moments_merge(A &a, const B &b)
{
    if (b.w > 0.0) {
        if (a.w > 0.0) {
            const double ww = a.w + b.w, f = b.w / ww, g = a.w * f;
            const double dax = b.ax - a.ax, day = b.ay - a.ay, dbx = b.bx - a.bx, dby = b.by - a.by;
            a.ax = a.ax + dax * f;
            a.ay = a.ay + day * f;
            a.bx = a.bx + dbx * f;
            a.by = a.by + dby * f;
            a.maa = (a.maa + b.maa) + (dax * dax + day * day) * g;
            a.mab = (a.mab + b.mab) + (dax * dbx + day * dby) * g;
            a.mbb = (a.mbb + b.mbb) + (dbx * dbx + dby * dby) * g;
            a.w = ww;
        } else {
            a.w = b.w;
            a.ax = b.ax; a.ay = b.ay; a.bx = b.bx; a.by = b.by;
            a.maa = b.maa; a.mab = b.mab; a.mbb = b.mbb;
        }
    }
    a.w_in = a.w_in + b.w_in;
    a.zi_min = fmin(a.zi_min, b.zi_min); a.zi_max = fmax(a.zi_max, b.zi_max);
    a.zo_min = fmin(a.zo_min, b.zo_min); a.zo_max = fmax(a.zo_max, b.zo_max);
}

__device__ __forceinline__ void acc_merge(Acc &a, const Acc &b)
{
    moments_merge(a, b);
    a.n += b.n; a.n_flat += b.n_flat; a.n_bad += b.n_bad; a.n_in += b.n_in;
}

__global__ __launch_bounds__(kBlock) void segfoci_kernel(const SfArgs a)
{
    const ItemIn it = a.items[blockIdx.y];
    const int lane = threadIdx.x & 63;
    const int n_seg = a.n_seg;

    // per ray: whether it counts (status ROX_OK and a weight that is finite and >= 0) and its weight
    int64_t r[kRays];
    bool use[kRays];
    double w[kRays];
    uint32_t n_bad = 0;
#pragma unroll
    for (int j = 0; j < kRays; ++j) {
        r[j] = Tile::ray(j);
        use[j] = false;
        w[j] = 1.0;
        if (r[j] < a.n_rays && it.status[r[j]] == ROX_OK) {
            if (it.weight)
                w[j] = it.weight[r[j]];
            use[j] = w[j] >= 0.0 && w[j] <= DBL_MAX;        // (NaN: neither)
            n_bad += use[j] ? 0u : 1u;
        }
    }

    Acc *out = a.part + Tile::part(a.n_waves, n_seg);

    for (int k = 0; k < n_seg; ++k) {
        const double *rec = it.seg + (size_t)k * ROX_SEG_DOUBLES * it.ld;
        double x[kRays], y[kRays], z[kRays], dl[kRays], dm[kRays], dn[kRays], dst[kRays];
#pragma unroll
        for (int j = 0; j < kRays; ++j) {
            x[j] = y[j] = z[j] = dl[j] = dm[j] = dn[j] = dst[j] = 0.0;
            if (use[j]) {
                x[j] = rec[r[j]];
                y[j] = rec[it.ld + r[j]];
                z[j] = rec[2 * it.ld + r[j]];
                dl[j] = rec[3 * it.ld + r[j]];
                dm[j] = rec[4 * it.ld + r[j]];
                dn[j] = rec[5 * it.ld + r[j]];
                dst[j] = rec[6 * it.ld + r[j]];
            }
        }

        // this thread's rays, each a record of its own (its a and b the means, no moments), merged
        // in the order j = 0 .. kRays - 1; then the wave's by a fixed butterfly
        Acc t = acc_empty();
        t.n_bad = n_bad;
#pragma unroll
        for (int j = 0; j < kRays; ++j) {
            if (use[j] && dn[j] == 0.0)
                t.n_flat += 1u;
            if (use[j] && dn[j] != 0.0) {
                Acc q;
                q.bx = dl[j] / dn[j];
                q.by = dm[j] / dn[j];
                q.ax = x[j] - z[j] * q.bx;                  // (-ffp-contract=off: no FMA)
                q.ay = y[j] - z[j] * q.by;
                const double zo = z[j] + dst[j] * dn[j];
                const bool in = !a.windowed || (fabs(q.ax) <= a.hx && fabs(q.ay) <= a.hy);
                q.w = w[j];
                q.w_in = in ? w[j] : 0.0;
                q.maa = q.mab = q.mbb = 0.0;
                q.zi_min = q.zi_max = z[j];
                q.zo_min = q.zo_max = zo;
                q.n = 1u; q.n_flat = 0u; q.n_bad = 0u; q.n_in = in ? 1u : 0u;
                acc_merge(t, q);
            }
        }
        rox::wave_merge(t, [](Acc &m, const Acc &b) { acc_merge(m, b); });
        if (lane == 0)
            out[k] = t;
    }
}

// what the partial records of an (item, slot) merge into: the counts in 64 bits
struct Sum {
    double w, w_in;
    double ax, ay, bx, by;
    double maa, mab, mbb;
    double zi_min, zi_max, zo_min, zo_max;
    int64_t n, n_flat, n_bad, n_in;
};

// rec[item][k] from part[item][w][k], w = 0 .. n_waves - 1, in the order of rox::block_merge
__global__ __launch_bounds__(kBlock) void segfoci_finish(const Acc *__restrict__ part, int n_waves, int n_seg,
                                                         rox_seg_focus *__restrict__ rec)
{
    __shared__ Sum lds[kBlock];
    const int k = blockIdx.x;
    const auto merge = [](Sum &m, const auto &b) {
        moments_merge(m, b);
        m.n += (int64_t)b.n; m.n_flat += (int64_t)b.n_flat; m.n_bad += (int64_t)b.n_bad; m.n_in += (int64_t)b.n_in;
    };
    const double inf = __builtin_inf();
    const Sum m = rox::block_merge<kBlock>(part + (size_t)blockIdx.y * n_waves * n_seg + k, n_waves, n_seg,
                                           Sum{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, inf, -inf, inf, -inf,
                                               0, 0, 0, 0},
                                           merge, lds);
    if (threadIdx.x == 0) {
        const double nan = __builtin_nan("");
        const bool any = m.n > 0 && m.w > 0.0;
        rox_seg_focus f;
        f.n = m.n; f.n_flat = m.n_flat; f.n_bad = m.n_bad; f.n_in = m.n_in;
        f.w_sum = m.w; f.w_in = m.w_in;
        f.a_mean[0] = any ? m.ax : nan; f.a_mean[1] = any ? m.ay : nan;
        f.b_mean[0] = any ? m.bx : nan; f.b_mean[1] = any ? m.by : nan;
        f.m_aa = any ? m.maa : nan; f.m_ab = any ? m.mab : nan; f.m_bb = any ? m.mbb : nan;
        f.z_in_min = m.zi_min; f.z_in_max = m.zi_max;
        f.z_out_min = m.zo_min; f.z_out_max = m.zo_max;
        rec[(size_t)blockIdx.y * n_seg + k] = f;
    }
}

rox::PerStream<rox::Workspace> g_sf_ws;

}  // namespace

extern "C" int rox_segment_foci(rox_system *sys, uint32_t trace_flags, int32_t n_items, const rox_out *outs,
                                int64_t n_rays, const double *weight, int64_t weight_stride, const double *window,
                                rox_seg_focus *rec, void *stream)
{
    static const char kE[] = "rox_segment_foci";
    // every argument check comes before anything touches a device
    ROX_TRY(rox::check_packet_call(kE, sys, outs, n_items));
    ROX_TRY(rox::check_packet_rays(kE, n_rays));
    if (!rec)
        return rox::host_fail(ROX_E_ARG, "%s: null rec", kE);
    if (weight && weight_stride < n_rays)
        return rox::host_fail(ROX_E_ARG, "%s: weight_stride %lld < n_rays %lld", kE, (long long)weight_stride,
                              (long long)n_rays);
    if (window)
        for (int c = 0; c < 2; ++c)
            if (!(window[c] > 0.0))
                return rox::host_fail(ROX_E_ARG, "%s: window[%d] = %g is not > 0", kE, c, window[c]);
    for (int32_t i = 0; i < n_items; ++i)
        ROX_TRY(rox::check_packet_item(kE, i, outs[i], n_rays, false));
    const rox::PacketSlots ps(sys, trace_flags);
    const int32_t n_seg = ps.n_seg;

    hipStream_t st = (hipStream_t)stream;
    rox::Turn<> ws;
    ROX_TRY(ws.take(g_sf_ws, st, kHipWhere));

    const bool host_dst = !rox::is_device(rec);
    const int n_tiles = Tile::tiles(n_rays), n_waves = n_tiles * kWaves;
    const size_t b_part = rox::up256(sizeof(Acc) * (size_t)n_waves * n_seg);
    const size_t b_rec = rox::up256(sizeof(rox_seg_focus) * (size_t)n_seg);
    const int64_t chunk = rox::chunk_for(n_items, b_part + b_rec + 256, kSfScratchBytes);

    const size_t b_tab = sizeof(ItemIn) * (size_t)n_items;
    ItemIn *d_tab;
    Acc *d_part;
    rox_seg_focus *d_rec;
    rox::Layout L;
    L.add(d_tab, rox::up256(b_tab));
    L.add(d_part, rox::up256(sizeof(Acc) * (size_t)n_waves * n_seg * chunk));
    L.add(d_rec, rox::up256(sizeof(rox_seg_focus) * (size_t)n_seg * chunk));
    ItemIn *h;
    ROX_TRY(ws.carve(L, b_tab, &h));
    for (int32_t i = 0; i < n_items; ++i)
        h[i] = ItemIn{outs[i].seg, outs[i].status, weight ? weight + (size_t)i * weight_stride : nullptr, outs[i].ld};
    ROX_TRY(ws.upload(d_tab, b_tab));

    SfArgs a{};
    a.n_seg = n_seg; a.n_waves = n_waves; a.n_rays = n_rays;
    a.hx = window ? window[0] : 0.0;
    a.hy = window ? window[1] : 0.0;
    a.windowed = window ? 1 : 0;
    a.part = d_part;
    for (int64_t i0 = 0; i0 < n_items; i0 += chunk) {
        const int64_t c = std::min<int64_t>(chunk, n_items - i0);
        a.items = d_tab + i0;
        hipLaunchKernelGGL(segfoci_kernel, dim3((unsigned)n_tiles, (unsigned)c), dim3(kBlock), 0, st, a);
        hipLaunchKernelGGL(segfoci_finish, dim3((unsigned)n_seg, (unsigned)c), dim3(kBlock), 0, st,
                           (const Acc *)d_part, n_waves, n_seg, d_rec);
        HIP_TRY(hipGetLastError());
        // this chunk's records, copied before the next chunk reuses the scratch
        HIP_TRY(hipMemcpyAsync(rec + (size_t)i0 * n_seg, d_rec, sizeof(rox_seg_focus) * (size_t)n_seg * c,
                               hipMemcpyDefault, st));
    }
    if (host_dst)
        HIP_TRY(hipStreamSynchronize(st));
    return 0;
}
