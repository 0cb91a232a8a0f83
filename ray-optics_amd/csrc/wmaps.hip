// wmaps.hip -- rox_weighted_maps: exact weighted histograms of the ROX_OUT_FULL packets of finished
// launches (include/roxtrace.h): numpy.histogram2d(weights=) of the points the OK rays of an item
// reach one slot at, several items into one map if the caller says so, summed in 64-bit fixed
// point.  A weight is quantised once to an integer at a power-of-two scale chosen per map from the
// map's largest weight, and integers are added: the sums are exact, so the maps do not depend on
// the order of rays, waves, workgroups, atomics or launches, nor on which of the two scatter
// paths below a workgroup takes.
//
// Pass 1 (wmaps_vmax, wmaps_vmax_finish, wmaps_scale): the largest usable v = weight * factor of
// every item, per wave, then per item by rox::block_merge, then per map with its scale exponent.
// A maximum is an exact selection.  Pass 2 (wmaps_kernel): the tile of rox::PacketTile --
// a workgroup owns kTile consecutive rays of one item, kRays per thread; it reads status, weight
// and the slot's p.x and p.y, of OK rays only.  Where the bins its rays fall into span a box of at
// most kLdsBins bins the workgroup sums them in LDS (64-bit integer adds and a 32-bit count) and
// adds the box's occupied bins to the map with global integer adds, consecutive threads on
// consecutive addresses of a map row; otherwise every wave adds to the map directly, its lanes
// that share a bin merged first (rox::wave_add).  The item records are integer sums too.  No
// floating-point atomics.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>
#include <cstring>

#include "rox_bins.hpp"
#include "rox_config.hpp"
#include "rox_packets.hpp"

namespace {

constexpr char kHipWhere[] = "rox_weighted_maps: ";

using Tile = rox::PacketTile<4>;                // rays per thread
constexpr int kBlock = Tile::kBlock, kWaves = Tile::kWaves, kRays = Tile::kRays;
// the LDS window of a workgroup: 12 bytes per bin, 48 KiB -- three workgroups per CU
constexpr int kLdsBins = 4096;
// Device scratch of one launch (pass 1's partial maxima; maps bound for host memory), or what one
// item / one map needs where that is more: larger jobs run as consecutive launches.
constexpr size_t kWmScratchBytes = size_t(32) << 20;

enum { kPathAuto = 0, kPathLds = 1, kPathGlobal = 2 };

struct ItemIn {
    const double *seg;
    const uint8_t *status;
    const double *weight;                       // or nullptr
    int64_t ld;
    double factor;
    int32_t map;
    int32_t idx;                                // the item's place in the caller's order
};

struct WmArgs {
    const ItemIn *items;                        // the launch's items, sorted by map
    const double *window;                       // [n_maps][4]
    const int32_t *scale;                       // [n_maps]
    int64_t n_rays;
    int32_t slot, nbx, nby;
    int32_t map0;                               // wmaps and counts start at this map
    int32_t path;
    unsigned long long *wmaps;                  // or nullptr
    uint32_t *counts;                           // or nullptr
    rox_wmap_item *item;                        // [n_items] in the caller's order
};

// whether a ray of weight w and value v = w * factor is usable (NaN: not)
__device__ __forceinline__ bool usable(double w, double v) { return w >= 0.0 && w <= DBL_MAX && v <= DBL_MAX; }

// part[item][wave] = the largest usable v of the wave's rays, -1 where it has none
__global__ __launch_bounds__(kBlock) void wmaps_vmax(const ItemIn *__restrict__ items, int64_t n_rays, int n_waves,
                                                     double *__restrict__ part)
{
    const ItemIn it = items[blockIdx.y];
    double vm = -1.0;
#pragma unroll
    for (int j = 0; j < kRays; ++j) {
        const int64_t r = Tile::ray(j);
        if (r < n_rays && it.status[r] == ROX_OK) {
            const double w = it.weight ? it.weight[r] : 1.0;
            const double v = w * it.factor;
            if (usable(w, v))
                vm = fmax(vm, v);
        }
    }
    for (int o = 32; o > 0; o >>= 1)
        vm = fmax(vm, __shfl_xor(vm, o));
    if ((threadIdx.x & 63) == 0)
        part[Tile::part(n_waves, 1)] = vm;
}

// vitem[item] from part[item][w], w = 0 .. n_waves - 1
__global__ __launch_bounds__(kBlock) void wmaps_vmax_finish(const double *__restrict__ part, int n_waves,
                                                            double *__restrict__ vitem)
{
    __shared__ double lds[kBlock];
    const auto merge = [](double &m, const double &b) { m = fmax(m, b); };
    const double vm = rox::block_merge<kBlock>(part + (size_t)blockIdx.x * n_waves, n_waves, 1, -1.0, merge, lds);
    if (threadIdx.x == 0)
        vitem[blockIdx.x] = vm;
}

// scale[m] from the maxima of map m's items first[m] .. first[m + 1] - 1 (one wave per map)
__global__ __launch_bounds__(64) void wmaps_scale(const double *__restrict__ vitem, const int32_t *__restrict__ first,
                                                  const int32_t *__restrict__ clog2, int32_t *__restrict__ scale)
{
    const int m = blockIdx.x;
    double vm = -1.0;
    for (int i = first[m] + (int)threadIdx.x; i < first[m + 1]; i += 64)
        vm = fmax(vm, vitem[i]);
    for (int o = 32; o > 0; o >>= 1)
        vm = fmax(vm, __shfl_xor(vm, o));
    if (threadIdx.x == 0) {
        int e = 0;
        if (vm > 0.0) {
            int E;
            (void)frexp(vm, &E);
            e = 61 - clog2[m] - E;
            e = e < -1000 ? -1000 : (e > 1000 ? 1000 : e);
        }
        scale[m] = e;
    }
}

__global__ __launch_bounds__(kBlock) void wmaps_kernel(const WmArgs a)
{
    __shared__ unsigned long long s_sum[kLdsBins];
    __shared__ uint32_t s_cnt[kLdsBins];
    __shared__ int s_box[kWaves][4];
    __shared__ unsigned long long s_rec[kWaves][5];

    const ItemIn it = a.items[blockIdx.y];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = it.map, nbx = a.nbx, nby = a.nby;
    const double *win = a.window + 4 * (size_t)m;
    const double lox = win[0] - win[2], hix = win[0] + win[2], stx = (hix - lox) / (double)nbx;
    const double loy = win[1] - win[3], hiy = win[1] + win[3], sty = (hiy - loy) / (double)nby;
    const int e = a.scale[m];
    const double *rec = it.seg + (size_t)a.slot * ROX_SEG_DOUBLES * it.ld;

    int bx[kRays], by[kRays];
    unsigned long long q[kRays];
    unsigned long long n_in = 0, n_out = 0, n_bad = 0, q_in = 0, q_out = 0;
    int x0 = nbx, x1 = -1, y0 = nby, y1 = -1;
#pragma unroll
    for (int j = 0; j < kRays; ++j) {
        const int64_t r = Tile::ray(j);
        bx[j] = by[j] = -1;
        q[j] = 0;
        if (r < a.n_rays && it.status[r] == ROX_OK) {
            const double w = it.weight ? it.weight[r] : 1.0;
            const double v = w * it.factor;
            if (!usable(w, v)) {
                ++n_bad;
                continue;
            }
            q[j] = (unsigned long long)llrint(ldexp(v, e));
            const int gx = rox::uniform_bin(rec[r], lox, hix, stx, nbx);
            const int gy = rox::uniform_bin(rec[it.ld + r], loy, hiy, sty, nby);
            if (gx >= 0 && gy >= 0) {
                bx[j] = gx; by[j] = gy;
                x0 = min(x0, gx); x1 = max(x1, gx);
                y0 = min(y0, gy); y1 = max(y1, gy);
                ++n_in; q_in += q[j];
            } else {
                ++n_out; q_out += q[j];
            }
        }
    }

    // the item's record: the wave's sums, then the workgroup's, then one integer add each
    for (int o = 32; o > 0; o >>= 1) {
        n_in += __shfl_xor(n_in, o); n_out += __shfl_xor(n_out, o); n_bad += __shfl_xor(n_bad, o);
        q_in += __shfl_xor(q_in, o); q_out += __shfl_xor(q_out, o);
        x0 = min(x0, __shfl_xor(x0, o)); x1 = max(x1, __shfl_xor(x1, o));
        y0 = min(y0, __shfl_xor(y0, o)); y1 = max(y1, __shfl_xor(y1, o));
    }
    if (lane == 0) {
        s_rec[wave][0] = n_in; s_rec[wave][1] = n_out; s_rec[wave][2] = n_bad;
        s_rec[wave][3] = q_in; s_rec[wave][4] = q_out;
        s_box[wave][0] = x0; s_box[wave][1] = x1; s_box[wave][2] = y0; s_box[wave][3] = y1;
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        unsigned long long s = 0;
        for (int w = 0; w < kWaves; ++w)
            s += s_rec[w][threadIdx.x];
        if (s)
            atomicAdd((unsigned long long *)&a.item[it.idx] + threadIdx.x, s);
    }
    if (!a.wmaps && !a.counts)
        return;
    for (int w = 0; w < kWaves; ++w) {
        x0 = min(x0, s_box[w][0]); x1 = max(x1, s_box[w][1]);
        y0 = min(y0, s_box[w][2]); y1 = max(y1, s_box[w][3]);
    }
    if (x1 < x0)
        return;                                 // none of the tile's rays is binned

    const size_t base = (size_t)(m - a.map0) * nbx * nby;
    unsigned long long *gsum = a.wmaps ? a.wmaps + base : nullptr;
    uint32_t *gcnt = a.counts ? a.counts + base : nullptr;
    const int bh = y1 - y0 + 1, n_box = (x1 - x0 + 1) * bh;      // (<= 2^20)
    if (a.path != kPathGlobal && n_box <= kLdsBins) {
        for (int i = threadIdx.x; i < n_box; i += kBlock) {
            s_sum[i] = 0;
            s_cnt[i] = 0;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kRays; ++j)
            if (bx[j] >= 0) {
                const int i = (bx[j] - x0) * bh + (by[j] - y0);
                atomicAdd(&s_sum[i], q[j]);
                atomicAdd(&s_cnt[i], 1u);
            }
        __syncthreads();
        for (int i = threadIdx.x; i < n_box; i += kBlock) {
            const uint32_t c = s_cnt[i];
            if (c) {
                const size_t g = (size_t)(x0 + i / bh) * nby + (y0 + i % bh);
                if (gsum)
                    atomicAdd(&gsum[g], s_sum[i]);
                if (gcnt)
                    atomicAdd(&gcnt[g], c);
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < kRays; ++j) {
            const int b = bx[j] >= 0 ? bx[j] * nby + by[j] : -1;
            if (gsum)
                rox::wave_add(gsum, gcnt, b, q[j]);
            else
                rox::wave_count(gcnt, b);
        }
    }
}

// ROX_WMAPS_PATH=lds / global forces one scatter path of wmaps_kernel (experiments, tests; read
// per call: tests flip it).  lds: the LDS window wherever the tile's box fits it.  The results
// are the same bits either way.
int forced_path()
{
    const char *e = getenv("ROX_WMAPS_PATH");
    if (e && !strcmp(e, "lds"))
        return kPathLds;
    if (e && !strcmp(e, "global"))
        return kPathGlobal;
    return kPathAuto;
}

rox::PerStream<rox::Workspace> g_wm_ws;

}  // namespace

extern "C" int rox_weighted_maps(rox_system *sys, uint32_t trace_flags, int32_t n_items, const rox_out *outs,
                                 int64_t n_rays, int32_t slot, const double *weight, int64_t weight_stride,
                                 const double *item_factor, const int32_t *item_map, int32_t n_maps,
                                 const double *window, int32_t nbx, int32_t nby, int64_t *wmaps, uint32_t *counts,
                                 int32_t *scale_exp, rox_wmap_item *item, void *stream)
{
    static const char kE[] = "rox_weighted_maps";
    // every argument check comes before anything touches a device
    ROX_TRY(rox::check_packet_call(kE, sys, outs, n_items));
    ROX_TRY(rox::check_packet_rays(kE, n_rays));
    if (!wmaps && !counts && !item)
        return rox::host_fail(ROX_E_ARG, "%s: null wmaps, counts and item", kE);
    if (wmaps && !scale_exp)
        return rox::host_fail(ROX_E_ARG, "%s: wmaps needs scale_exp", kE);
    if (weight && weight_stride < n_rays)
        return rox::host_fail(ROX_E_ARG, "%s: weight_stride %lld < n_rays %lld", kE, (long long)weight_stride,
                              (long long)n_rays);
    ROX_TRY(rox::check_range(kE, "n_maps", n_maps, 1, ROX_MAX_FOCUS_ITEMS));
    ROX_TRY(rox::check_range(kE, "nbx", nbx, 1, 1024));
    ROX_TRY(rox::check_range(kE, "nby", nby, 1, 1024));
    if (!item_map && n_maps != n_items)
        return rox::host_fail(ROX_E_ARG, "%s: n_maps %d != n_items %d without item_map", kE, n_maps, n_items);
    if (!window)
        return rox::host_fail(ROX_E_ARG, "%s: null window", kE);
    for (int32_t m = 0; m < n_maps; ++m) {
        const double *w = window + 4 * (size_t)m;
        for (int c = 0; c < 4; ++c)
            if (!std::isfinite(w[c]) || (c >= 2 && !(w[c] > 0.0)))
                return rox::host_fail(ROX_E_ARG, "%s: window[%d][%d] = %g is not finite%s", kE, m, c, w[c],
                                      c >= 2 ? " and > 0" : "");
        for (int c = 0; c < 2; ++c) {
            const double lo = w[c] - w[c + 2], hi = w[c] + w[c + 2];
            if (!std::isfinite(hi - lo) || !(hi > lo))
                return rox::host_fail(ROX_E_ARG, "%s: window[%d]: the edges %g and %g do not span a finite range", kE,
                                      m, lo, hi);
        }
    }
    for (int32_t i = 0; i < n_items; ++i) {
        ROX_TRY(rox::check_packet_item(kE, i, outs[i], n_rays, false));
        if (item_factor && !(std::isfinite(item_factor[i]) && item_factor[i] >= 0.0))
            return rox::host_fail(ROX_E_ARG, "%s: item %d: item_factor %g is not finite and >= 0", kE, i,
                                  item_factor[i]);
        if (item_map && (item_map[i] < 0 || item_map[i] >= n_maps))
            return rox::host_fail(ROX_E_ARG, "%s: item %d: item_map %d outside [0, %d)", kE, i, item_map[i], n_maps);
    }
    const rox::PacketSlots ps(sys, trace_flags);
    const int32_t n_seg = ps.n_seg;
    if (slot < -1 || slot >= n_seg)
        return rox::host_fail(ROX_E_ARG, "%s: slot %d outside [-1, %d)", kE, slot, n_seg);

    hipStream_t st = (hipStream_t)stream;
    rox::Turn<> ws;
    ROX_TRY(ws.take(g_wm_ws, st, kHipWhere));

    const bool w_host = wmaps && !rox::is_device(wmaps), c_host = counts && !rox::is_device(counts);
    const bool e_host = scale_exp && !rox::is_device(scale_exp), i_host = item && !rox::is_device(item);
    const size_t nb = (size_t)nbx * nby;
    const int n_tiles = Tile::tiles(n_rays), n_waves = n_tiles * kWaves;
    // pass 1 runs over chunk1 items per launch, pass 2 over the items of chunk2 maps
    const int64_t chunk1 = rox::chunk_for(n_items, rox::up256(sizeof(double) * (size_t)n_waves), kWmScratchBytes);
    const size_t map_host = (w_host ? sizeof(int64_t) * nb : 0) + (c_host ? sizeof(uint32_t) * nb : 0);
    const int64_t chunk2 = map_host ? rox::chunk_for(n_maps, map_host, kWmScratchBytes) : n_maps;

    // the tables, staged as one block: [items, sorted by map][window][first][clog2]
    const size_t o_win = sizeof(ItemIn) * (size_t)n_items, o_first = o_win + sizeof(double) * 4 * n_maps;
    const size_t o_clog = o_first + sizeof(int32_t) * ((size_t)n_maps + 1), b_tab = o_clog + sizeof(int32_t) * n_maps;
    char *d_tab;
    double *d_part, *d_vitem;
    int32_t *d_scale;
    rox_wmap_item *d_item;
    unsigned long long *d_w;
    uint32_t *d_c;
    rox::Layout L;
    L.add(d_tab, rox::up256(b_tab));
    L.add(d_part, rox::up256(sizeof(double) * (size_t)n_waves * chunk1));
    L.add(d_vitem, rox::up256(sizeof(double) * (size_t)n_items));
    L.add(d_scale, rox::up256(sizeof(int32_t) * (size_t)n_maps));
    L.add(d_item, rox::up256(sizeof(rox_wmap_item) * (size_t)n_items));
    L.add(d_w, w_host ? rox::up256(sizeof(int64_t) * nb * chunk2) : 0);
    L.add(d_c, c_host ? rox::up256(sizeof(uint32_t) * nb * chunk2) : 0);
    char *h;
    ROX_TRY(ws.carve(L, b_tab, &h));
    ItemIn *h_items = (ItemIn *)h;
    int32_t *h_first = (int32_t *)(h + o_first), *h_clog = (int32_t *)(h + o_clog);
    // a counting sort of the items by their map, stable: h_first[m] = the first item of map m
    for (int32_t m = 0; m <= n_maps; ++m)
        h_first[m] = 0;
    for (int32_t i = 0; i < n_items; ++i)
        ++h_first[(item_map ? item_map[i] : i) + 1];
    for (int32_t m = 0; m < n_maps; ++m) {
        // N = n_rays * the map's items; clog2 = ceil(log2(N)), 0 for a map without items
        const uint64_t N = (uint64_t)n_rays * (uint64_t)h_first[m + 1];
        int32_t c = 0;
        while (c < 63 && (uint64_t(1) << c) < N)
            ++c;
        h_clog[m] = c;
        h_first[m + 1] += h_first[m];
    }
    {
        std::vector<int32_t> at(h_first, h_first + n_maps);
        for (int32_t i = 0; i < n_items; ++i) {
            const int32_t m = item_map ? item_map[i] : i;
            const double *w = weight ? weight + (size_t)i * weight_stride : nullptr;
            h_items[at[m]++] = ItemIn{outs[i].seg, outs[i].status, w, outs[i].ld, item_factor ? item_factor[i] : 1.0, m, i};
        }
    }
    memcpy(h + o_win, window, sizeof(double) * 4 * (size_t)n_maps);
    ROX_TRY(ws.upload(d_tab, b_tab));
    const ItemIn *d_items = (const ItemIn *)d_tab;
    const int32_t *d_first = (const int32_t *)(d_tab + o_first);

    for (int64_t i0 = 0; i0 < n_items; i0 += chunk1) {
        const int64_t c = std::min<int64_t>(chunk1, n_items - i0);
        hipLaunchKernelGGL(wmaps_vmax, dim3((unsigned)n_tiles, (unsigned)c), dim3(kBlock), 0, st, d_items + i0, n_rays,
                           n_waves, d_part);
        hipLaunchKernelGGL(wmaps_vmax_finish, dim3((unsigned)c), dim3(kBlock), 0, st, (const double *)d_part, n_waves,
                           d_vitem + i0);
    }
    hipLaunchKernelGGL(wmaps_scale, dim3((unsigned)n_maps), dim3(64), 0, st, (const double *)d_vitem, d_first,
                       (const int32_t *)(d_tab + o_clog), d_scale);
    HIP_TRY(hipGetLastError());

    rox_wmap_item *k_item = (item && !i_host) ? item : d_item;
    HIP_TRY(hipMemsetAsync(k_item, 0, sizeof(rox_wmap_item) * (size_t)n_items, st));
    WmArgs a{};
    a.window = (const double *)(d_tab + o_win);
    a.scale = d_scale;
    a.n_rays = n_rays;
    a.slot = slot < 0 ? n_seg - 1 : slot;
    a.nbx = nbx; a.nby = nby;
    a.path = forced_path();
    a.item = k_item;
    for (int64_t m0 = 0; m0 < n_maps; m0 += chunk2) {
        const int64_t c = std::min<int64_t>(chunk2, n_maps - m0);
        a.map0 = (int32_t)m0;
        a.wmaps = wmaps ? (w_host ? d_w : (unsigned long long *)wmaps + (size_t)m0 * nb) : nullptr;
        a.counts = counts ? (c_host ? d_c : counts + (size_t)m0 * nb) : nullptr;
        if (a.wmaps)
            HIP_TRY(hipMemsetAsync(a.wmaps, 0, sizeof(int64_t) * nb * c, st));
        if (a.counts)
            HIP_TRY(hipMemsetAsync(a.counts, 0, sizeof(uint32_t) * nb * c, st));
        const int32_t f0 = h_first[m0], f1 = h_first[m0 + c];
        if (f1 > f0) {
            a.items = d_items + f0;
            hipLaunchKernelGGL(wmaps_kernel, dim3((unsigned)n_tiles, (unsigned)(f1 - f0)), dim3(kBlock), 0, st, a);
            HIP_TRY(hipGetLastError());
        }
        // this chunk's maps, copied before the next chunk reuses the scratch
        if (w_host)
            HIP_TRY(hipMemcpyAsync(wmaps + (size_t)m0 * nb, d_w, sizeof(int64_t) * nb * c, hipMemcpyDefault, st));
        if (c_host)
            HIP_TRY(hipMemcpyAsync(counts + (size_t)m0 * nb, d_c, sizeof(uint32_t) * nb * c, hipMemcpyDefault, st));
    }
    if (scale_exp)
        HIP_TRY(hipMemcpyAsync(scale_exp, d_scale, sizeof(int32_t) * (size_t)n_maps, hipMemcpyDefault, st));
    if (i_host)
        HIP_TRY(hipMemcpyAsync(item, d_item, sizeof(rox_wmap_item) * (size_t)n_items, hipMemcpyDefault, st));
    if (w_host || c_host || e_host || i_host)
        HIP_TRY(hipStreamSynchronize(st));
    return 0;
}
