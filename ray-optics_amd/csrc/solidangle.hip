// solidangle.hip -- rox_projected_solid_angle: the signed area a finished num x num pupil grid
// covers in the plane of the direction cosines (L, M) its rays arrive with (include/roxtrace.h
// states the arithmetic), the quantity radiometric relative illumination is a ratio of.
//
// A wave owns 64 consecutive columns j of a chunk of rows i: 63 cells per row, strips step by 63.
// It walks its rows with the previous row's L, M, weight and OK bit in registers and takes the
// j + 1 neighbour with a cross-lane shuffle, so that every value is loaded once per strip (the
// chunk's first row once more), in coalesced row pieces of 512 bytes, and no LDS is used in the
// walk.  A ray belongs to the one wave that has it in lanes 0 .. 62 of the rows before its
// chunk's last (the grid's last column and last row go to the waves that reach them); a cell to
// the one wave that has its corner a.  Each wave writes one partial record; the finishing kernel
// merges an item's partial records in a fixed order (rox::block_merge).  No floating-point atomics.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rox_packets.hpp"

namespace {

constexpr char kHipWhere[] = "rox_projected_solid_angle: ";

// the workgroup of the packet entries; the rays are dealt in strips, not in its tiles
constexpr int kBlock = rox::PacketTile<1>::kBlock, kWaves = rox::PacketTile<1>::kWaves;
constexpr int kStrip = 63;                      // cells per wave and row
// Device scratch of one launch (partial records, records and cells bound for host memory): a call
// that needs more per launch runs as consecutive launches over fewer items.
constexpr size_t kSaScratchBytes = size_t(32) << 20;

struct ItemIn {
    const double *l, *m;                        // the rows of L and of M
    const uint8_t *status;
    const double *w;                            // the row of weights or nullptr
};

// the floating-point part of a partial record
struct Acc {
    double a_full, a_tri, a_abs, aw_full, aw_tri, l_sum, m_sum;
    double l_min, l_max, m_min, m_max, r2;
};

struct Part {
    Acc a;
    uint32_t n_ok, n_cells[5];
};                                              // 120 bytes

struct SaArgs {
    const ItemIn *items;                        // the launch's items
    int32_t num, rows;                          // rows: rows of cells per chunk
    int32_t n_strips, n_units;                  // per item: n_units = n_strips * chunks
    Part *part;                                 // [items][n_units] or nullptr
    double *cells;                              // [items][num-1][num-1] or nullptr
};

// Rows of cells a wave walks: a function of num alone, so that an item's partial records and
// their merge do not depend on the call it is part of.  Small grids take short chunks (64^2 x 9
// items still makes 72 waves); the first row of a chunk is read twice, 1/rows of the traffic.
inline int chunk_rows(int num) { return num <= 256 ? 8 : num <= 2048 ? 32 : 128; }

__device__ __forceinline__ Acc acc_empty()
{
    const double inf = __builtin_inf();
    return Acc{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, inf, -inf, inf, -inf, -inf};
}

// a <- a merged with b, a's records first
__device__ __forceinline__ void acc_merge(Acc &a, const Acc &b)
{
    a.a_full = a.a_full + b.a_full; a.a_tri = a.a_tri + b.a_tri; a.a_abs = a.a_abs + b.a_abs;
    a.aw_full = a.aw_full + b.aw_full; a.aw_tri = a.aw_tri + b.aw_tri;
    a.l_sum = a.l_sum + b.l_sum; a.m_sum = a.m_sum + b.m_sum;
    a.l_min = fmin(a.l_min, b.l_min); a.l_max = fmax(a.l_max, b.l_max);
    a.m_min = fmin(a.m_min, b.m_min); a.m_max = fmax(a.m_max, b.m_max);
    a.r2 = fmax(a.r2, b.r2);
}

__global__ __launch_bounds__(kBlock) void solid_angle_kernel(const SaArgs a)
{
    const int lane = threadIdx.x & 63;
    const int unit = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (unit >= a.n_units)
        return;                                 // (whole waves: no barrier follows)
    const ItemIn it = a.items[blockIdx.y];
    const int num = a.num;
    const int strip = unit % a.n_strips, chunk = unit / a.n_strips;
    const int j = strip * kStrip + lane;
    const int i0 = chunk * a.rows;
    const int i1 = min(i0 + a.rows, num - 1);   // the chunk's last row of rays, its cells' corners b and c
    const bool in_grid = j < num;
    const bool own_col = in_grid && (lane < kStrip || j == num - 1);
    const bool cell_col = lane < kStrip && j < num - 1;
    double *cells = a.cells ? a.cells + (size_t)blockIdx.y * (num - 1) * (num - 1) : nullptr;

    Acc t = acc_empty();
    uint32_t n_ok = 0, nc[5] = {0, 0, 0, 0, 0};
    // the previous row: this lane's ray (corner a) and its j + 1 neighbour (corner d)
    double la = 0.0, ma = 0.0, wa = 0.0, ld = 0.0, md = 0.0, wd = 0.0;
    bool oka = false, okd = false;
    // a row's status is loaded one row ahead: its L, M and weight loads depend on it
    int st_next = in_grid ? (int)it.status[(size_t)i0 * num + j] : -1;
    for (int i = i0; i <= i1; ++i) {
        const size_t r = (size_t)i * num + j;
        const bool okb = st_next == ROX_OK;
        st_next = in_grid && i < i1 ? (int)it.status[r + num] : -1;
        double lb = 0.0, mb = 0.0, wb = 0.0;
        if (okb) {
            lb = it.l[r];
            mb = it.m[r];
            wb = it.w ? it.w[r] : 1.0;
        }
        if (okb && own_col && (i < i0 + a.rows || i == num - 1)) {
            ++n_ok;
            t.l_sum = t.l_sum + lb; t.m_sum = t.m_sum + mb;
            t.l_min = fmin(t.l_min, lb); t.l_max = fmax(t.l_max, lb);
            t.m_min = fmin(t.m_min, mb); t.m_max = fmax(t.m_max, mb);
            t.r2 = fmax(t.r2, lb * lb + mb * mb);       // (-ffp-contract=off: no FMA)
        }
        const double lc = __shfl_down(lb, 1), mc = __shfl_down(mb, 1), wc = __shfl_down(wb, 1);
        const bool okc = __shfl_down((int)okb, 1) != 0;
        if (i > i0 && cell_col) {
            const int k = (int)oka + (int)okb + (int)okc + (int)okd;
            double area = 0.0;
            if (k == 4) {
                area = ((lc - la) * (md - mb) - (ld - lb) * (mc - ma)) * 0.5;
                const double w = ((wa + wb) + (wc + wd)) * 0.25;
                t.a_full = t.a_full + area;
                t.aw_full = t.aw_full + area * w;
                t.a_abs = t.a_abs + fabs(area);
            } else if (k == 3) {
                // (p, q, r): a, b, c, d in that order without the missing one
                const bool pa = oka, qb = oka && okb, rd = okd;
                const double lp = pa ? la : lb, mp = pa ? ma : mb, wp = pa ? wa : wb;
                const double lq = qb ? lb : lc, mq = qb ? mb : mc, wq = qb ? wb : wc;
                const double lr = rd ? ld : lc, mr = rd ? md : mc, wr = rd ? wd : wc;
                area = ((lq - lp) * (mr - mp) - (lr - lp) * (mq - mp)) * 0.5;
                const double w = ((wp + wq) + wr) / 3.0;
                t.a_tri = t.a_tri + area;
                t.aw_tri = t.aw_tri + area * w;
                t.a_abs = t.a_abs + fabs(area);
            }
            ++nc[k];
            if (cells)
                cells[(size_t)(i - 1) * (num - 1) + j] = area;
        }
        la = lb; ma = mb; wa = wb; oka = okb;
        ld = lc; md = mc; wd = wc; okd = okc;
    }
    if (!a.part)
        return;
    // the wave's record by a fixed butterfly
    Part p{t, n_ok, {nc[0], nc[1], nc[2], nc[3], nc[4]}};
    rox::wave_merge(p, [](Part &m, const Part &b) {
        acc_merge(m.a, b.a);
        m.n_ok += b.n_ok;
        for (int k = 0; k < 5; ++k)
            m.n_cells[k] += b.n_cells[k];
    });
    if (lane == 0)
        a.part[(size_t)blockIdx.y * a.n_units + unit] = p;
}

// what an item's partial records merge into, and a count as either holds it
struct Sum {
    Acc a;
    int64_t c[6];                               // n_ok, n_cells[0..4]
};

__device__ __forceinline__ int64_t count_of(const Sum &b, int s) { return b.c[s]; }
__device__ __forceinline__ int64_t count_of(const Part &q, int s)
{
    return (int64_t)(s == 0 ? q.n_ok : q.n_cells[s - 1]);
}

// item[i] from part[i][u], u = 0 .. n_units - 1, in the order of rox::block_merge
__global__ __launch_bounds__(kBlock) void solid_angle_finish(const Part *__restrict__ part, int n_units,
                                                             rox_sa_item *__restrict__ item)
{
    __shared__ Sum lds[kBlock];
    const auto merge = [](Sum &m, const auto &b) {
        acc_merge(m.a, b.a);
        for (int s = 0; s < 6; ++s)
            m.c[s] += count_of(b, s);
    };
    const Sum sum = rox::block_merge<kBlock>(part + (size_t)blockIdx.x * n_units, n_units, 1,
                                             Sum{acc_empty(), {0, 0, 0, 0, 0, 0}}, merge, lds);
    if (threadIdx.x == 0) {
        const Acc m = sum.a;
        const double nan = __builtin_nan("");
        const bool any = sum.c[0] > 0;
        rox_sa_item f;
        f.n_ok = sum.c[0];
        for (int k = 0; k < 5; ++k)
            f.n_cells[k] = sum.c[k + 1];
        f.a_full = m.a_full; f.a_tri = m.a_tri; f.a_abs = m.a_abs;
        f.aw_full = m.aw_full; f.aw_tri = m.aw_tri;
        f.l_sum = m.l_sum; f.m_sum = m.m_sum;
        f.l_min = any ? m.l_min : nan; f.l_max = any ? m.l_max : nan;
        f.m_min = any ? m.m_min : nan; f.m_max = any ? m.m_max : nan;
        f.r2_max = any ? m.r2 : nan;
        item[blockIdx.x] = f;
    }
}

rox::PerStream<rox::Workspace> g_sa_ws;

}  // namespace

extern "C" int rox_projected_solid_angle(int32_t n_items, int32_t num, const rox_out *outs, int32_t dir_row,
                                         const double *weight, int64_t weight_stride, rox_sa_item *item,
                                         double *cells, void *stream)
{
    static const char kE[] = "rox_projected_solid_angle";
    // every argument check comes before anything touches a device
    if (!outs)
        return rox::host_fail(ROX_E_ARG, "%s: null outs", kE);
    ROX_TRY(rox::check_range(kE, "n_items", n_items, 1, ROX_MAX_FOCUS_ITEMS));
    ROX_TRY(rox::check_range(kE, "num", num, 2, ROX_MAX_SA_NUM));
    if (dir_row < 0)
        return rox::host_fail(ROX_E_ARG, "%s: dir_row %d < 0", kE, dir_row);
    if (!item && !cells)
        return rox::host_fail(ROX_E_ARG, "%s: null item and cells", kE);
    const int64_t n_rays = (int64_t)num * num;
    if (weight && weight_stride < n_rays)
        return rox::host_fail(ROX_E_ARG, "%s: weight_stride %lld < num*num %lld", kE, (long long)weight_stride,
                              (long long)n_rays);
    for (int32_t i = 0; i < n_items; ++i)
        ROX_TRY(rox::check_packet_item(kE, i, outs[i], n_rays, false));

    hipStream_t st = (hipStream_t)stream;
    rox::Turn<> ws;
    ROX_TRY(ws.take(g_sa_ws, st, kHipWhere));

    const bool cells_host = cells && !rox::is_device(cells);
    const bool host_dst = (item && !rox::is_device(item)) || cells_host;
    const int rows = chunk_rows(num);
    const int n_strips = (num - 1 + kStrip - 1) / kStrip, n_chunks = (num - 1 + rows - 1) / rows;
    const int n_units = n_strips * n_chunks;
    const size_t cells_item = sizeof(double) * (size_t)(num - 1) * (num - 1);
    const size_t b_part = item ? rox::up256(sizeof(Part) * (size_t)n_units) : 0;
    const size_t per_item = b_part + (item ? 256 : 0) + (cells_host ? rox::up256(cells_item) : 0) + 256;
    const int64_t chunk = rox::chunk_for(n_items, per_item, kSaScratchBytes);

    const size_t b_tab = sizeof(ItemIn) * (size_t)n_items;
    ItemIn *d_tab;
    Part *d_part;
    rox_sa_item *d_item;
    double *d_cells;
    rox::Layout L;
    L.add(d_tab, rox::up256(b_tab));
    L.add(d_part, item ? rox::up256(sizeof(Part) * (size_t)n_units * chunk) : 0);
    L.add(d_item, item ? rox::up256(sizeof(rox_sa_item) * (size_t)chunk) : 0);
    L.add(d_cells, cells_host ? rox::up256(cells_item * chunk) : 0);
    ItemIn *h;
    ROX_TRY(ws.carve(L, b_tab, &h));
    for (int32_t i = 0; i < n_items; ++i) {
        const double *seg = outs[i].seg + (size_t)dir_row * outs[i].ld;
        h[i] = ItemIn{seg, seg + outs[i].ld, outs[i].status, weight ? weight + (size_t)i * weight_stride : nullptr};
    }
    ROX_TRY(ws.upload(d_tab, b_tab));

    SaArgs a{};
    a.num = num; a.rows = rows; a.n_strips = n_strips; a.n_units = n_units;
    a.part = item ? d_part : nullptr;
    const unsigned n_blocks = (unsigned)((n_units + kWaves - 1) / kWaves);
    for (int64_t i0 = 0; i0 < n_items; i0 += chunk) {
        const int64_t c = std::min<int64_t>(chunk, n_items - i0);
        a.items = d_tab + i0;
        a.cells = cells ? (cells_host ? d_cells : cells + (size_t)i0 * (num - 1) * (num - 1)) : nullptr;
        hipLaunchKernelGGL(solid_angle_kernel, dim3(n_blocks, (unsigned)c), dim3(kBlock), 0, st, a);
        if (item)
            hipLaunchKernelGGL(solid_angle_finish, dim3((unsigned)c), dim3(kBlock), 0, st, (const Part *)d_part,
                               n_units, d_item);
        HIP_TRY(hipGetLastError());
        // this chunk's results, copied before the next chunk reuses the scratch
        if (item)
            HIP_TRY(hipMemcpyAsync(item + i0, d_item, sizeof(rox_sa_item) * (size_t)c, hipMemcpyDefault, st));
        if (cells_host)
            HIP_TRY(hipMemcpyAsync(cells + (size_t)i0 * (num - 1) * (num - 1), d_cells, cells_item * c,
                                   hipMemcpyDefault, st));
    }
    if (host_dst)
        HIP_TRY(hipStreamSynchronize(st));
    return 0;
}
