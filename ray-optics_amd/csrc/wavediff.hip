// wavediff.hip -- rox_wave_differentials: the first-order change of every OK ray's optical path
// under rigid-body, curvature, power, irregularity and index perturbations of the selected
// interfaces (Hopkins & Tiziani's wavefront differentials), from the ROX_OUT_FULL packets of
// finished launches, and the covariance sums of those per-ray columns (include/roxtrace.h states
// the arithmetic in operation order; every step of a column is one IEEE double operation, no FMA).
//
// Passes (each a fixed order, no floating-point atomics; identical calls give identical bits):
//   wd_walk    the tile walk of the packet entries (rox::PacketTile): a workgroup owns kTile rays
//              of one item and walks the slots with the previous direction of each ray in registers,
//              as fresnel.hip does; of a slot's 10 rows it reads d, and p and dst where the slot is
//              selected, of OK rays only.  It writes the columns [n_cols][ld] along the ray axis,
//              NaN for a ray that is not counted, and counts n, n_bad and the lowest counted ray by
//              integer atomics (exact, whatever their order).
//   wd_pivot   the pivot ray's columns, once the walk that holds it has run.
//   wd_gram    zernike.hip's rank-n update: a workgroup takes a chunk of rays of one item in 32-ray
//              LDS tiles of [col - pivot | 1] (rows of rays that are not counted are zero) and
//              accumulates upper 16x16 tiles of the Gram matrix with v_mfma_f64_16x16x4_f64; the
//              column "1" gives the sums.  The columns go in panels of 96: blockIdx.z is a pair of
//              panels, so that the accumulators of one workgroup hold whatever n_cols is.  One
//              partial record per (item, chunk).
//   wd_sum     adds the chunks' records in chunk order onto a running record: the same sum however
//              the chunks are grouped into launches.
//   wd_finish  both triangles of gram, the sums and the item record.
// The chunking of an item's rays is a function of its ray count alone, so splitting a job into
// launches (the scratch bound) does not change a bit.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "rox_math.hpp"
#include "rox_packets.hpp"
#include "rox_system.hpp"

namespace {

using rox::ctbli;
using rox::ctblp;
using rox::kRtDoubles;

constexpr char kHipWhere[] = "rox_wave_differentials: ";

typedef double d4 __attribute__((ext_vector_type(4)));

using Tile = rox::PacketTile<2>;                // rays per thread of the walk
constexpr int kBlock = Tile::kBlock, kRays = Tile::kRays;
constexpr int kSlotCols = ROX_WD_SLOT_COLS;     // columns of a selected slot
constexpr int kGT = 32;                         // rays per LDS tile of the Gram pass (8 MFMA k-steps of 4)
constexpr int kGroups = kBlock / kGT;           // 8 thread groups of one half-wave each
constexpr int kPanelTiles = 6;                  // 16-column tiles per panel
constexpr int kPanel = 16 * kPanelTiles;        // 96 columns
constexpr int kLdm = 2 * kPanel + 1;            // an odd row pitch (zernike.hip)
constexpr int kMaxTilesPerWave = kPanelTiles * kPanelTiles / 4;     // 36 tiles of two panels over 4 waves
// rays per workgroup before another chunk is added, and the most chunks of an item: a workgroup
// works through its chunk one 32-ray tile after the other (load, barrier, MFMA, barrier), so the
// chunks are what fills the device (8192 and 64, zernike.hip's figures, left 27 workgroups for
// 9 items of 64^2 rays: 1.2 ms)
constexpr int kRaysPerChunk = 512;
constexpr int kMaxChunks = 256;
// Device scratch of one launch, or what one item needs where that is more; within it the columns
// of a range of rays and the partial records of a group of chunks take kPartBytes each
constexpr size_t kWdScratchBytes = size_t(32) << 20;
constexpr size_t kPartBytes = size_t(8) << 20;

struct ItemIn {
    const double *seg;
    const uint8_t *status;
    const double *aux;                          // the item's first aux row, or nullptr
    int64_t ld;
    int32_t wvl;
    int32_t pad;
};

struct WalkArgs {
    const ItemIn *items;                        // the launch's items
    const double *rt;                           // [n_ifcs][kRtDoubles]
    const double *kq;                           // [n_ifcs] (ec*cv)*cv
    const double *n_table;                      // [n_wvls][n_ifcs]
    const int32_t *slot_ifc;                    // [n_seg] interface of slot k
    const int32_t *sel_of;                      // [n_seg] the slot's place in the selection, or -1
    const int32_t *conic;                       // [n_ifcs] 1: column 6 from q
    int32_t n_ifcs, n_seg, n_aux, n_cols;
    int64_t ray0, ray1;                         // this launch's rays
    int64_t ld_aux;
    double *cols;                               // the launch's first item: [n_cols][ld_cols], column 0 = ray col_ray0
    int64_t col_stride, ld_cols, col_ray0;      // (col_stride between items)
    unsigned long long *cnt;                    // the launch's first item: n, n_bad, the lowest counted ray
};

// the direction carried between frames exactly as fresnel.hip carries it: rox_packets.hpp
using rox::carry;
using rox::cross;
using rox::V3;

__device__ __forceinline__ bool finite(double v) { return fabs(v) <= DBL_MAX; }     // (NaN: not)

__global__ __launch_bounds__(kBlock) void wd_walk(const WalkArgs a)
{
    const ItemIn it = a.items[blockIdx.y];
    const int lane = threadIdx.x & 63;
    const int n_seg = a.n_seg;
    const ctbli slot_ifc = (ctbli)a.slot_ifc, sel_of = (ctbli)a.sel_of, conic = (ctbli)a.conic;
    const ctblp rt_of = (ctblp)a.rt, kq_of = (ctblp)a.kq;
    const ctblp ntab = (ctblp)a.n_table + (size_t)it.wvl * a.n_ifcs;
    const double nan = __builtin_nan("");
    const int64_t ld = a.ld_cols;
    double *const cols = a.cols ? a.cols + (size_t)blockIdx.y * a.col_stride : nullptr;

    int64_t r[kRays];
    bool in[kRays], ok[kRays], fin[kRays];
    V3 b4[kRays];
#pragma unroll
    for (int j = 0; j < kRays; ++j) {
        r[j] = Tile::ray(j, a.ray0);
        in[j] = r[j] < a.ray1;
        ok[j] = in[j] && it.status[r[j]] == ROX_OK;
        fin[j] = true;
        b4[j] = V3{0.0, 0.0, 0.0};
    }

    for (int c = 0; c < a.n_aux; ++c) {
#pragma unroll
        for (int j = 0; j < kRays; ++j) {
            const double v = ok[j] ? it.aux[(size_t)c * a.ld_aux + r[j]] : nan;
            fin[j] = fin[j] && (!ok[j] || finite(v));
            if (cols && in[j])
                cols[(size_t)c * ld + (r[j] - a.col_ray0)] = v;
        }
    }

    for (int k = 0; k < n_seg; ++k) {
        const double *rec = it.seg + (size_t)k * ROX_SEG_DOUBLES * it.ld;
        const int s = slot_ifc[k], sel = sel_of[k];
        V3 p[kRays], d[kRays];
        double dst[kRays];
#pragma unroll
        for (int j = 0; j < kRays; ++j) {
            p[j] = d[j] = V3{0.0, 0.0, 0.0};
            dst[j] = 0.0;
            if (ok[j]) {
                d[j] = V3{rec[3 * it.ld + r[j]], rec[4 * it.ld + r[j]], rec[5 * it.ld + r[j]]};
                if (sel >= 0) {
                    p[j] = V3{rec[r[j]], rec[it.ld + r[j]], rec[2 * it.ld + r[j]]};
                    dst[j] = rec[6 * it.ld + r[j]];
                }
            }
        }

        // the previous direction into this slot's frame: through every interface in between
        if (k >= 1)
            for (int i = slot_ifc[k - 1]; i < s; ++i) {
                const ctblp rt = rt_of + (size_t)i * kRtDoubles;
                const bool c_order = rt[9] != 0.0;
#pragma unroll
                for (int j = 0; j < kRays; ++j)
                    b4[j] = carry(rt, c_order, b4[j]);
            }

        if (sel >= 0) {
            // the two unsigned indices: the same for every ray of the workgroup
            const bool last = k == n_seg - 1;
            const double n1 = fabs(k == 0 ? ntab[0] : ntab[s - 1]);
            const double n2 = last ? 0.0 : fabs(k == 0 ? ntab[0] : ntab[s]);
            const double kq = kq_of[s];
            const bool use_q = conic[s] != 0;
            const size_t cb = (size_t)(a.n_aux + kSlotCols * sel);
#pragma unroll
            for (int j = 0; j < kRays; ++j) {
                const V3 bb = k == 0 ? d[j] : b4[j];
                const V3 g{n1 * bb.x - n2 * d[j].x, n1 * bb.y - n2 * d[j].y, n1 * bb.z - n2 * d[j].z};
                const V3 m = cross(p[j], g);
                const double x = p[j].x, y = p[j].y;
                const double r2 = x * x + y * y;
                const double rad = 1.0 - kq * r2;
                double cvf = r2 / 2.0;
                if (use_q && rad > 0.0) {
                    const double q = sqrt(rad);
                    cvf = r2 / (q * (1.0 + q));
                }
                double v[kSlotCols];
                v[0] = g.x; v[1] = g.y; v[2] = g.z;
                v[3] = m.x; v[4] = m.y; v[5] = m.z;
                v[6] = g.z * cvf;
                v[7] = g.z * r2;
                v[8] = g.z * (x * x - y * y);
                v[9] = g.z * ((x + x) * y);
                v[10] = last ? 0.0 : dst[j];
                bool f = true;
#pragma unroll
                for (int c = 0; c < kSlotCols; ++c)
                    f = f && finite(v[c]);
                fin[j] = fin[j] && (!ok[j] || f);
                if (cols && in[j]) {
                    double *o = cols + cb * ld + (r[j] - a.col_ray0);
#pragma unroll
                    for (int c = 0; c < kSlotCols; ++c)
                        o[(size_t)c * ld] = ok[j] ? v[c] : nan;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kRays; ++j)
            b4[j] = d[j];
    }

    // an OK ray with a value that is not finite is not counted: its columns are NaN as well
    unsigned long long *cnt = a.cnt + (size_t)blockIdx.y * 3;
#pragma unroll
    for (int j = 0; j < kRays; ++j) {
        const bool bad = ok[j] && !fin[j], counted = ok[j] && fin[j];
        if (cols && bad)
            for (int c = 0; c < a.n_cols; ++c)
                cols[(size_t)c * ld + (r[j] - a.col_ray0)] = nan;
        const unsigned long long mc = __ballot(counted), mb = __ballot(bad);
        if (lane == 0) {
            if (mc) {
                atomicAdd(cnt, (unsigned long long)__popcll(mc));
                atomicMin(cnt + 2, (unsigned long long)(r[j] + (__ffsll((long long)mc) - 1)));
            }
            if (mb)
                atomicAdd(cnt + 1, (unsigned long long)__popcll(mb));
        }
    }
}

// block (0, item): pivot[c] = column c of the item's lowest counted ray, where this range holds it
__global__ __launch_bounds__(kBlock) void wd_pivot(const unsigned long long *__restrict__ cnt,
                                                   const double *__restrict__ cols, int64_t col_stride, int64_t ld,
                                                   int64_t col_ray0, int64_t ray0, int64_t ray1, int n_cols,
                                                   double *__restrict__ pivot)
{
    const unsigned long long pr = cnt[(size_t)blockIdx.y * 3 + 2];
    if (pr < (unsigned long long)ray0 || pr >= (unsigned long long)ray1)
        return;
    const double *c = cols + (size_t)blockIdx.y * col_stride + ((int64_t)pr - col_ray0);
    for (int e = threadIdx.x; e < n_cols; e += kBlock)
        pivot[(size_t)blockIdx.y * n_cols + e] = c[(size_t)e * ld];
}

struct GramArgs {
    const double *cols;                         // the launch's first item, column 0 = ray col_ray0
    int64_t col_stride, ld, col_ray0;
    const double *pivot;                        // the launch's first item: [n_cols]
    int32_t n_cols, NT, CP;                     // columns; 16-column tiles of [cols | 1]; 16*NT
    int64_t n_rays, span;                       // rays per chunk, a multiple of kGT
    int32_t ch0;                                // the launch's first chunk
    double *part;                               // [items][gridDim.x][CP*CP]
};

__global__ __launch_bounds__(kBlock) void wd_gram(const GramArgs a)
{
    __shared__ double M[kGT * kLdm];
    const int li = blockIdx.y;
    const int npan = (a.NT + kPanelTiles - 1) / kPanelTiles;
    // blockIdx.z -> the pair of panels (pa, pb), pa <= pb, row-major
    int pa = 0, rem = blockIdx.z;
    while (rem >= npan - pa) {
        rem -= npan - pa;
        ++pa;
    }
    const int pb = pa + rem;
    const bool diag = pa == pb;
    const int nta = min(kPanelTiles, a.NT - kPanelTiles * pa), ntb = min(kPanelTiles, a.NT - kPanelTiles * pb);
    const int ntiles = diag ? nta * (nta + 1) / 2 : nta * ntb;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ray_l = tid & (kGT - 1), grp = tid >> 5;
    const int boff = diag ? 0 : kPanel;         // panel b's first column in M

    d4 acc[kMaxTilesPerWave];
    int trow[kMaxTilesPerWave], tcol[kMaxTilesPerWave];     // tile i's row tile of panel a, column tile of panel b
#pragma unroll
    for (int i = 0; i < kMaxTilesPerWave; ++i) {
        acc[i] = d4{0., 0., 0., 0.};
        const int tix = wave + 4 * i;
        int rt = 0, ct = 0;
        if (tix < ntiles) {
            if (diag) {                         // (rt, ct), ct >= rt, row-major
                int q = tix;
                while (q >= nta - rt) {
                    q -= nta - rt;
                    ++rt;
                }
                ct = rt + q;
            } else {
                rt = tix / ntb;
                ct = tix - rt * ntb;
            }
        }
        trow[i] = rt;
        tcol[i] = ct;
    }

    const double *cols = a.cols + (size_t)li * a.col_stride;
    const double *piv = a.pivot + (size_t)li * a.n_cols;
    const int64_t rb = (int64_t)(a.ch0 + blockIdx.x) * a.span, re = min<int64_t>(a.n_rays, rb + a.span);
    const int na = 16 * nta, nb = 16 * ntb;

    for (int64_t t0 = rb; t0 < re; t0 += kGT) {
        const int64_t r = t0 + ray_l;
        const double *cr = cols + (r - a.col_ray0);
        const bool counted = r < re && finite(cr[0]);
        double *row = M + ray_l * kLdm;
        for (int j = grp; j < na; j += kGroups) {
            const int gc = kPanel * pa + j;
            row[j] = !counted ? 0.0 : gc < a.n_cols ? cr[(size_t)gc * a.ld] - piv[gc] : gc == a.n_cols ? 1.0 : 0.0;
        }
        if (!diag)
            for (int j = grp; j < nb; j += kGroups) {
                const int gc = kPanel * pb + j;
                row[kPanel + j] =
                    !counted ? 0.0 : gc < a.n_cols ? cr[(size_t)gc * a.ld] - piv[gc] : gc == a.n_cols ? 1.0 : 0.0;
            }
        __syncthreads();
        const int ar = lane >> 4, ac = lane & 15;
#pragma unroll
        for (int ks = 0; ks < kGT; ks += 4) {
            const double *mr = M + (ks + ar) * kLdm;
#pragma unroll
            for (int i = 0; i < kMaxTilesPerWave; ++i) {
                if (wave + 4 * i < ntiles)
                    acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(mr[16 * trow[i] + ac], mr[boff + 16 * tcol[i] + ac],
                                                                  acc[i], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    double *g = a.part + ((size_t)li * gridDim.x + blockIdx.x) * ((size_t)a.CP * a.CP);
    const int ar = lane >> 4, ac = lane & 15;
#pragma unroll
    for (int i = 0; i < kMaxTilesPerWave; ++i) {
        if (wave + 4 * i >= ntiles)
            continue;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int row = kPanel * pa + 16 * trow[i] + ar + 4 * q, col = kPanel * pb + 16 * tcol[i] + ac;
            g[(size_t)row * a.CP + col] = acc[i][q];
        }
    }
}

// acc[item] (0 when `first`) + the launch's chunks in order, over the upper 16x16 tiles
__global__ __launch_bounds__(kBlock) void wd_sum(const double *__restrict__ part, int n_ch, int CP, int first,
                                                 double *__restrict__ acc)
{
    const size_t rec = (size_t)CP * CP;
    const size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= rec || (int)(e % CP) / 16 < (int)(e / CP) / 16)
        return;
    const double *p = part + (size_t)blockIdx.y * n_ch * rec + e;
    double v = first ? 0.0 : acc[(size_t)blockIdx.y * rec + e];
    for (int c = 0; c < n_ch; ++c)
        v += p[(size_t)c * rec];
    acc[(size_t)blockIdx.y * rec + e] = v;
}

// gram (both triangles) and sums from the running record; the item record from the counters
__global__ __launch_bounds__(kBlock) void wd_finish(const double *__restrict__ acc, int CP, int n_cols,
                                                    const unsigned long long *__restrict__ cnt,
                                                    double *__restrict__ gram, double *__restrict__ sums,
                                                    rox_wd_item *__restrict__ item)
{
    const size_t li = blockIdx.y;
    const size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const double *A = acc ? acc + li * (size_t)CP * CP : nullptr;
    if (gram && e < (size_t)n_cols * n_cols) {
        const int i = (int)(e / n_cols), j = (int)(e % n_cols);
        gram[li * (size_t)n_cols * n_cols + e] = A[(size_t)min(i, j) * CP + max(i, j)];
    }
    if (sums && e < (size_t)n_cols)
        sums[li * n_cols + e] = A[e * CP + n_cols];
    if (item && e == 0) {
        const unsigned long long *c = cnt + li * 3;
        rox_wd_item f;
        f.n = (int64_t)c[0];
        f.n_bad = (int64_t)c[1];
        f.pivot_ray = c[0] ? (int64_t)c[2] : -1;
        item[li] = f;
    }
}

rox::PerStream<rox::Workspace> g_wd_ws;

}  // namespace

extern "C" int rox_wave_differentials(rox_system *sys, uint32_t trace_flags, int32_t n_items, const rox_out *outs,
                                      int64_t n_rays, const int32_t *wvl_idx, int32_t n_sel, const int32_t *sel_slot,
                                      int32_t n_aux, const double *aux, int64_t aux_stride, int64_t ld_aux,
                                      double *cols, int64_t ld_cols, rox_wd_item *item, double *pivot, double *sums,
                                      double *gram, void *stream)
{
    static const char kE[] = "rox_wave_differentials";
    // every argument check comes before anything touches a device
    ROX_TRY(rox::check_packet_call(kE, sys, outs, n_items));
    ROX_TRY(rox::check_packet_rays(kE, n_rays));
    if (!wvl_idx)
        return rox::host_fail(ROX_E_ARG, "%s: null wvl_idx", kE);
    if (!cols && !item && !gram)
        return rox::host_fail(ROX_E_ARG, "%s: null cols, item and gram", kE);
    if (gram && !(item && pivot && sums))
        return rox::host_fail(ROX_E_ARG, "%s: gram goes with item, pivot and sums", kE);
    if ((pivot || sums) && !item)
        return rox::host_fail(ROX_E_ARG, "%s: pivot and sums go with item", kE);
    if (sums && !pivot)
        return rox::host_fail(ROX_E_ARG, "%s: sums go with pivot", kE);
    ROX_TRY(rox::check_range(kE, "n_aux", n_aux, 0, ROX_MAX_WD_AUX));
    if (n_aux > 0 && !aux)
        return rox::host_fail(ROX_E_ARG, "%s: null aux with n_aux %d", kE, n_aux);
    if (n_aux > 0 && ld_aux < n_rays)
        return rox::host_fail(ROX_E_ARG, "%s: ld_aux %lld < n_rays %lld", kE, (long long)ld_aux, (long long)n_rays);
    if (cols && ld_cols < n_rays)
        return rox::host_fail(ROX_E_ARG, "%s: ld_cols %lld < n_rays %lld", kE, (long long)ld_cols, (long long)n_rays);
    for (int32_t i = 0; i < n_items; ++i) {
        ROX_TRY(rox::check_packet_item(kE, i, outs[i], n_rays, false));
        if (wvl_idx[i] < 0)
            return rox::host_fail(ROX_E_ARG, "%s: item %d: wvl_idx %d outside the index table", kE, i, wvl_idx[i]);
    }
    const rox::PacketSlots ps(sys, trace_flags);
    const int32_t n_ifcs = ps.n_ifcs, n_seg = ps.n_seg;
    for (int32_t i = 0; i < n_items; ++i)
        if (wvl_idx[i] >= sys->n_wvls)
            return rox::host_fail(ROX_E_ARG, "%s: item %d: wvl_idx %d outside the index table of %d wavelengths",
                                  kE, i, wvl_idx[i], sys->n_wvls);
    if (sel_slot ? (n_sel < 0 || n_sel > n_seg) : n_sel != n_seg)
        return rox::host_fail(ROX_E_ARG, "%s: n_sel %d %s %d slots", kE, n_sel,
                              sel_slot ? "outside [0, n_seg] of the" : "without sel_slot is not the", n_seg);
    for (int32_t j = 0; sel_slot && j < n_sel; ++j)
        if (sel_slot[j] < 0 || sel_slot[j] >= n_seg || (j && sel_slot[j] <= sel_slot[j - 1]))
            return rox::host_fail(ROX_E_ARG, "%s: sel_slot[%d] = %d is outside [0, %d) or does not increase", kE, j,
                                  sel_slot[j], n_seg);
    const int64_t n_cols64 = (int64_t)n_aux + (int64_t)kSlotCols * n_sel;
    if (n_cols64 < 1 || n_cols64 > ROX_MAX_WD_COLS)
        return rox::host_fail(ROX_E_ARG, "%s: n_cols = n_aux + %d*n_sel = %lld outside [1, %d]", kE, kSlotCols,
                              (long long)n_cols64, ROX_MAX_WD_COLS);
    const int n_cols = (int)n_cols64;

    hipStream_t st = (hipStream_t)stream;
    rox::Turn<> ws;
    ROX_TRY(ws.take(g_wd_ws, st, kHipWhere));

    const bool want_gram = sums || gram;
    const bool cols_dev = cols && rox::is_device(cols), cols_host = cols && !cols_dev;
    const bool host_dst = cols_host || (item && !rox::is_device(item)) || (pivot && !rox::is_device(pivot)) ||
                          (sums && !rox::is_device(sums)) || (gram && !rox::is_device(gram));
    // the chunks of an item's rays: a function of n_rays alone
    int64_t nch = std::max<int64_t>(1, std::min<int64_t>(kMaxChunks, (n_rays + kRaysPerChunk - 1) / kRaysPerChunk));
    const int64_t span = ((n_rays + nch - 1) / nch + kGT - 1) / kGT * kGT;
    nch = (n_rays + span - 1) / span;
    const int NT = (n_cols + 1 + 15) / 16, CP = 16 * NT;
    const int npan = (NT + kPanelTiles - 1) / kPanelTiles, npairs = npan * (npan + 1) / 2;
    const size_t rec = sizeof(double) * (size_t)CP * CP;
    // the walk runs over a range of chunks whose columns fit the scratch (all of them where the
    // columns go to the caller's device memory); the Gram pass over groups of chunks of a range
    const bool scratch_cols = !cols_dev && (cols_host || want_gram || pivot);
    const int64_t range_ch =
        scratch_cols ? std::max<int64_t>(1, std::min<int64_t>(nch, (int64_t)(kPartBytes / (sizeof(double) * n_cols * span))))
                     : nch;
    const int64_t range_rays = range_ch * span;
    const int64_t group_ch = std::max<int64_t>(1, std::min<int64_t>(range_ch, (int64_t)(kPartBytes / rec)));
    const size_t b_cols = scratch_cols ? rox::up256(sizeof(double) * n_cols * (size_t)range_rays) : 0;
    const size_t b_part = want_gram ? rox::up256(rec * group_ch) : 0;
    const size_t b_acc = want_gram ? rox::up256(rec) : 0;
    const size_t b_gram = gram ? rox::up256(sizeof(double) * (size_t)n_cols * n_cols) : 0;
    const size_t b_sums = sums ? rox::up256(sizeof(double) * n_cols) : 0;
    const int64_t chunk = rox::chunk_for(n_items, b_cols + b_part + b_acc + b_gram + b_sums + 256, kWdScratchBytes);

    // the tables, staged as one block: [items][rt][kq][counters][pivot][slot_ifc][sel_of][conic]
    const size_t o_rt = sizeof(ItemIn) * (size_t)n_items, o_kq = o_rt + sizeof(double) * kRtDoubles * n_ifcs;
    const size_t o_cn = o_kq + sizeof(double) * n_ifcs, o_pv = o_cn + sizeof(uint64_t) * 3 * n_items;
    const size_t o_si = o_pv + sizeof(double) * (size_t)n_cols * n_items, o_so = o_si + sizeof(int32_t) * n_seg;
    const size_t o_co = o_so + sizeof(int32_t) * n_seg, b_tab = o_co + sizeof(int32_t) * n_ifcs;
    char *d_tab;
    double *d_cols, *d_part, *d_acc, *d_gram, *d_sums;
    rox_wd_item *d_item;
    rox::Layout L;
    L.add(d_tab, rox::up256(b_tab));
    L.add(d_cols, b_cols * chunk);
    L.add(d_part, b_part * chunk);
    L.add(d_acc, b_acc * chunk);
    L.add(d_gram, b_gram * chunk);
    L.add(d_sums, b_sums * chunk);
    L.add(d_item, rox::up256(sizeof(rox_wd_item) * (size_t)chunk));
    char *h;
    ROX_TRY(ws.carve(L, b_tab, &h));
    for (int32_t i = 0; i < n_items; ++i) {
        ((ItemIn *)h)[i] = ItemIn{outs[i].seg, outs[i].status, n_aux > 0 ? aux + (size_t)i * aux_stride : nullptr,
                                  outs[i].ld, wvl_idx[i], 0};
        uint64_t *c = (uint64_t *)(h + o_cn) + 3 * (size_t)i;
        c[0] = c[1] = 0;
        c[2] = ~uint64_t(0);
        for (int e = 0; e < n_cols; ++e)
            ((double *)(h + o_pv))[(size_t)i * n_cols + e] = __builtin_nan("");
    }
    ps.stage_rt((double *)(h + o_rt));
    ps.stage_slot_ifc((int32_t *)(h + o_si));
    for (int32_t k = 0; k < n_seg; ++k)
        ((int32_t *)(h + o_so))[k] = sel_slot ? -1 : k;
    for (int32_t j = 0; sel_slot && j < n_sel; ++j)
        ((int32_t *)(h + o_so))[sel_slot[j]] = j;
    for (int32_t i = 0; i < n_ifcs; ++i) {
        const rox_surface &row = ps.rows[i];
        ((double *)(h + o_kq))[i] = (row.ec * row.cv) * row.cv;
        ((int32_t *)(h + o_co))[i] = row.profile == ROX_SPHERICAL || row.profile == ROX_CONIC ||
                                     row.profile == ROX_EVENPOLY || row.profile == ROX_RADIALPOLY;
    }
    ROX_TRY(ws.upload(d_tab, b_tab));
    unsigned long long *const d_cnt = (unsigned long long *)(d_tab + o_cn);
    double *const d_pivot = (double *)(d_tab + o_pv);

    WalkArgs a{};
    a.rt = (const double *)(d_tab + o_rt);
    a.kq = (const double *)(d_tab + o_kq);
    a.n_table = sys->d_ntab;
    a.slot_ifc = (const int32_t *)(d_tab + o_si);
    a.sel_of = (const int32_t *)(d_tab + o_so);
    a.conic = (const int32_t *)(d_tab + o_co);
    a.n_ifcs = n_ifcs; a.n_seg = n_seg; a.n_aux = n_aux; a.n_cols = n_cols;
    a.ld_aux = ld_aux;
    GramArgs ga{};
    ga.n_cols = n_cols; ga.NT = NT; ga.CP = CP;
    ga.n_rays = n_rays; ga.span = span;
    ga.part = d_part;
    for (int64_t i0 = 0; i0 < n_items; i0 += chunk) {
        const int64_t c = std::min<int64_t>(chunk, n_items - i0);
        a.items = (const ItemIn *)d_tab + i0;
        a.cnt = d_cnt + 3 * i0;
        for (int64_t c0 = 0; c0 < nch; c0 += range_ch) {
            const int64_t c1 = std::min<int64_t>(nch, c0 + range_ch);
            const int64_t first = c0 * span, end = std::min<int64_t>(n_rays, c1 * span), count = end - first;
            a.ray0 = first;
            a.ray1 = end;
            a.cols = scratch_cols ? d_cols : cols_dev ? cols + (size_t)i0 * n_cols * ld_cols : nullptr;
            a.ld_cols = scratch_cols ? range_rays : ld_cols;
            a.col_stride = (int64_t)n_cols * a.ld_cols;
            a.col_ray0 = scratch_cols ? first : 0;
            hipLaunchKernelGGL(wd_walk, dim3((unsigned)Tile::tiles(count), (unsigned)c), dim3(kBlock), 0, st, a);
            HIP_TRY(hipGetLastError());
            // this range's columns, copied before the next launch reuses the scratch
            if (cols_host)
                HIP_TRY(hipMemcpy2DAsync(cols + (size_t)i0 * n_cols * ld_cols + first, sizeof(double) * ld_cols,
                                         d_cols, sizeof(double) * range_rays, sizeof(double) * count,
                                         (size_t)c * n_cols, hipMemcpyDeviceToHost, st));
            if (!want_gram && !pivot)
                continue;
            hipLaunchKernelGGL(wd_pivot, dim3(1, (unsigned)c), dim3(kBlock), 0, st,
                               (const unsigned long long *)a.cnt, (const double *)a.cols, a.col_stride, a.ld_cols,
                               a.col_ray0, first, end, n_cols,
                               d_pivot + (size_t)i0 * n_cols);
            if (!want_gram)
                continue;
            ga.cols = a.cols; ga.col_stride = a.col_stride; ga.ld = a.ld_cols; ga.col_ray0 = a.col_ray0;
            ga.pivot = d_pivot + (size_t)i0 * n_cols;
            for (int64_t g0 = c0; g0 < c1; g0 += group_ch) {
                const int ng = (int)std::min<int64_t>(group_ch, c1 - g0);
                ga.ch0 = (int32_t)g0;
                hipLaunchKernelGGL(wd_gram, dim3((unsigned)ng, (unsigned)c, (unsigned)npairs), dim3(kBlock), 0, st, ga);
                hipLaunchKernelGGL(wd_sum, dim3((unsigned)(((size_t)CP * CP + kBlock - 1) / kBlock), (unsigned)c),
                                   dim3(kBlock), 0, st, (const double *)d_part, ng, CP, g0 == 0 ? 1 : 0, d_acc);
            }
            HIP_TRY(hipGetLastError());
        }
        if (item) {
            const size_t n_el = gram ? (size_t)n_cols * n_cols : (size_t)n_cols;
            hipLaunchKernelGGL(wd_finish, dim3((unsigned)((n_el + kBlock - 1) / kBlock), (unsigned)c), dim3(kBlock), 0,
                               st, want_gram ? (const double *)d_acc : nullptr, CP, n_cols,
                               (const unsigned long long *)a.cnt, gram ? d_gram : nullptr, sums ? d_sums : nullptr,
                               d_item);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(item + i0, d_item, sizeof(rox_wd_item) * (size_t)c, hipMemcpyDefault, st));
            if (pivot)
                HIP_TRY(hipMemcpyAsync(pivot + (size_t)i0 * n_cols, d_pivot + (size_t)i0 * n_cols,
                                       sizeof(double) * (size_t)n_cols * c, hipMemcpyDefault, st));
            if (sums)
                HIP_TRY(hipMemcpyAsync(sums + (size_t)i0 * n_cols, d_sums, sizeof(double) * (size_t)n_cols * c,
                                       hipMemcpyDefault, st));
            if (gram)
                HIP_TRY(hipMemcpyAsync(gram + (size_t)i0 * n_cols * n_cols, d_gram,
                                       sizeof(double) * (size_t)n_cols * n_cols * c, hipMemcpyDefault, st));
        }
    }
    if (host_dst)
        HIP_TRY(hipStreamSynchronize(st));
    return 0;
}
