// fresnel.hip -- rox_surface_transmission: Fresnel transmission and polarization ray tracing over
// the ROX_OUT_FULL packets of finished launches (include/roxtrace.h states the arithmetic in
// operation order; every step is one IEEE double operation, no FMA, so NumPy float64 restates a
// ray's rows bit for bit).
//
// A workgroup owns kTile consecutive rays of one item, kRays per thread, and walks the slots in
// order with the previous direction, the two carried field vectors and the flux factor of each
// ray in registers: of a record's 10 rows it reads d and nrml once each, coalesced along the ray
// axis, and never p or dst.  A slot of a ray is read only where the ray's status is ROX_OK.  What
// is the same for every ray of the workgroup -- the slot's interface, its model, its two indices,
// its coating values, the rt of the interfaces in between -- is read through the constant address
// space at wave-uniform addresses: scalar loads into SGPRs (the kernel's only vector loads are
// the status byte and the twelve packet reads of a slot).  Each wave writes one partial record per slot and one for the item; the
// finishing kernel merges them in a fixed order.  No floating-point atomics.  (Shared with
// footprint.hip: rox_packets.hpp.)
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rox_device.hpp"
#include "rox_packets.hpp"
#include "rox_system.hpp"

namespace {

using rox::ctbli;
using rox::ctblp;
using rox::kRtDoubles;

constexpr char kHipWhere[] = "rox_surface_transmission: ";

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kRays = 2;                        // rays per thread: 107 VGPRs, no scratch, 4 waves per SIMD
constexpr int kTile = kBlock * kRays;           // rays per workgroup
// Device scratch of one launch (partial records, records, rows bound for host memory): a call that
// needs more per launch runs as consecutive launches over fewer items and, for the rows, fewer
// rays.  One item's partial records are not split: an item whose records exceed the cap (more than
// 4.8 M rays at 13 slots) runs alone with the scratch it needs, sizeof(Part) per wave and slot.
constexpr size_t kTxScratchBytes = size_t(32) << 20;

// what an interface does to the field, decided on the host from its row and its coating
enum Model : int32_t {
    kIdeal = 0,                                 // carried through the bend, nothing lost
    kBare = 1,                                  // Fresnel (ideal when n1 == n2)
    kMirror = 2,                                // ts = -1
    kFixed = 3,                                 // given power coefficients
    kFixedMirror = 4,
};

struct ItemIn {
    const double *seg;
    const uint8_t *status;
    int64_t ld;
    int32_t wvl;
    int32_t pad;
};

// a partial record: v[0] the count, v[1..3] and v[6] sums, v[4] a minimum, v[5] and v[7] minima
// (a slot) or maxima (the item)
//   slot: n, sum Ts, sum Tp, sum (Ts + Tp)/2, min Ts, min Tp, sum ci, min ci
//   item: n, sum T, sum T1, sum T2, min T, max T, sum D, max D
struct Part {
    double v[8];
};

struct TxArgs {
    const ItemIn *items;                        // the chunk's items
    const double *rt;                           // [n_ifcs][kRtDoubles]
    const int32_t *slot_ifc;                    // [n_seg] interface of slot k
    const int32_t *model;                       // [n_ifcs] Model
    const double *coat;                         // [n_ifcs][2] (Ts, Tp) of kFixed / kFixedMirror
    const double *n_table;                      // [n_wvls][n_ifcs]
    int32_t n_ifcs, n_seg;
    int64_t n_rays;
    int64_t ray0;                               // first ray of this launch (a multiple of kTile)
    int32_t n_rows;                             // 4 or 10
    int32_t n_waves;                            // per item, over all of its rays
    double *rows;                               // [items][n_rows][ld_rows], column 0 = ray row_ray0; or nullptr
    int64_t ld_rows, row_ray0;
    Part *part;                                 // [items][n_waves][n_seg + 1] or nullptr
};

struct V3 {
    double x, y, z;
};

__device__ __forceinline__ double dot(const V3 &a, const V3 &b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(const V3 &a, const V3 &b)
{
    return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ V3 over(const V3 &a, double s) { return V3{a.x / s, a.y / s, a.z / s}; }

// rt . v, the columns summed in the row's rt_order, unfused
__device__ __forceinline__ V3 carry(ctblp rt, bool c_order, const V3 &v)
{
    if (c_order)
        return V3{(rt[1] * v.y + rt[0] * v.x) + rt[2] * v.z, (rt[4] * v.y + rt[3] * v.x) + rt[5] * v.z,
                  (rt[7] * v.y + rt[6] * v.x) + rt[8] * v.z};
    return V3{(rt[0] * v.x + rt[1] * v.y) + rt[2] * v.z, (rt[3] * v.x + rt[4] * v.y) + rt[5] * v.z,
              (rt[6] * v.x + rt[7] * v.y) + rt[8] * v.z};
}

// E <- (ts*(s . E))*s + (tp*(p_in . E))*p_out
__device__ __forceinline__ V3 through(const V3 &E, const V3 &s, const V3 &pi, const V3 &po, double ts, double tp)
{
    const double a = ts * dot(s, E), b = tp * dot(pi, E);
    return V3{a * s.x + b * po.x, a * s.y + b * po.y, a * s.z + b * po.z};
}

__device__ __forceinline__ Part part_empty()
{
    const double inf = __builtin_inf();
    return Part{{0.0, 0.0, 0.0, 0.0, inf, inf, 0.0, inf}};
}

// a <- a merged with b, a's rays first; kItem: v[5] and v[7] are maxima
template <bool kItem>
__device__ __forceinline__ void part_merge(Part &a, const Part &b)
{
    a.v[0] = a.v[0] + b.v[0];
    a.v[1] = a.v[1] + b.v[1];
    a.v[2] = a.v[2] + b.v[2];
    a.v[3] = a.v[3] + b.v[3];
    a.v[4] = fmin(a.v[4], b.v[4]);
    a.v[5] = kItem ? fmax(a.v[5], b.v[5]) : fmin(a.v[5], b.v[5]);
    a.v[6] = a.v[6] + b.v[6];
    a.v[7] = kItem ? fmax(a.v[7], b.v[7]) : fmin(a.v[7], b.v[7]);
}

template <bool kItem>
__device__ __forceinline__ Part wave_merge(Part t)
{
    for (int o = 32; o > 0; o >>= 1) {
        Part b;
#pragma unroll
        for (int i = 0; i < 8; ++i)
            b.v[i] = __shfl_xor(t.v[i], o);
        part_merge<kItem>(t, b);
    }
    return t;
}

__global__ __launch_bounds__(kBlock) void fresnel_kernel(const TxArgs a)
{
    const ItemIn it = a.items[blockIdx.y];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n_seg = a.n_seg;
    // the tables through the constant address space (rox_device.hpp): a wave-uniform address there is
    // a scalar load into SGPRs, and the stores of the partial records do not order it
    const ctbli slot_ifc = (ctbli)a.slot_ifc, model_of = (ctbli)a.model;
    const ctblp rt_of = (ctblp)a.rt, coat = (ctblp)a.coat;
    const ctblp ntab = (ctblp)a.n_table + (size_t)it.wvl * a.n_ifcs;
    const double nan = __builtin_nan("");

    int64_t r[kRays];
    bool ok[kRays];
    V3 b4[kRays], E1[kRays], E2[kRays];
    double q[kRays];
#pragma unroll
    for (int j = 0; j < kRays; ++j) {
        r[j] = a.ray0 + (int64_t)blockIdx.x * kTile + j * kBlock + threadIdx.x;
        ok[j] = r[j] < a.n_rays && it.status[r[j]] == ROX_OK;
        b4[j] = E1[j] = E2[j] = V3{0.0, 0.0, 0.0};
        q[j] = 1.0;
    }
    const size_t wave_of_item = (size_t)(a.ray0 / kTile + blockIdx.x) * kWaves + wave;
    Part *out = a.part ? a.part + ((size_t)blockIdx.y * a.n_waves + wave_of_item) * (n_seg + 1) : nullptr;

    for (int k = 0; k < n_seg; ++k) {
        const double *rec = it.seg + (size_t)k * ROX_SEG_DOUBLES * it.ld;
        V3 d[kRays], N[kRays];
#pragma unroll
        for (int j = 0; j < kRays; ++j) {
            d[j] = N[j] = V3{0.0, 0.0, 0.0};
            if (ok[j]) {
                d[j] = V3{rec[3 * it.ld + r[j]], rec[4 * it.ld + r[j]], rec[5 * it.ld + r[j]]};
                N[j] = V3{rec[7 * it.ld + r[j]], rec[8 * it.ld + r[j]], rec[9 * it.ld + r[j]]};
            }
        }

        // the state into this slot's frame: through every interface in between
        const int s = slot_ifc[k];
        if (k >= 1)
            for (int i = slot_ifc[k - 1]; i < s; ++i) {
                const ctblp rt = rt_of + (size_t)i * kRtDoubles;
                const bool c_order = rt[9] != 0.0;
#pragma unroll
                for (int j = 0; j < kRays; ++j) {
                    b4[j] = carry(rt, c_order, b4[j]);
                    E1[j] = carry(rt, c_order, E1[j]);
                    E2[j] = carry(rt, c_order, E2[j]);
                }
            }

        // the slot's model: the same for every ray of the workgroup
        const bool inner = k > 0 && k < n_seg - 1;
        int model = kIdeal;
        double n1 = 1.0, n2 = 1.0, cTs = 1.0, cTp = 1.0, cts = 1.0, ctp = 1.0;
        if (inner) {
            model = model_of[s];
            n1 = ntab[s - 1];
            n2 = ntab[s];
            if (model == kBare && n1 == n2)
                model = kIdeal;
            if (model == kFixed || model == kFixedMirror) {
                cTs = coat[2 * s];
                cTp = coat[2 * s + 1];
                cts = sqrt(cTs);
                ctp = sqrt(cTp);
            }
            if (model == kMirror || model == kFixedMirror)
                cts = -cts;
        }

        Part t = part_empty();
#pragma unroll
        for (int j = 0; j < kRays; ++j) {
            if (k == 0) {
                V3 e = V3{d[j].z, 0.0, -d[j].x};
                double ee = dot(e, e);
                if (ee == 0.0) {
                    e = V3{1.0, 0.0, 0.0};
                    ee = dot(e, e);
                }
                E1[j] = over(e, sqrt(ee));
                E2[j] = cross(d[j], E1[j]);
                b4[j] = d[j];
            }
            const double ci = fabs(dot(b4[j], N[j]));
            double Ts = 1.0, Tp = 1.0;
            if (inner) {
                double ts = cts, tp = ctp, qs = 1.0;
                Ts = cTs;
                Tp = cTp;
                if (model == kBare) {
                    const double ct = fabs(dot(d[j], N[j]));
                    const double A = n1 * ci, B = n2 * ct;
                    ts = (A + A) / (A + B);
                    tp = (A + A) / (n2 * ci + n1 * ct);
                    qs = B / A;
                    if (ci == 0.0)
                        ts = tp = qs = 0.0;
                    Ts = qs * (ts * ts);
                    Tp = qs * (tp * tp);
                }
                V3 c = cross(b4[j], N[j]);
                double cc = dot(c, c);
                if (cc == 0.0) {
                    c = fabs(b4[j].x) <= fabs(b4[j].y) ? cross(b4[j], V3{1.0, 0.0, 0.0})
                                                       : cross(b4[j], V3{0.0, 1.0, 0.0});
                    cc = dot(c, c);
                }
                const V3 sh = over(c, sqrt(cc));
                const V3 pi = cross(b4[j], sh), po = cross(d[j], sh);
                E1[j] = through(E1[j], sh, pi, po, ts, tp);
                E2[j] = through(E2[j], sh, pi, po, ts, tp);
                q[j] = q[j] * qs;
            }
            if (ok[j]) {
                t.v[0] += 1.0;
                t.v[1] += Ts;
                t.v[2] += Tp;
                t.v[3] += (Ts + Tp) / 2.0;
                t.v[4] = fmin(t.v[4], Ts);
                t.v[5] = fmin(t.v[5], Tp);
                t.v[6] += ci;
                t.v[7] = fmin(t.v[7], ci);
            }
            b4[j] = d[j];
        }
        if (out) {
            t = wave_merge<false>(t);
            if (lane == 0)
                out[k] = t;
        }
    }

    // the rows of each ray, and the item's partial record
    const double inf = __builtin_inf();
    Part t{{0.0, 0.0, 0.0, 0.0, inf, -inf, 0.0, -inf}};
#pragma unroll
    for (int j = 0; j < kRays; ++j) {
        const double g11 = dot(E1[j], E1[j]), g12 = dot(E1[j], E2[j]), g22 = dot(E2[j], E2[j]);
        const double m = (g11 + g22) / 2.0, h = (g11 - g22) / 2.0;
        const double rr = sqrt(h * h + g12 * g12);
        const double T = q[j] * m, T1 = q[j] * g11, T2 = q[j] * g22;
        const double D = m == 0.0 ? 0.0 : rr / m;
        if (ok[j]) {
            t.v[0] += 1.0;
            t.v[1] += T;
            t.v[2] += T1;
            t.v[3] += T2;
            t.v[4] = fmin(t.v[4], T);
            t.v[5] = fmax(t.v[5], T);
            t.v[6] += D;
            t.v[7] = fmax(t.v[7], D);
        }
        if (a.rows && r[j] < a.n_rays) {
            double *row = a.rows + (size_t)blockIdx.y * a.n_rows * a.ld_rows + (r[j] - a.row_ray0);
            row[0] = ok[j] ? T : nan;
            row[a.ld_rows] = ok[j] ? T1 : nan;
            row[2 * a.ld_rows] = ok[j] ? T2 : nan;
            row[3 * a.ld_rows] = ok[j] ? D : nan;
            if (a.n_rows == 10) {
                row[4 * a.ld_rows] = ok[j] ? E1[j].x : nan;
                row[5 * a.ld_rows] = ok[j] ? E1[j].y : nan;
                row[6 * a.ld_rows] = ok[j] ? E1[j].z : nan;
                row[7 * a.ld_rows] = ok[j] ? E2[j].x : nan;
                row[8 * a.ld_rows] = ok[j] ? E2[j].y : nan;
                row[9 * a.ld_rows] = ok[j] ? E2[j].z : nan;
            }
        }
    }
    if (out) {
        t = wave_merge<true>(t);
        if (lane == 0)
            out[n_seg] = t;
    }
}

// block (k, item): slot k's record, or with k == n_seg the item's, its partial records merged in the
// order of rox::block_merge
__global__ __launch_bounds__(kBlock) void fresnel_finish(const Part *__restrict__ part, int n_waves, int n_seg,
                                                         int64_t n_rays, rox_tx_surface *__restrict__ surf,
                                                         rox_tx_item *__restrict__ item)
{
    __shared__ Part sa[kBlock];
    const int k = blockIdx.x;
    const Part *p = part + (size_t)blockIdx.y * n_waves * (n_seg + 1) + k;
    const double nan = __builtin_nan(""), inf = __builtin_inf();
    if (k < n_seg) {
        const Part m = rox::block_merge<kBlock>(p, n_waves, n_seg + 1, part_empty(),
                                                [](Part &a, const Part &b) { part_merge<false>(a, b); }, sa);
        if (threadIdx.x == 0) {
            const bool any = m.v[0] > 0.0;
            rox_tx_surface f;
            f.n = (int64_t)m.v[0];
            f.ts_sum = m.v[1]; f.tp_sum = m.v[2]; f.t_sum = m.v[3];
            f.ts_min = any ? m.v[4] : nan; f.tp_min = any ? m.v[5] : nan;
            f.ci_sum = m.v[6]; f.ci_min = any ? m.v[7] : nan;
            surf[(size_t)blockIdx.y * n_seg + k] = f;
        }
    } else {
        const Part m = rox::block_merge<kBlock>(p, n_waves, n_seg + 1, Part{{0.0, 0.0, 0.0, 0.0, inf, -inf, 0.0, -inf}},
                                                [](Part &a, const Part &b) { part_merge<true>(a, b); }, sa);
        if (threadIdx.x == 0) {
            const bool any = m.v[0] > 0.0;
            rox_tx_item f;
            f.n_ok = (int64_t)m.v[0];
            f.n_rays = n_rays;
            f.t_sum = m.v[1]; f.t_min = any ? m.v[4] : nan; f.t_max = any ? m.v[5] : nan;
            f.t1_sum = m.v[2]; f.t2_sum = m.v[3];
            f.d_sum = m.v[6]; f.d_max = any ? m.v[7] : nan;
            item[blockIdx.y] = f;
        }
    }
}

rox::PerStream<rox::Workspace> g_tx_ws;

}  // namespace

extern "C" int rox_surface_transmission(rox_system *sys, uint32_t trace_flags, uint32_t tx_flags, int32_t n_items,
                                        const rox_out *outs, int64_t n_rays, const int32_t *wvl_idx,
                                        int32_t n_coat, const int32_t *coat_kind, const double *coat_value,
                                        double *rows, int64_t ld_rows, rox_tx_surface *surf, rox_tx_item *item,
                                        void *stream)
{
    static const char kE[] = "rox_surface_transmission";
    // every argument check comes before anything touches a device; those that do not need the
    // system come before the system is read
    ROX_TRY(rox::check_packet_call(kE, sys, outs, n_items));
    if (tx_flags & ~ROX_TX_FIELDS)
        return rox::host_fail(ROX_E_ARG, "%s: unknown tx_flags bits 0x%x", kE, tx_flags & ~ROX_TX_FIELDS);
    ROX_TRY(rox::check_packet_rays(kE, n_rays));
    if (!rows && !surf && !item)
        return rox::host_fail(ROX_E_ARG, "%s: null rows, surf and item", kE);
    if (rows && ld_rows < n_rays)
        return rox::host_fail(ROX_E_ARG, "%s: ld_rows %lld < n_rays %lld", kE, (long long)ld_rows, (long long)n_rays);
    if (!wvl_idx)
        return rox::host_fail(ROX_E_ARG, "%s: null wvl_idx", kE);
    for (int32_t i = 0; i < n_items; ++i) {
        ROX_TRY(rox::check_packet_item(kE, i, outs[i], n_rays, false));
        if (wvl_idx[i] < 0)
            return rox::host_fail(ROX_E_ARG, "%s: item %d: wvl_idx %d outside the index table", kE, i, wvl_idx[i]);
    }
    if ((coat_kind == nullptr) != (coat_value == nullptr))
        return rox::host_fail(ROX_E_ARG, "%s: coat_kind and coat_value go together", kE);
    if (coat_kind) {
        if (n_coat < 2)
            return rox::host_fail(ROX_E_ARG, "%s: n_coat %d is not the number of interfaces", kE, n_coat);
        for (int32_t s = 0; s < n_coat; ++s) {
            if (coat_kind[s] < ROX_COAT_BARE || coat_kind[s] > ROX_COAT_FIXED)
                return rox::host_fail(ROX_E_ARG, "%s: coat_kind[%d] = %d is not a ROX_COAT_* kind", kE, s,
                                      coat_kind[s]);
            for (int c = 0; c < 2 && coat_kind[s] == ROX_COAT_FIXED; ++c)
                if (!(coat_value[2 * s + c] >= 0.0 && coat_value[2 * s + c] <= 1.0))
                    return rox::host_fail(ROX_E_ARG, "%s: coat_value[%d][%d] = %g outside [0, 1]", kE, s, c,
                                          coat_value[2 * s + c]);
        }
    }
    const rox::PacketSlots ps(sys, trace_flags);
    const int32_t n_ifcs = ps.n_ifcs, n_seg = ps.n_seg;
    for (int32_t i = 0; i < n_items; ++i)
        if (wvl_idx[i] >= sys->n_wvls)
            return rox::host_fail(ROX_E_ARG, "%s: item %d: wvl_idx %d outside the index table of %d wavelengths",
                                  kE, i, wvl_idx[i], sys->n_wvls);
    if (coat_kind && n_coat != n_ifcs)
        return rox::host_fail(ROX_E_ARG, "%s: n_coat %d is not the number of interfaces %d", kE, n_coat, n_ifcs);

    hipStream_t st = (hipStream_t)stream;
    rox::PerStream<rox::Workspace>::Slot *slot;
    ROX_TRY(g_tx_ws.take(st, kHipWhere, &slot));
    std::lock_guard<std::mutex> turn(slot->mu);
    rox::Workspace *ws = &slot->data;

    const bool want_rec = surf || item;
    const bool rows_host = rows && !rox::is_device(rows);
    const bool host_dst = rows_host || (surf && !rox::is_device(surf)) || (item && !rox::is_device(item));
    const int n_rows = (tx_flags & ROX_TX_FIELDS) ? 10 : 4;
    const int64_t n_tiles = (n_rays + kTile - 1) / kTile;
    const int n_waves = (int)n_tiles * kWaves;
    // rows bound for host memory pass through the scratch, a range of rays at a time
    const int64_t range_tiles =
        rows_host ? std::max<int64_t>(1, std::min<int64_t>(n_tiles, (int64_t)(kTxScratchBytes / 4 /
                                                                              (sizeof(double) * n_rows * kTile))))
                  : n_tiles;
    const int64_t range_rays = range_tiles * kTile;
    const size_t b_rows = rows_host ? rox::up256(sizeof(double) * n_rows * (size_t)range_rays) : 0;
    const size_t b_part = want_rec ? rox::up256(sizeof(Part) * (size_t)n_waves * (n_seg + 1)) : 0;
    const size_t b_surf = want_rec ? rox::up256(sizeof(rox_tx_surface) * (size_t)n_seg) : 0;
    const size_t b_item = want_rec ? 256 : 0;
    const int64_t chunk = rox::chunk_for(n_items, b_rows + b_part + b_surf + b_item + 256, kTxScratchBytes);

    // the tables, staged as one block: [items][rt][coat][model][slot_ifc]
    const size_t o_rt = sizeof(ItemIn) * (size_t)n_items, o_cv = o_rt + sizeof(double) * kRtDoubles * n_ifcs;
    const size_t o_md = o_cv + sizeof(double) * 2 * n_ifcs, o_si = o_md + sizeof(int32_t) * n_ifcs;
    const size_t b_tab = o_si + sizeof(int32_t) * n_seg;
    char *d_tab;
    double *d_rows;
    Part *d_part;
    rox_tx_surface *d_surf;
    rox_tx_item *d_item;
    rox::Layout L;
    L.add(d_tab, rox::up256(b_tab));
    L.add(d_rows, b_rows * chunk);
    L.add(d_part, b_part * chunk);
    L.add(d_surf, b_surf * chunk);
    L.add(d_item, want_rec ? rox::up256(sizeof(rox_tx_item) * (size_t)chunk) : 0);
    HIP_TRY(ws->reserve(L.size()));
    L.carve(ws->buf);
    HIP_TRY(ws->stage.acquire(b_tab));
    char *h = ws->stage.h;
    for (int32_t i = 0; i < n_items; ++i)
        ((ItemIn *)h)[i] = ItemIn{outs[i].seg, outs[i].status, outs[i].ld, wvl_idx[i], 0};
    ps.stage_rt((double *)(h + o_rt));
    ps.stage_slot_ifc((int32_t *)(h + o_si));
    for (int32_t i = 0; i < n_ifcs; ++i) {
        const rox_surface &row = ps.rows[i];
        const int kind = coat_kind ? coat_kind[i] : ROX_COAT_BARE;
        const bool mirror = row.mode == ROX_REFLECT, glass = row.mode == ROX_TRANSMIT;
        int32_t model = kIdeal;
        if (mirror)
            model = kind == ROX_COAT_FIXED ? kFixedMirror : kMirror;
        else if (glass && kind == ROX_COAT_FIXED)
            model = kFixed;
        else if (glass && kind == ROX_COAT_BARE && row.profile != ROX_THINLENS && row.ph.kind == ROX_PH_NONE)
            model = kBare;
        const bool fixed = model == kFixed || model == kFixedMirror;
        ((double *)(h + o_cv))[2 * i] = fixed ? coat_value[2 * i] : 1.0;
        ((double *)(h + o_cv))[2 * i + 1] = fixed ? coat_value[2 * i + 1] : 1.0;
        ((int32_t *)(h + o_md))[i] = model;
    }
    HIP_TRY(hipMemcpyAsync(d_tab, h, b_tab, hipMemcpyHostToDevice, st));
    HIP_TRY(ws->stage.record(st));

    TxArgs a{};
    a.rt = (const double *)(d_tab + o_rt);
    a.coat = (const double *)(d_tab + o_cv);
    a.model = (const int32_t *)(d_tab + o_md);
    a.slot_ifc = (const int32_t *)(d_tab + o_si);
    a.n_table = sys->d_ntab;
    a.n_ifcs = n_ifcs; a.n_seg = n_seg; a.n_rays = n_rays;
    a.n_rows = n_rows; a.n_waves = n_waves;
    a.part = want_rec ? d_part : nullptr;
    for (int64_t i0 = 0; i0 < n_items; i0 += chunk) {
        const int64_t c = std::min<int64_t>(chunk, n_items - i0);
        a.items = (const ItemIn *)d_tab + i0;
        for (int64_t t0 = 0; t0 < n_tiles; t0 += range_tiles) {
            const int64_t nt = std::min<int64_t>(range_tiles, n_tiles - t0);
            const int64_t first = t0 * kTile, count = std::min<int64_t>(nt * kTile, n_rays - first);
            a.ray0 = first;
            a.rows = rows ? (rows_host ? d_rows : rows + (size_t)i0 * n_rows * ld_rows) : nullptr;
            a.ld_rows = rows_host ? range_rays : ld_rows;
            a.row_ray0 = rows_host ? first : 0;
            hipLaunchKernelGGL(fresnel_kernel, dim3((unsigned)nt, (unsigned)c), dim3(kBlock), 0, st, a);
            HIP_TRY(hipGetLastError());
            // this range's rows, copied before the next launch reuses the scratch
            if (rows_host)
                HIP_TRY(hipMemcpy2DAsync(rows + (size_t)i0 * n_rows * ld_rows + first, sizeof(double) * ld_rows,
                                         d_rows, sizeof(double) * range_rays, sizeof(double) * count,
                                         (size_t)c * n_rows, hipMemcpyDeviceToHost, st));
        }
        if (want_rec) {
            hipLaunchKernelGGL(fresnel_finish, dim3((unsigned)(n_seg + 1), (unsigned)c), dim3(kBlock), 0, st,
                               (const Part *)d_part, n_waves, n_seg, n_rays, d_surf, d_item);
            HIP_TRY(hipGetLastError());
            if (surf)
                HIP_TRY(hipMemcpyAsync(surf + (size_t)i0 * n_seg, d_surf, sizeof(rox_tx_surface) * (size_t)n_seg * c,
                                       hipMemcpyDefault, st));
            if (item)
                HIP_TRY(hipMemcpyAsync(item + i0, d_item, sizeof(rox_tx_item) * (size_t)c, hipMemcpyDefault, st));
        }
    }
    if (host_dst)
        HIP_TRY(hipStreamSynchronize(st));
    return 0;
}
