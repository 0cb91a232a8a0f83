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
// finishing kernel merges them in a fixed order.  No floating-point atomics.  (The tile, the
// merges and the host's turn are those of every packet entry: rox_packets.hpp.)
//
// rox_surface_thinfilm is the same walk with complex field vectors and, where an interface has a
// stack of thin films or a metal behind it, the characteristic matrix of the stack evaluated per
// ray (the layer loop wave-uniform in trip count, a stack's layer tables for the item's wavelength
// scalar loads as well).  The walk is written once, fresnel_kernel<F, Args>, and instantiated for
// real (V3, TxArgs) and for complex (C3, FilmArgs) field vectors; what the two do differently is in
// the overloads beside carry and through, and the stack exists only in the complex instantiation.
// Both entries share the argument checks, the staging, the launch loop and the finishing kernel
// (tx_entry).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "rox_math.hpp"
#include "rox_packets.hpp"
#include "rox_system.hpp"

namespace {

using rox::ctbli;
using rox::ctblp;
using rox::kRtDoubles;

constexpr char kHipWhere[] = "rox_surface_transmission: ";

using Tile = rox::PacketTile<2>;                // rays per thread: 107 VGPRs and 4 waves per SIMD (real), 214 and 2
                                                // (complex), no scratch
constexpr int kBlock = Tile::kBlock, kWaves = Tile::kWaves, kRays = Tile::kRays, kTile = Tile::kTile;
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
    kStack = 5,                                 // thin films between two real media (the complex walk only)
    kStackMirror = 6,                           // thin films, or none, over a metal
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

// what the complex walk reads besides: a layer's row of `layer` is (re N^2, im N^2, re 1/N^2, im 1/N^2).
// Derived, so that the walk binds the TxArgs of either launch as `const TxArgs &` to the kernel
// argument itself: reached through a function that returns a reference, the packet and status
// reads of both instantiations turn from global into flat loads.
struct FilmArgs : TxArgs {                      // n_rows is 4 or 16
    const double *wvl;                          // [chunk's items] vacuum wavelength, the thicknesses' unit
    const int32_t *stack_first;                 // [n_ifcs + 1] CSR offsets into the layers
    const double *thick;                        // [n_layers]
    const double *layer;                        // [n_wvls][n_layers][4]
    const double *sub;                          // [n_wvls][n_ifcs][2] N^2 behind a kStackMirror
    int32_t n_layers;
};

// V3, dot, cross and carry (rt . v in the row's rt_order, unfused): rox_packets.hpp
using rox::carry;
using rox::cross;
using rox::dot;
using rox::V3;

__device__ __forceinline__ V3 over(const V3 &a, double s) { return V3{a.x / s, a.y / s, a.z / s}; }

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

// ---- thin films: complex amplitudes (include/roxtrace.h rox_surface_thinfilm states the order)
struct Cx {
    double r, i;
};

__device__ __forceinline__ Cx cmul(const Cx &a, const Cx &b)
{
    return Cx{a.r * b.r - a.i * b.i, a.r * b.i + a.i * b.r};
}
__device__ __forceinline__ Cx cinv(const Cx &a)
{
    const double m = a.r * a.r + a.i * a.i;
    return Cx{a.r / m, -a.i / m};
}
// sqrt(zr + i zi), zi >= 0, on the branch Im >= 0 (Re >= 0 when Im == 0)
__device__ __forceinline__ Cx csqrt_up(double zr, double zi)
{
    const double m = sqrt(zr * zr + zi * zi);
    if (zr >= 0.0) {
        const double gr = sqrt((m + zr) / 2.0);
        return Cx{gr, gr == 0.0 ? 0.0 : zi / (gr + gr)};
    }
    const double gi = sqrt((m - zr) / 2.0);
    return Cx{zi / (gi + gi), gi};
}
// a layer of admittance y (iy = 1/y): (B, C) <- (cs*B - i*sn*C/y, -i*y*sn*B + cs*C)
__device__ __forceinline__ void film_layer(Cx &B, Cx &C, const Cx &cs, const Cx &sn, const Cx &y, const Cx &iy)
{
    const Cx u = cmul(sn, cmul(C, iy)), v = cmul(cmul(y, sn), B);
    const Cx cb = cmul(cs, B), cc = cmul(cs, C);
    B = Cx{cb.r + u.i, cb.i - u.r};
    C = Cx{cc.r + v.i, cc.i - v.r};
}

struct C3 {
    V3 re, im;
};

// What a complex field vector does differently from a real one: the walk below is written once
// over either, and these overloads (with carry and through above) are all that tells them apart.
__device__ __forceinline__ C3 carry(ctblp rt, bool c_order, const C3 &v)
{
    return C3{carry(rt, c_order, v.re), carry(rt, c_order, v.im)};
}

// a field that starts as the real vector v
__device__ __forceinline__ void start(V3 &E, const V3 &v) { E = v; }
__device__ __forceinline__ void start(C3 &E, const V3 &v) { E = C3{v, V3{0.0, 0.0, 0.0}}; }

// ts and tp are real for a real field and complex for a complex one, where only a stack gives them
// an imaginary part: the real part of either
__device__ __forceinline__ double &re(double &t) { return t; }
__device__ __forceinline__ double &re(Cx &t) { return t.r; }

// real ts, tp act on the real and on the imaginary part separately
__device__ __forceinline__ C3 through(const C3 &E, const V3 &s, const V3 &pi, const V3 &po, double ts, double tp)
{
    return C3{through(E.re, s, pi, po, ts, tp), through(E.im, s, pi, po, ts, tp)};
}

// E <- (ts*(s . E))*s + (tp*(p_in . E))*p_out with complex ts, tp and E
__device__ __forceinline__ C3 through_cx(const C3 &E, const V3 &s, const V3 &pi, const V3 &po, const Cx &ts,
                                         const Cx &tp)
{
    const Cx a = cmul(ts, Cx{dot(s, E.re), dot(s, E.im)}), b = cmul(tp, Cx{dot(pi, E.re), dot(pi, E.im)});
    return C3{V3{a.r * s.x + b.r * po.x, a.r * s.y + b.r * po.y, a.r * s.z + b.r * po.z},
              V3{a.i * s.x + b.i * po.x, a.i * s.y + b.i * po.y, a.i * s.z + b.i * po.z}};
}

// the Gram products of the two fields: <E1, E1>, <E2, E2> and |<E1, E2>|^2 (Hermitian when complex)
struct Gram {
    double g11, g22, g12sq;
};
__device__ __forceinline__ Gram gram(const V3 &E1, const V3 &E2)
{
    const double g11 = dot(E1, E1), g12 = dot(E1, E2), g22 = dot(E2, E2);
    return Gram{g11, g22, g12 * g12};
}
__device__ __forceinline__ Gram gram(const C3 &E1, const C3 &E2)
{
    const double g11 = dot(E1.re, E1.re) + dot(E1.im, E1.im), g22 = dot(E2.re, E2.re) + dot(E2.im, E2.im);
    const double g12r = dot(E1.re, E2.re) + dot(E1.im, E2.im), g12i = dot(E1.re, E2.im) - dot(E1.im, E2.re);
    return Gram{g11, g22, g12r * g12r + g12i * g12i};
}

// the field rows of a ray, from row `first` of its column `row` on: E1, E2 (6 rows), or re(E1), re(E2),
// im(E1), im(E2) (12)
__device__ __forceinline__ void store_fields(double *row, int64_t ld, int first, bool ok, const V3 &E1, const V3 &E2)
{
    const double nan = __builtin_nan("");
    const double f[6] = {E1.x, E1.y, E1.z, E2.x, E2.y, E2.z};
#pragma unroll
    for (int c = 0; c < 6; ++c)
        row[(first + c) * ld] = ok ? f[c] : nan;
}
__device__ __forceinline__ void store_fields(double *row, int64_t ld, int first, bool ok, const C3 &E1, const C3 &E2)
{
    store_fields(row, ld, first, ok, E1.re, E2.re);
    store_fields(row, ld, first + 6, ok, E1.im, E2.im);
}

// the state of a ray along the walk
template <class F>
struct Ray {
    int64_t r;
    bool ok;
    V3 b4;                                      // the direction before the slot
    F E1, E2;
    double q;                                   // the flux factor
};

// The walk of both entries: F = V3, Args = TxArgs carries real field vectors (rox_surface_transmission),
// F = C3, Args = FilmArgs complex ones (rox_surface_thinfilm).  Both walk the same tile with the same
// rays per thread and wave, so the partial sums of the records are formed in the same order.  An
// interface of the models kIdeal .. kFixedMirror applies the same real formulas to either field;
// kStack / kStackMirror, in the complex walk only, evaluate the stack per ray: the layer loop's trip
// count, a layer's N^2 and thickness and the wavelength are wave-uniform (scalar loads); s and p
// share g, delta, its cosine and its sine.
template <class F, class Args>
__global__ __launch_bounds__(kBlock) void fresnel_kernel(const Args args)
{
    constexpr bool kFilm = std::is_same<F, C3>::value;
    using Co = typename std::conditional<kFilm, Cx, double>::type;      // of (ts, tp)
    const TxArgs &a = args;                     // bound to the argument itself: see FilmArgs
    const ItemIn it = a.items[blockIdx.y];
    const int lane = threadIdx.x & 63;
    const int n_seg = a.n_seg;
    // the tables through the constant address space (rox_math.hpp): a wave-uniform address there is
    // a scalar load into SGPRs, and the stores of the partial records do not order it
    const ctbli slot_ifc = (ctbli)a.slot_ifc, model_of = (ctbli)a.model;
    const ctblp rt_of = (ctblp)a.rt, coat = (ctblp)a.coat;
    const ctblp ntab = (ctblp)a.n_table + (size_t)it.wvl * a.n_ifcs;
    [[maybe_unused]] ctbli first = nullptr;
    [[maybe_unused]] ctblp thick = nullptr, layer = nullptr, sub = nullptr;
    [[maybe_unused]] double wvl = 1.0;
    if constexpr (kFilm) {
        first = (ctbli)args.stack_first;
        thick = (ctblp)args.thick;
        layer = (ctblp)args.layer + (size_t)it.wvl * args.n_layers * 4;
        sub = (ctblp)args.sub + (size_t)it.wvl * a.n_ifcs * 2;
        wvl = args.wvl ? ((ctblp)args.wvl)[blockIdx.y] : 1.0;
    }
    const double nan = __builtin_nan("");

    const V3 zero{0.0, 0.0, 0.0};
    Ray<F> ray[kRays];
#pragma unroll
    for (int j = 0; j < kRays; ++j) {
        Ray<F> &y = ray[j];
        y.r = Tile::ray(j, a.ray0);
        y.ok = y.r < a.n_rays && it.status[y.r] == ROX_OK;
        y.b4 = zero;
        start(y.E1, zero);
        start(y.E2, zero);
        y.q = 1.0;
    }
    Part *out = a.part ? a.part + Tile::part(a.n_waves, n_seg + 1, a.ray0) : nullptr;

    for (int k = 0; k < n_seg; ++k) {
        const double *rec = it.seg + (size_t)k * ROX_SEG_DOUBLES * it.ld;
        V3 dj[kRays], Nj[kRays];
#pragma unroll
        for (int j = 0; j < kRays; ++j) {
            const int64_t r = ray[j].r;
            dj[j] = Nj[j] = zero;
            if (ray[j].ok) {
                dj[j] = V3{rec[3 * it.ld + r], rec[4 * it.ld + r], rec[5 * it.ld + r]};
                Nj[j] = V3{rec[7 * it.ld + r], rec[8 * it.ld + r], rec[9 * it.ld + r]};
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
                    Ray<F> &y = ray[j];
                    y.b4 = carry(rt, c_order, y.b4);
                    y.E1 = carry(rt, c_order, y.E1);
                    y.E2 = carry(rt, c_order, y.E2);
                }
            }

        // the slot's model: the same for every ray of the workgroup
        const bool inner = k > 0 && k < n_seg - 1;
        int model = kIdeal;
        double n1 = 1.0, n2 = 1.0, cTs = 1.0, cTp = 1.0, cts = 1.0, ctp = 1.0;
        [[maybe_unused]] int l0 = 0, l1 = 0;
        [[maybe_unused]] Cx sub2{1.0, 0.0};
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
            if constexpr (kFilm) {
                if (model == kStack || model == kStackMirror) {
                    l0 = first[s];
                    l1 = first[s + 1];
                }
                if (model == kStackMirror)
                    sub2 = Cx{sub[2 * s], sub[2 * s + 1]};
            }
        }
        const bool stack = kFilm && (model == kStack || model == kStackMirror);

        Part t = part_empty();
#pragma unroll
        for (int j = 0; j < kRays; ++j) {
            const V3 d = dj[j], N = Nj[j];
            V3 &b4 = ray[j].b4;
            F &E1 = ray[j].E1, &E2 = ray[j].E2;
            if (k == 0) {
                V3 e = V3{d.z, 0.0, -d.x};
                double ee = dot(e, e);
                if (ee == 0.0) {
                    e = V3{1.0, 0.0, 0.0};
                    ee = dot(e, e);
                }
                const V3 e1 = over(e, sqrt(ee));
                start(E1, e1);
                start(E2, cross(d, e1));
                b4 = d;
            }
            const double ci = fabs(dot(b4, N));
            double Ts = 1.0, Tp = 1.0;
            if (inner) {
                Co ts{cts}, tp{ctp};
                double qs = 1.0;
                Ts = cTs;
                Tp = cTp;
                if (model == kBare) {
                    const double ct = fabs(dot(d, N));
                    const double A = n1 * ci, B = n2 * ct;
                    re(ts) = (A + A) / (A + B);
                    re(tp) = (A + A) / (n2 * ci + n1 * ct);
                    qs = B / A;
                    if (ci == 0.0)
                        re(ts) = re(tp) = qs = 0.0;
                    Ts = qs * (re(ts) * re(ts));
                    Tp = qs * (re(tp) * re(tp));
                } else if constexpr (kFilm) {
                    if (stack) {
                        const double ct = fabs(dot(d, N));
                        const double A = n1 * ci, a2 = (n1 * n1) * (1.0 - ci * ci);
                        const double Bx = n2 * ct;
                        // (B, C) at the exit side: (1, y_exit) for s and for p
                        Cx ys{Bx, 0.0}, yp{(n2 * n2) / Bx, 0.0};
                        if (model == kStackMirror) {
                            ys = csqrt_up(sub2.r - a2, sub2.i);
                            yp = cmul(sub2, cinv(ys));
                        }
                        Cx Bs{1.0, 0.0}, Cs = ys, Bp{1.0, 0.0}, Cp = yp;
                        double att = 0.0;
                        for (int l = l1 - 1; l >= l0; --l) {
                            const Cx N2{layer[4 * l], layer[4 * l + 1]}, iN2{layer[4 * l + 2], layer[4 * l + 3]};
                            const double kd = (6.283185307179586 * thick[l]) / wvl;
                            const Cx g = csqrt_up(N2.r - a2, N2.i), ig = cinv(g);
                            const double x = kd * g.r, y = kd * g.i;
                            double sx, cx;
                            sincos(x, &sx, &cx);
                            // cos and sin of x + iy over e^y: only e^(-2y) <= 1 is formed
                            const double e2 = exp(-(y + y));
                            const double ch = (1.0 + e2) / 2.0, sh = (1.0 - e2) / 2.0;
                            const Cx cs{cx * ch, -(sx * sh)}, sn{sx * ch, cx * sh};
                            att = att + y;
                            film_layer(Bs, Cs, cs, sn, g, ig);
                            film_layer(Bp, Cp, cs, sn, cmul(N2, ig), cmul(g, iN2));
                        }
                        const double y0s = A, y0p = (n1 * n1) / A;
                        const Cx ds{y0s * Bs.r + Cs.r, y0s * Bs.i + Cs.i}, dp{y0p * Bp.r + Cp.r, y0p * Bp.i + Cp.i};
                        const Cx is = cinv(ds), ip = cinv(dp);
                        if (model == kStack) {
                            const double f = exp(-att);
                            const double fs = f * (y0s + y0s), fp = (f * (y0p + y0p)) * (ci / ct);
                            ts = Cx{fs * is.r, fs * is.i};
                            tp = Cx{fp * ip.r, fp * ip.i};
                            qs = Bx / A;
                            if (ci == 0.0) {
                                ts = tp = Cx{0.0, 0.0};
                                qs = 0.0;
                            }
                        } else {
                            ts = cmul(Cx{y0s * Bs.r - Cs.r, y0s * Bs.i - Cs.i}, is);
                            const Cx rp = cmul(Cx{y0p * Bp.r - Cp.r, y0p * Bp.i - Cp.i}, ip);
                            tp = Cx{-rp.r, -rp.i};
                            if (ci == 0.0) {
                                ts = Cx{-1.0, 0.0};
                                tp = Cx{-1.0, 0.0};
                            }
                        }
                        Ts = qs * (ts.r * ts.r + ts.i * ts.i);
                        Tp = qs * (tp.r * tp.r + tp.i * tp.i);
                    }
                }
                V3 c = cross(b4, N);
                double cc = dot(c, c);
                if (cc == 0.0) {
                    c = fabs(b4.x) <= fabs(b4.y) ? cross(b4, V3{1.0, 0.0, 0.0}) : cross(b4, V3{0.0, 1.0, 0.0});
                    cc = dot(c, c);
                }
                const V3 sh = over(c, sqrt(cc));
                const V3 pi = cross(b4, sh), po = cross(d, sh);
                if (stack) {
                    if constexpr (kFilm) {
                        E1 = through_cx(E1, sh, pi, po, ts, tp);
                        E2 = through_cx(E2, sh, pi, po, ts, tp);
                    }
                } else {
                    E1 = through(E1, sh, pi, po, re(ts), re(tp));
                    E2 = through(E2, sh, pi, po, re(ts), re(tp));
                }
                ray[j].q = ray[j].q * qs;
            }
            if (ray[j].ok) {
                t.v[0] += 1.0;
                t.v[1] += Ts;
                t.v[2] += Tp;
                t.v[3] += (Ts + Tp) / 2.0;
                t.v[4] = fmin(t.v[4], Ts);
                t.v[5] = fmin(t.v[5], Tp);
                t.v[6] += ci;
                t.v[7] = fmin(t.v[7], ci);
            }
            b4 = d;
        }
        if (out) {
            rox::wave_merge(t, [](Part &m, const Part &b) { part_merge<false>(m, b); });
            if (lane == 0)
                out[k] = t;
        }
    }

    // the rows of each ray, and the item's partial record
    const double inf = __builtin_inf();
    Part t{{0.0, 0.0, 0.0, 0.0, inf, -inf, 0.0, -inf}};
#pragma unroll
    for (int j = 0; j < kRays; ++j) {
        const Ray<F> &y = ray[j];
        const Gram g = gram(y.E1, y.E2);
        const double m = (g.g11 + g.g22) / 2.0, h = (g.g11 - g.g22) / 2.0;
        const double rr = sqrt(h * h + g.g12sq);
        const double T = y.q * m, T1 = y.q * g.g11, T2 = y.q * g.g22;
        const double D = m == 0.0 ? 0.0 : rr / m;
        if (y.ok) {
            t.v[0] += 1.0;
            t.v[1] += T;
            t.v[2] += T1;
            t.v[3] += T2;
            t.v[4] = fmin(t.v[4], T);
            t.v[5] = fmax(t.v[5], T);
            t.v[6] += D;
            t.v[7] = fmax(t.v[7], D);
        }
        if (a.rows && y.r < a.n_rays) {
            double *row = a.rows + (size_t)blockIdx.y * a.n_rows * a.ld_rows + (y.r - a.row_ray0);
            row[0] = y.ok ? T : nan;
            row[a.ld_rows] = y.ok ? T1 : nan;
            row[2 * a.ld_rows] = y.ok ? T2 : nan;
            row[3 * a.ld_rows] = y.ok ? D : nan;
            if (a.n_rows == (kFilm ? 16 : 10))
                store_fields(row, a.ld_rows, 4, y.ok, y.E1, y.E2);
        }
    }
    if (out) {
        rox::wave_merge(t, [](Part &m, const Part &b) { part_merge<true>(m, b); });
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

// what rox_surface_thinfilm takes besides (HOST arrays)
struct Film {
    const double *wvl;                          // [n_items]
    const int32_t *stack_first;                 // [n_coat + 1]
    const double *thick;                        // [n_layers]
    const double *index;                        // [n_wvls][n_layers][2]
    const double *sub;                          // [n_wvls][n_coat][2]
};

inline bool index_ok(double re, double im, bool layer)
{
    return std::isfinite(re) && std::isfinite(im) && im >= 0.0 && (layer ? re > 0.0 : (re >= 0.0 && re + im > 0.0));
}

// the layer checks of wavelength row w
int check_layer_index(const char *kE, const Film *film, int32_t n_layers, int32_t w)
{
    for (int32_t l = 0; l < n_layers; ++l) {
        const double *v = film->index + 2 * ((size_t)w * n_layers + l);
        if (!index_ok(v[0], v[1], true))
            return rox::host_fail(ROX_E_ARG, "%s: layer_index[%d][%d] = (%g, %g): re must be > 0 and im >= 0", kE, w,
                                  l, v[0], v[1]);
    }
    return 0;
}

// both entries: rox_surface_transmission (film == nullptr, the real walk) and rox_surface_thinfilm
int tx_entry(const char *kE, const Film *film, rox_system *sys, uint32_t trace_flags, uint32_t tx_flags,
             int32_t n_items, const rox_out *outs, int64_t n_rays, const int32_t *wvl_idx, int32_t n_coat,
             const int32_t *coat_kind, const double *coat_value, double *rows, int64_t ld_rows, rox_tx_surface *surf,
             rox_tx_item *item, void *stream)
{
    // HIP_TRY (rox_host.hpp) names `kHipWhere` for the prefix of its messages: this local, in place of
    // the file's, gives it the prefix of the entry that called
    const char *const kHipWhere = film ? "rox_surface_thinfilm: " : ::kHipWhere;
    const int max_kind = film ? ROX_COAT_STACK : ROX_COAT_FIXED;
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
            if (coat_kind[s] < ROX_COAT_BARE || coat_kind[s] > max_kind)
                return rox::host_fail(ROX_E_ARG, "%s: coat_kind[%d] = %d is not a ROX_COAT_* kind", kE, s,
                                      coat_kind[s]);
            for (int c = 0; c < 2 && coat_kind[s] == ROX_COAT_FIXED; ++c)
                if (!(coat_value[2 * s + c] >= 0.0 && coat_value[2 * s + c] <= 1.0))
                    return rox::host_fail(ROX_E_ARG, "%s: coat_value[%d][%d] = %g outside [0, 1]", kE, s, c,
                                          coat_value[2 * s + c]);
        }
    }
    // the stacks: what can be checked without the system (of layer_index the first wavelength's row)
    int32_t n_layers = 0;
    if (film) {
        const int32_t *sf = film->stack_first;
        if (sf && !coat_kind)
            return rox::host_fail(ROX_E_ARG, "%s: stack_first without coat_kind", kE);
        for (int32_t s = 0; coat_kind && s < n_coat; ++s) {
            if (coat_kind[s] == ROX_COAT_STACK && !sf)
                return rox::host_fail(ROX_E_ARG, "%s: coat_kind[%d] is ROX_COAT_STACK without stack_first", kE, s);
            if (!sf)
                continue;
            const int64_t n = (int64_t)sf[s + 1] - sf[s];
            if (sf[0] != 0 || n < 0 || n > ROX_MAX_COAT_LAYERS)
                return rox::host_fail(ROX_E_ARG, "%s: stack_first[%d]: %lld layers outside [0, %d] (stack_first[0] %d)",
                                      kE, s, (long long)n, ROX_MAX_COAT_LAYERS, sf[0]);
            if (n > 0 && coat_kind[s] != ROX_COAT_STACK)
                return rox::host_fail(ROX_E_ARG, "%s: stack_first[%d]: %lld layers where coat_kind[%d] = %d is not "
                                      "ROX_COAT_STACK", kE, s, (long long)n, s, coat_kind[s]);
            if (sf[s + 1] > ROX_MAX_COAT_LAYERS_TOTAL)
                return rox::host_fail(ROX_E_ARG, "%s: stack_first[%d] = %d: more than %d layers in all", kE, s + 1,
                                      sf[s + 1], ROX_MAX_COAT_LAYERS_TOTAL);
        }
        n_layers = sf ? sf[n_coat] : 0;
        if (n_layers > 0 && (!film->thick || !film->index || !film->wvl))
            return rox::host_fail(ROX_E_ARG, "%s: wvl, layer_thickness and layer_index go with the %d layers of "
                                  "stack_first", kE, n_layers);
        for (int32_t i = 0; film->wvl && i < n_items; ++i)
            if (!(std::isfinite(film->wvl[i]) && film->wvl[i] > 0.0))
                return rox::host_fail(ROX_E_ARG, "%s: item %d: wvl %g must be finite and > 0", kE, i, film->wvl[i]);
        for (int32_t l = 0; l < n_layers; ++l)
            if (!(std::isfinite(film->thick[l]) && film->thick[l] >= 0.0))
                return rox::host_fail(ROX_E_ARG, "%s: layer_thickness[%d] = %g must be finite and >= 0", kE, l,
                                      film->thick[l]);
        ROX_TRY(check_layer_index(kE, film, n_layers, 0));
    }
    const rox::PacketSlots ps(sys, trace_flags);
    const int32_t n_ifcs = ps.n_ifcs, n_seg = ps.n_seg;
    for (int32_t i = 0; i < n_items; ++i)
        if (wvl_idx[i] >= sys->n_wvls)
            return rox::host_fail(ROX_E_ARG, "%s: item %d: wvl_idx %d outside the index table of %d wavelengths",
                                  kE, i, wvl_idx[i], sys->n_wvls);
    if (coat_kind && n_coat != n_ifcs)
        return rox::host_fail(ROX_E_ARG, "%s: n_coat %d is not the number of interfaces %d", kE, n_coat, n_ifcs);
    // the stacks: what needs the system
    for (int32_t w = 1; film && w < sys->n_wvls; ++w)
        ROX_TRY(check_layer_index(kE, film, n_layers, w));
    for (int32_t s = 0; film && coat_kind && s < n_ifcs; ++s) {
        if (coat_kind[s] != ROX_COAT_STACK)
            continue;
        const rox_surface &row = ps.rows[s];
        const bool inner = s > 0 && s < n_ifcs - 1;
        const bool glass = row.mode == ROX_TRANSMIT && row.profile != ROX_THINLENS && row.ph.kind == ROX_PH_NONE;
        if (!inner || !(glass || row.mode == ROX_REFLECT))
            return rox::host_fail(ROX_E_ARG, "%s: coat_kind[%d]: a stack belongs on a ROX_TRANSMIT interface that is "
                                  "no thin lens or phase element, or on a ROX_REFLECT interface", kE, s);
        if (row.mode != ROX_REFLECT)
            continue;
        if (!film->sub)
            return rox::host_fail(ROX_E_ARG, "%s: coat_kind[%d]: a stack on a ROX_REFLECT interface needs sub_index",
                                  kE, s);
        for (int32_t w = 0; w < sys->n_wvls; ++w) {
            const double *v = film->sub + 2 * ((size_t)w * n_ifcs + s);
            if (!index_ok(v[0], v[1], false))
                return rox::host_fail(ROX_E_ARG, "%s: sub_index[%d][%d] = (%g, %g): re and im must be >= 0 and not "
                                      "both 0", kE, w, s, v[0], v[1]);
        }
    }

    hipStream_t st = (hipStream_t)stream;
    rox::Turn<> ws;
    ROX_TRY(ws.take(g_tx_ws, st, kHipWhere));

    const bool want_rec = surf || item;
    const bool rows_host = rows && !rox::is_device(rows);
    const bool host_dst = rows_host || (surf && !rox::is_device(surf)) || (item && !rox::is_device(item));
    const int n_rows = (tx_flags & ROX_TX_FIELDS) ? (film ? 16 : 10) : 4;
    const int64_t n_tiles = Tile::tiles(n_rays);
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

    // the tables, staged as one block: [items][rt][coat][model][slot_ifc] and, for the stacks,
    // [stack_first][pad to 8][wvl][thickness][layer N^2, 1/N^2][sub N^2]
    const size_t o_rt = sizeof(ItemIn) * (size_t)n_items, o_cv = o_rt + sizeof(double) * kRtDoubles * n_ifcs;
    const size_t o_md = o_cv + sizeof(double) * 2 * n_ifcs, o_si = o_md + sizeof(int32_t) * n_ifcs;
    const size_t n_wl = film ? (size_t)sys->n_wvls : 0;
    const bool stacks = film && film->stack_first, sub = stacks && film->sub;
    const size_t o_sf = o_si + sizeof(int32_t) * n_seg;
    const size_t o_wv = (o_sf + (stacks ? sizeof(int32_t) * (n_ifcs + 1) : 0) + 7) & ~size_t(7);
    const size_t o_th = o_wv + (film && film->wvl ? sizeof(double) * n_items : 0);
    const size_t o_ly = o_th + sizeof(double) * n_layers, o_sb = o_ly + sizeof(double) * 4 * n_wl * n_layers;
    const size_t b_tab = film ? o_sb + (sub ? sizeof(double) * 2 * n_wl * n_ifcs : 0) : o_sf;
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
    char *h;
    ROX_TRY(ws.carve(L, b_tab, &h));
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
        if (kind == ROX_COAT_STACK)             // rox_surface_thinfilm only, where it was checked above
            model = mirror ? kStackMirror : kStack;
        const bool fixed = model == kFixed || model == kFixedMirror;
        ((double *)(h + o_cv))[2 * i] = fixed ? coat_value[2 * i] : 1.0;
        ((double *)(h + o_cv))[2 * i + 1] = fixed ? coat_value[2 * i + 1] : 1.0;
        ((int32_t *)(h + o_md))[i] = model;
    }
    if (stacks)
        memcpy(h + o_sf, film->stack_first, sizeof(int32_t) * (n_ifcs + 1));
    if (film && film->wvl)
        memcpy(h + o_wv, film->wvl, sizeof(double) * n_items);
    if (n_layers > 0)
        memcpy(h + o_th, film->thick, sizeof(double) * n_layers);
    // N^2 = (re*re - im*im, (re + re)*im) and its reciprocal conj(N^2) / |N^2|^2
    const auto square = [](const double *v, double *n2) {
        n2[0] = v[0] * v[0] - v[1] * v[1];
        n2[1] = (v[0] + v[0]) * v[1];
    };
    for (size_t j = 0; j < n_wl * n_layers; ++j) {
        double *n2 = (double *)(h + o_ly) + 4 * j;
        square(film->index + 2 * j, n2);
        const double m = n2[0] * n2[0] + n2[1] * n2[1];
        n2[2] = n2[0] / m;
        n2[3] = -n2[1] / m;
    }
    for (size_t j = 0; sub && j < n_wl * n_ifcs; ++j) {
        double *n2 = (double *)(h + o_sb) + 2 * j;
        n2[0] = 1.0;                            // read only behind a stack on a mirror
        n2[1] = 0.0;
        if (coat_kind[j % n_ifcs] == ROX_COAT_STACK && ps.rows[j % n_ifcs].mode == ROX_REFLECT)
            square(film->sub + 2 * j, n2);
    }
    ROX_TRY(ws.upload(d_tab, b_tab));

    FilmArgs fa{};
    if (film) {
        fa.stack_first = stacks ? (const int32_t *)(d_tab + o_sf) : nullptr;
        fa.thick = (const double *)(d_tab + o_th);
        fa.layer = (const double *)(d_tab + o_ly);
        fa.sub = sub ? (const double *)(d_tab + o_sb) : nullptr;
        fa.n_layers = n_layers;
    }
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
            if (film) {
                static_cast<TxArgs &>(fa) = a;
                fa.wvl = film->wvl ? (const double *)(d_tab + o_wv) + i0 : nullptr;
                hipLaunchKernelGGL((fresnel_kernel<C3, FilmArgs>), dim3((unsigned)nt, (unsigned)c), dim3(kBlock), 0,
                                   st, fa);
            } else {
                hipLaunchKernelGGL((fresnel_kernel<V3, TxArgs>), dim3((unsigned)nt, (unsigned)c), dim3(kBlock), 0, st,
                                   a);
            }
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

}  // namespace

extern "C" int rox_surface_transmission(rox_system *sys, uint32_t trace_flags, uint32_t tx_flags, int32_t n_items,
                                        const rox_out *outs, int64_t n_rays, const int32_t *wvl_idx,
                                        int32_t n_coat, const int32_t *coat_kind, const double *coat_value,
                                        double *rows, int64_t ld_rows, rox_tx_surface *surf, rox_tx_item *item,
                                        void *stream)
{
    return tx_entry("rox_surface_transmission", nullptr, sys, trace_flags, tx_flags, n_items, outs, n_rays, wvl_idx,
                    n_coat, coat_kind, coat_value, rows, ld_rows, surf, item, stream);
}

extern "C" int rox_surface_thinfilm(rox_system *sys, uint32_t trace_flags, uint32_t tx_flags, int32_t n_items,
                                    const rox_out *outs, int64_t n_rays, const int32_t *wvl_idx, const double *wvl,
                                    int32_t n_coat, const int32_t *coat_kind, const double *coat_value,
                                    const int32_t *stack_first, const double *layer_thickness,
                                    const double *layer_index, const double *sub_index, double *rows,
                                    int64_t ld_rows, rox_tx_surface *surf, rox_tx_item *item, void *stream)
{
    const Film film{wvl, stack_first, layer_thickness, layer_index, sub_index};
    return tx_entry("rox_surface_thinfilm", &film, sys, trace_flags, tx_flags, n_items, outs, n_rays, wvl_idx, n_coat,
                    coat_kind, coat_value, rows, ld_rows, surf, item, stream);
}
