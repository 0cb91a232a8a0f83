// zernike.hip -- rox_focus_zernike: least-squares Zernike fits of the OPD of every plane of a
// through-focus scan, next to the rows rox_trace_through_focus[_grids] leaves in HBM.
//
// Per item the fit is the normal equations G c_k = b_k with G = Z^T Z (n_terms^2, the same for
// every plane: status does not depend on focus) and b_k = Z^T W_k, Z evaluated once per ray.
//
// Basis: term j = P_j(s) * {1 | Re | Im}((x + i y)^|m|), s = x*x + y*y, P_j the radial polynomial
// R_n^|m| / rho^|m| in s with the term's scale folded into its coefficients on the host (exact
// integers times scale, one IEEE product each), evaluated by Horner from the highest power; the
// power (x + i y)^|m| by |m| complex products from (1, 0).  No trig, no sqrt.
//
// Passes (each a fixed order, no floating-point atomics; identical calls give identical bits):
//   zk_pass<kMoments>  a workgroup takes a chunk of rays of one item in 32-ray tiles; per tile it
//                      writes [Z | 1 | W] (rows of rays that are not fitted are zero) into LDS and
//                      accumulates the upper 16x16 tiles of G and the tiles of B with
//                      v_mfma_f64_16x16x4_f64.  The column "1" gives n and sum W.  One partial
//                      record per (item, chunk); zk_sum adds the chunks in order.
//   zk_solve           one workgroup per item: Jacobi-equilibrated Cholesky of G in LDS, pivots
//                      checked against kMinPivot; then per plane two triangular solves.
//   zk_pass<kRefine>   the same GEMM with W replaced by r = W - Z c: one step of iterative
//                      refinement (c += G^-1 Z^T r with the stored factor), which holds the
//                      coefficients at the accuracy of a least-squares solve on vignetted pupils
//                      where the normal equations alone lose cond(G) * eps.
//   zk_pass<kStats>    a third read: r = W - Z c per fitted ray, sums of r^2 and (W - mean)^2 and
//                      max / min r per plane, reduced per half-wave by a fixed butterfly; the
//                      integer counts n and n_outside by ballots; zk_finish adds the chunks in
//                      order and writes the rox_zernike_stats.
// The chunking of an item's rays is a function of its ray count alone, so splitting a job into
// launches (the scratch bound) does not change a bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "rox_host.hpp"

namespace {

constexpr char kHipWhere[] = "rox_focus_zernike: ";

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int kBlock = 256;                   // 4 waves
constexpr int kTile = 32;                     // rays per LDS tile (8 MFMA k-steps of 4)
constexpr int kGroups = kBlock / kTile;       // 8 thread groups of one half-wave each
constexpr int kPG = 32;                       // planes per workgroup (blockIdx.z groups)
constexpr int kMaxJP = 96;                    // ROX_MAX_ZERNIKE_TERMS + 1, rounded up to 16
constexpr int kMaxTilesPerWave = 9;           // (21 G tiles + 6 x 2 B tiles) / 4 waves, rounded up
constexpr int kRaysPerChunk = 8192;           // rays per workgroup before another chunk is added
constexpr int kMaxChunks = 64;                // chunks per item (bounds the partial records)
constexpr double kMinPivot = 1e-12;           // Cholesky pivot of the equilibrated G: below -> fit 2
constexpr size_t kScratchBytes = size_t(256) << 20;

enum Mode { kMoments = 0, kRefine = 1, kStats = 2 };

struct TermDev {
    int32_t m;      // |m|
    int32_t kind;   // 0: m == 0; 1: cos (Re); 2: sin (Im)
    int32_t nc;     // coefficients of P, highest power of s first
    int32_t off;    // into the coefficient table
};

struct ItemDev {
    const double *px, *py;   // the pupil axes, [num] each
    double cx, cy, radius, wave_scale;
    int64_t R;               // num * num
    int32_t num, nch;        // pupil axis length; ray chunks
    int64_t span;            // rays per chunk, a multiple of kTile
};

struct PassArgs {
    const double *rows;
    const uint8_t *status;
    int64_t ld;
    int32_t n_planes;
    int32_t i0;              // first item of this launch (rows / status index)
    int32_t J, JP;           // terms; columns of Z in LDS (J + 1 rounded up to 16)
    const ItemDev *items;    // [launch items]
    const TermDev *terms;
    const double *tcoef;
    double *part;            // [item][chunk][JP*JP + JP*K]   (moments / refine)
    const double *coef;      // [item][K][J]                  (refine / stats)
    const double *mean;      // [item][K]                     (stats)
    double *spart;           // [item][chunk][K][4]           (stats)
    int64_t *cpart;          // [item][chunk][2]              (stats)
};

__device__ __forceinline__ double basis(const TermDev &t, const double *tc, double x, double y, double s)
{
    const double *c = tc + t.off;
    double q = c[0];
    for (int i = 1; i < t.nc; ++i)
        q = q * s + c[i];
    if (t.kind == 0)
        return q;
    double re = 1.0, im = 0.0;
    for (int i = 0; i < t.m; ++i) {
        const double nr = re * x - im * y;
        const double ni = re * y + im * x;
        re = nr;
        im = ni;
    }
    return q * (t.kind == 1 ? re : im);
}

// ray r of item it: pupil coordinates normalised to the circle, and whether it is fitted
// (status OK and x*x + y*y <= 1); outside = OK but outside the circle
__device__ __forceinline__ bool select_ray(const PassArgs &a, const ItemDev &it, int64_t item, int64_t r,
                                           double &x, double &y, double &s, bool &outside)
{
    outside = false;
    if (r >= it.R || a.status[item * a.ld + r] != ROX_OK)
        return false;
    const int64_t ia = r / it.num, ib = r - ia * it.num;
    x = (it.px[ia] - it.cx) / it.radius;
    y = (it.py[ib] - it.cy) / it.radius;
    s = x * x + y * y;
    outside = !(s <= 1.0);
    return !outside;
}

template <int MODE>
__global__ void __launch_bounds__(kBlock) zk_pass(PassArgs a)
{
    extern __shared__ double M[];                        // [kTile][ldm], then this group's c [kPG][J]
    const int li = blockIdx.y, ch = blockIdx.x;
    const ItemDev it = a.items[li];
    if (ch >= it.nch)
        return;
    const int64_t item = a.i0 + li;
    const int K = a.n_planes, J = a.J, JP = a.JP;
    const int k0 = blockIdx.z * kPG, kg = min(kPG, K - k0);
    const int KGP = (kg + 15) & ~15;
    const int ncol = JP + KGP;
    // an odd row pitch: the 32 rays of a half-wave reading one column of their rows (the r = W - Z c
    // dot products) hit 32 distinct bank pairs; the MFMA operand reads pay at most 2-way
    const int ldm = ncol + 1;
    double *cs = M + kTile * (kMaxJP + kPG + 1);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ray_l = tid & (kTile - 1), grp = tid >> 5;
    const int64_t rb = (int64_t)ch * it.span, re = min<int64_t>(it.R, rb + it.span);

    // GEMM tiles of this wave: G's upper tiles (moments, first plane group only), then B's
    const int nrt = JP / 16;
    const int ng = (MODE == kMoments && blockIdx.z == 0) ? nrt * (nrt + 1) / 2 : 0;
    const int ntiles = ng + nrt * (KGP / 16);
    d4 acc[kMaxTilesPerWave];
    int arow[kMaxTilesPerWave], acol[kMaxTilesPerWave];   // first row / column of tile i in M
#pragma unroll
    for (int i = 0; i < kMaxTilesPerWave; ++i) {
        acc[i] = d4{0., 0., 0., 0.};
        const int tix = wave + 4 * i;
        int rt = 0, co = 0;
        if (tix < ng) {                                  // G tile (rt, ct), ct >= rt, row-major
            int rem = tix;
            while (rem >= nrt - rt) {
                rem -= nrt - rt;
                ++rt;
            }
            co = 16 * (rt + rem);
        } else if (tix < ntiles) {                       // B tile: W columns
            rt = (tix - ng) % nrt;
            co = JP + 16 * ((tix - ng) / nrt);
        }
        arow[i] = 16 * rt;
        acol[i] = co;
    }

    // stats accumulators: planes grp + kGroups * i of this group
    constexpr int kPP = kPG / kGroups;
    double s_r2[kPP], s_d2[kPP], s_max[kPP], s_min[kPP];
#pragma unroll
    for (int i = 0; i < kPP; ++i) {
        s_r2[i] = s_d2[i] = 0.0;
        s_max[i] = -INFINITY;
        s_min[i] = INFINITY;
    }
    int64_t n_fit = 0, n_out = 0;
    if (MODE != kMoments)
        for (int e = threadIdx.x; e < kg * J; e += kBlock)
            cs[e] = a.coef[((size_t)li * K + k0) * J + e];

    for (int64_t t0 = rb; t0 < re; t0 += kTile) {
        const int64_t r = t0 + ray_l;
        double x = 0., y = 0., s = 0.;
        bool outside = false;
        const bool fit = r < re && select_ray(a, it, item, r, x, y, s, outside);
        double *row = M + ray_l * ldm;
        for (int j = grp; j < JP; j += kGroups)
            row[j] = !fit ? 0.0 : j < J ? basis(a.terms[j], a.tcoef, x, y, s) : j == J ? 1.0 : 0.0;
        if (MODE == kStats && grp == 0) {
            n_fit += __popcll(__ballot(fit));
            n_out += __popcll(__ballot(r < re && outside));
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kPP; ++i) {
            const int kk = grp + kGroups * i;
            if (kk >= KGP)
                break;
            double w = 0.0;
            if (fit && kk < kg) {
                const int k = k0 + kk;
                w = it.wave_scale * a.rows[((item * K + k) * 3 + 2) * a.ld + r];
                if (MODE != kMoments) {
                    const double *c = cs + kk * J;
                    double zc = 0.0;
                    for (int j = 0; j < J; ++j)
                        zc += c[j] * row[j];
                    const double res = w - zc;
                    if (MODE == kStats) {
                        const double d = w - a.mean[(size_t)li * K + k];
                        s_r2[i] += res * res;
                        s_d2[i] += d * d;
                        s_max[i] = fmax(s_max[i], res);
                        s_min[i] = fmin(s_min[i], res);
                    }
                    w = res;
                }
            }
            if (MODE != kStats)
                row[JP + kk] = w;
        }
        if (MODE != kStats) {
            __syncthreads();
            const int ar = lane >> 4, ac = lane & 15;
#pragma unroll
            for (int ks = 0; ks < kTile; ks += 4) {
                const double *mr = M + (ks + ar) * ldm;
#pragma unroll
                for (int i = 0; i < kMaxTilesPerWave; ++i) {
                    if (wave + 4 * i < ntiles)
                        acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(mr[arow[i] + ac], mr[acol[i] + ac], acc[i], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }

    if (MODE != kStats) {
        const size_t rec = (size_t)JP * JP + (size_t)JP * K;
        double *g = a.part + ((size_t)li * kMaxChunks + ch) * rec;
        double *b = g + (size_t)JP * JP;
        const int ar = lane >> 4, ac = lane & 15;
#pragma unroll
        for (int i = 0; i < kMaxTilesPerWave; ++i) {
            if (wave + 4 * i >= ntiles)
                continue;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = arow[i] + ar + 4 * q, col = acol[i] + ac;
                if (col < JP)
                    g[(size_t)row * JP + col] = acc[i][q];
                else if (col - JP < kg)
                    b[(size_t)row * K + k0 + col - JP] = acc[i][q];
            }
        }
        return;
    }

    // stats: each half-wave group reduces its planes over its 32 lanes by a fixed butterfly
#pragma unroll
    for (int i = 0; i < kPP; ++i) {
        for (int off = 16; off; off >>= 1) {
            s_r2[i] += __shfl_xor(s_r2[i], off, 32);
            s_d2[i] += __shfl_xor(s_d2[i], off, 32);
            s_max[i] = fmax(s_max[i], __shfl_xor(s_max[i], off, 32));
            s_min[i] = fmin(s_min[i], __shfl_xor(s_min[i], off, 32));
        }
        const int kk = grp + kGroups * i;
        if (ray_l == 0 && kk < kg) {
            double *o = a.spart + (((size_t)li * kMaxChunks + ch) * K + k0 + kk) * 4;
            o[0] = s_r2[i];
            o[1] = s_d2[i];
            o[2] = s_max[i];
            o[3] = s_min[i];
        }
    }
    if (blockIdx.z == 0 && tid == 0) {
        int64_t *o = a.cpart + ((size_t)li * kMaxChunks + ch) * 2;
        o[0] = n_fit;
        o[1] = n_out;
    }
}

// sums of the partial records of each item over its chunks, in chunk order: the upper triangle of
// G (moments only) and B, into sums [item][JP*JP + JP*K]
__global__ void __launch_bounds__(kBlock) zk_sum(const ItemDev *items, const double *part, int JP, int K,
                                                 int with_g, double *sums)
{
    const int li = blockIdx.y;
    const int nch = items[li].nch;
    const size_t rec = (size_t)JP * JP + (size_t)JP * K;
    const size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= rec)
        return;
    if (e < (size_t)JP * JP) {
        if (!with_g || (int)(e % JP) < (int)(e / JP))
            return;
    }
    const double *p = part + (size_t)li * kMaxChunks * rec + e;
    double v = 0.0;
    for (int c = 0; c < nch; ++c)
        v += p[(size_t)c * rec];
    sums[(size_t)li * rec + e] = v;
}

struct ItemFit {
    double n;        // fitted rays (G[J][J], exact)
    double cond;     // max / min Cholesky pivot of the equilibrated G
    int32_t fit;     // 0 / 1 / 2
    int32_t pad;
};

// One workgroup per item.  REFINE = 0: factor D G D = L L^T (D = diag(G)^-1/2, L packed by rows
// into LDS and kept in fac), then c = D L^-T L^-1 D b for every plane and mean = sum W / n.
// REFINE = 1: c += D L^-T L^-1 D (Z^T r) with the stored factor.  tmp [item][K][J] holds the
// correction while it is solved for.
__device__ __forceinline__ int tri(int i, int j) { return i * (i + 1) / 2 + j; }   // i >= j

template <int REFINE>
__global__ void __launch_bounds__(kBlock) zk_solve(const double *sums, int J, int JP, int K, double *fac,
                                                   ItemFit *fits, double *coef, double *tmp, double *mean)
{
    extern __shared__ double A[];                        // L [J(J+1)/2], then D [J]
    const int li = blockIdx.x, tid = threadIdx.x;
    const size_t rec = (size_t)JP * JP + (size_t)JP * K;
    const int nt = J * (J + 1) / 2;
    const double *G = sums + (size_t)li * rec;
    const double *B = G + (size_t)JP * JP;
    double *F = fac + (size_t)li * (nt + J);
    double *c = coef + (size_t)li * K * J;
    double *D = A + nt;
    __shared__ int bad;
    __shared__ double pmin, pmax;

    if (!REFINE) {
        const double n = G[(size_t)J * JP + J];
        for (int k = tid; k < K; k += kBlock)
            mean[(size_t)li * K + k] = n > 0 ? B[(size_t)J * K + k] / n : __builtin_nan("");
        if (tid == 0) {
            bad = n < J ? 1 : 0;
            pmin = INFINITY;
            pmax = 0.0;
        }
        __syncthreads();
        if (!bad) {
            for (int j = tid; j < J; j += kBlock) {
                const double gjj = G[(size_t)j * JP + j];
                D[j] = gjj > 0 ? 1.0 / sqrt(gjj) : 0.0;
            }
            __syncthreads();
            for (int i = 0; i < J; ++i)
                for (int j = tid; j <= i; j += kBlock)
                    A[tri(i, j)] = D[i] * G[(size_t)j * JP + i] * D[j];
            for (int k = 0; k < J; ++k) {
                __syncthreads();
                const double d = A[tri(k, k)];
                if (!(d > kMinPivot)) {                  // NaN, a zero column or dependent terms
                    if (tid == 0) {
                        bad = 2;
                        pmin = d;
                    }
                    break;
                }
                const double l = sqrt(d);
                __syncthreads();                         // every thread has read the pivot
                if (tid == 0) {
                    A[tri(k, k)] = l;
                    pmin = fmin(pmin, d);
                    pmax = fmax(pmax, d);
                }
                for (int i = k + 1 + tid; i < J; i += kBlock)
                    A[tri(i, k)] /= l;
                __syncthreads();
                const int m = J - k - 1;
                for (int e = tid; e < m * m; e += kBlock) {
                    const int i = k + 1 + e / m, j = k + 1 + e % m;
                    if (j <= i)
                        A[tri(i, j)] -= A[tri(i, k)] * A[tri(j, k)];
                }
            }
            __syncthreads();
        }
        if (tid == 0) {
            ItemFit f;
            f.n = n;
            f.fit = bad;
            f.cond = bad == 1 ? __builtin_nan("") : bad == 2 ? (pmin > 0 ? 1.0 / pmin : INFINITY) : pmax / pmin;
            f.pad = 0;
            fits[li] = f;
        }
        for (int e = tid; e < nt + J; e += kBlock)
            F[e] = bad ? 0.0 : A[e];
    } else {
        if (tid == 0)
            bad = fits[li].fit;
        __syncthreads();
        if (bad)
            return;
        for (int e = tid; e < nt + J; e += kBlock)
            A[e] = F[e];
    }
    __syncthreads();

    // per plane: y = D b; L y' = y; L^T z = y'; c = D z (or c += D z)
    for (int k = tid; k < K; k += kBlock) {
        double *ck = c + (size_t)k * J;
        if (bad) {
            for (int j = 0; j < J; ++j)
                ck[j] = __builtin_nan("");
            continue;
        }
        double *t = REFINE ? tmp + ((size_t)li * K + k) * J : ck;
        for (int j = 0; j < J; ++j) {
            double v = D[j] * B[(size_t)j * K + k];
            for (int i = 0; i < j; ++i)
                v -= A[tri(j, i)] * t[i];
            t[j] = v / A[tri(j, j)];
        }
        for (int j = J - 1; j >= 0; --j) {
            double v = t[j];
            for (int i = j + 1; i < J; ++i)
                v -= A[tri(i, j)] * t[i];
            t[j] = v / A[tri(j, j)];
        }
        for (int j = 0; j < J; ++j) {
            if (REFINE)
                ck[j] += D[j] * t[j];
            else
                ck[j] = D[j] * t[j];
        }
    }
}

// per (item, plane): the chunks' stats in order, into rox_zernike_stats; NaN coefficients where
// the fit failed
__global__ void __launch_bounds__(kBlock) zk_finish(const ItemDev *items, const ItemFit *fits, const double *spart,
                                                    const int64_t *cpart, int J, int K, int total,
                                                    rox_zernike_stats *stats)
{
    const int z = blockIdx.x * kBlock + threadIdx.x;
    if (z >= total)
        return;
    const int li = z / K, k = z % K;
    const int nch = items[li].nch;
    double r2 = 0., d2 = 0., mx = -INFINITY, mn = INFINITY;
    int64_t n = 0, nout = 0;
    for (int c = 0; c < nch; ++c) {
        const double *p = spart + (((size_t)li * kMaxChunks + c) * K + k) * 4;
        r2 += p[0];
        d2 += p[1];
        mx = fmax(mx, p[2]);
        mn = fmin(mn, p[3]);
        const int64_t *q = cpart + ((size_t)li * kMaxChunks + c) * 2;
        n += q[0];
        nout += q[1];
    }
    const ItemFit f = fits[li];
    const double nan = __builtin_nan("");
    rox_zernike_stats s;
    s.n = n;
    s.n_outside = nout;
    s.rms = n > 0 ? sqrt(d2 / (double)n) : nan;
    s.rms_residual = f.fit == 0 ? sqrt(r2 / (double)n) : nan;
    s.pv_residual = f.fit == 0 ? mx - mn : nan;
    s.cond = f.cond;
    s.fit = f.fit;
    s.reserved = 0;
    stats[z] = s;
}

// ---- host ---------------------------------------------------------------------------------------
rox::PerStream<rox::Workspace> g_zk_ws;

// (n-k)! / (k! ((n+m)/2-k)! ((n-m)/2-k)!) as an exact integer (n <= 20: 20! < 2^64), then a double
double radial_coef(int n, int m, int k)
{
    auto fact = [](int v) {
        uint64_t f = 1;
        for (int i = 2; i <= v; ++i)
            f *= (uint64_t)i;
        return f;
    };
    return (double)(fact(n - k) / (fact(k) * fact((n + m) / 2 - k) * fact((n - m) / 2 - k)));
}

}  // namespace

extern "C" int rox_focus_zernike(int32_t n_items, int32_t n_planes, const double *rows, int64_t ld,
                                 const uint8_t *status, const rox_grid *grids, const double *circle,
                                 const double *wave_scale, int32_t n_terms, const rox_zernike_term *terms,
                                 double *coef, rox_zernike_stats *stats, void *stream)
{
    static const char kE[] = "rox_focus_zernike";
    ROX_TRY(rox::check_range(kE, "n_items", n_items, 1, ROX_MAX_FOCUS_ITEMS));
    ROX_TRY(rox::check_range(kE, "n_planes", n_planes, 1, ROX_MAX_FOCUS_PLANES));
    ROX_TRY(rox::check_range(kE, "n_terms", n_terms, 1, ROX_MAX_ZERNIKE_TERMS));
    if (!rows || !status || !grids || !wave_scale || !terms)
        return rox::host_fail(ROX_E_ARG, "%s: null rows, status, grids, wave_scale or terms", kE);
    if (!coef && !stats)
        return rox::host_fail(ROX_E_ARG, "%s: null coef and stats", kE);
    for (int32_t j = 0; j < n_terms; ++j) {
        const int n = terms[j].n, m = terms[j].m;
        if (n < 0 || n > ROX_MAX_ZERNIKE_ORDER || m < -n || m > n || ((n - (m < 0 ? -m : m)) & 1))
            return rox::host_fail(ROX_E_ARG, "%s: terms[%d] (n, m) = (%d, %d): need 0 <= n <= %d, |m| <= n, n - |m| even",
                                  kE, j, n, m, ROX_MAX_ZERNIKE_ORDER);
        if (!std::isfinite(terms[j].scale))
            return rox::host_fail(ROX_E_ARG, "%s: terms[%d].scale = %g is not finite", kE, j, terms[j].scale);
    }
    for (int32_t i = 0; i < n_items; ++i) {
        const rox_grid &g = grids[i];
        if (g.kind != ROX_GRID_PRODUCT)
            return rox::host_fail(ROX_E_ARG, "%s: item %d: grid kind %d is not ROX_GRID_PRODUCT", kE, i, g.kind);
        if (g.num < 2 || (int64_t)g.num * g.num > (int64_t(1) << 28))
            return rox::host_fail(ROX_E_ARG, "%s: item %d: grid num %d outside [2, 16384]", kE, i, g.num);
        if (g.row_begin != 0 || (g.row_count != 0 && g.row_count != g.num))
            return rox::host_fail(ROX_E_ARG, "%s: item %d: partial grid (row_begin %d, row_count %d)", kE, i,
                                  g.row_begin, g.row_count);
        if (ld < (int64_t)g.num * g.num)
            return rox::host_fail(ROX_E_ARG, "%s: item %d: ld %lld below the grid's %lld rays", kE, i, (long long)ld,
                                  (long long)g.num * g.num);
        if (!std::isfinite(wave_scale[i]))
            return rox::host_fail(ROX_E_ARG, "%s: item %d: wave_scale %g is not finite", kE, i, wave_scale[i]);
        if (circle) {
            const double *c = circle + 3 * (size_t)i;
            if (!std::isfinite(c[0]) || !std::isfinite(c[1]))
                return rox::host_fail(ROX_E_ARG, "%s: item %d: circle centre (%g, %g) is not finite", kE, i, c[0], c[1]);
            if (!std::isfinite(c[2]) || !(c[2] > 0))
                return rox::host_fail(ROX_E_ARG, "%s: item %d: circle radius %g is not finite and > 0", kE, i, c[2]);
        }
    }

    hipStream_t st = (hipStream_t)stream;
    rox::Turn<> ws;
    ROX_TRY(ws.take(g_zk_ws, st, kHipWhere));

    const int J = n_terms, K = n_planes;
    const int JP = (J + 1 + 15) & ~15;
    const int ngroups = (K + kPG - 1) / kPG;

    // host tables: terms, coefficients, per-item pupil axes by repeated += (trace.py:566-570)
    std::vector<TermDev> th(J);
    std::vector<double> tc;
    for (int j = 0; j < J; ++j) {
        const int n = terms[j].n, m = terms[j].m < 0 ? -terms[j].m : terms[j].m;
        th[j].m = m;
        th[j].kind = terms[j].m == 0 ? 0 : terms[j].m > 0 ? 1 : 2;
        th[j].nc = (n - m) / 2 + 1;
        th[j].off = (int32_t)tc.size();
        for (int k = 0; k <= (n - m) / 2; ++k) {          // s^((n-m)/2 - k), highest power first
            const double v = radial_coef(n, m, k) * terms[j].scale;
            tc.push_back((k & 1) ? -v : v);
        }
    }
    int64_t axes_total = 0;
    for (int32_t i = 0; i < n_items; ++i)
        axes_total += 2 * (int64_t)grids[i].num;

    const size_t rec = (size_t)JP * JP + (size_t)JP * K;
    const size_t per_item = sizeof(ItemDev) + sizeof(double) * (kMaxChunks * rec + rec + (size_t)J * J + J + (size_t)2 * K * J + K) +
                            sizeof(ItemFit) + sizeof(double) * kMaxChunks * K * 4 + sizeof(int64_t) * kMaxChunks * 2 +
                            sizeof(rox_zernike_stats) * K + sizeof(double) * 2 * 16384;
    // (n_items <= ROX_MAX_FOCUS_ITEMS: chunk_for's grid bound never binds)
    const int32_t per_launch = (int32_t)rox::chunk_for(n_items, per_item, kScratchBytes);

    // [terms][term coefficients][axes][items] are staged and copied in one transfer
    TermDev *d_terms;
    double *d_tc, *d_axes, *d_part, *d_sums, *d_fac, *d_coef, *d_tmp, *d_mean, *d_spart;
    ItemDev *d_items;
    ItemFit *d_fits;
    int64_t *d_cpart;
    rox_zernike_stats *d_stats;
    rox::Layout L;
    L.add(d_terms, rox::up256(sizeof(TermDev) * J)).add(d_tc, rox::up256(sizeof(double) * tc.size()));
    L.add(d_axes, rox::up256(sizeof(double) * (size_t)axes_total));
    L.add(d_items, rox::up256(sizeof(ItemDev) * n_items));
    const size_t stage_bytes = L.size();
    L.add(d_part, rox::up256(sizeof(double) * kMaxChunks * rec * per_launch));
    L.add(d_sums, rox::up256(sizeof(double) * rec * per_launch));
    L.add(d_fac, rox::up256(sizeof(double) * ((size_t)J * (J + 1) / 2 + J) * per_launch));
    L.add(d_fits, rox::up256(sizeof(ItemFit) * per_launch));
    L.add(d_coef, rox::up256(sizeof(double) * (size_t)K * J * per_launch));
    L.add(d_tmp, rox::up256(sizeof(double) * (size_t)K * J * per_launch));
    L.add(d_mean, rox::up256(sizeof(double) * (size_t)K * per_launch));
    L.add(d_spart, rox::up256(sizeof(double) * kMaxChunks * K * 4 * per_launch));
    L.add(d_cpart, rox::up256(sizeof(int64_t) * kMaxChunks * 2 * per_launch));
    L.add(d_stats, rox::up256(sizeof(rox_zernike_stats) * (size_t)K * per_launch));
    HIP_TRY(ws->reserve(L.size()));
    HIP_TRY(ws->stage.acquire(stage_bytes));
    L.carve(ws->buf);

    char *h = ws->stage.h;                      // the staged regions at their device offsets
    auto host = [&](const void *d) { return h + ((const char *)d - ws->buf); };
    memcpy(host(d_terms), th.data(), sizeof(TermDev) * J);
    memcpy(host(d_tc), tc.data(), sizeof(double) * tc.size());
    double *h_axes = (double *)host(d_axes);
    ItemDev *h_items = (ItemDev *)host(d_items);
    int64_t ax_off = 0;
    for (int32_t i = 0; i < n_items; ++i) {
        const rox_grid &g = grids[i];
        double *ax = h_axes + ax_off;
        for (int d = 0; d < 2; ++d) {
            const double step = (g.stop[d] - g.start[d]) / (g.num - 1);
            double v = g.start[d];
            for (int k = 0; k < g.num; ++k) {
                ax[d * g.num + k] = v;
                v += step;
            }
        }
        ItemDev &it = h_items[i];
        it.px = d_axes + ax_off;
        it.py = it.px + g.num;
        ax_off += 2 * (int64_t)g.num;
        it.cx = circle ? circle[3 * (size_t)i] : 0.0;
        it.cy = circle ? circle[3 * (size_t)i + 1] : 0.0;
        it.radius = circle ? circle[3 * (size_t)i + 2] : 1.0;
        it.wave_scale = wave_scale[i];
        it.num = g.num;
        it.R = (int64_t)g.num * g.num;
        it.nch = (int32_t)std::max<int64_t>(1, std::min<int64_t>(kMaxChunks, (it.R + kRaysPerChunk - 1) / kRaysPerChunk));
        const int64_t span = (it.R + it.nch - 1) / it.nch;
        it.span = (span + kTile - 1) / kTile * kTile;
    }
    HIP_TRY(hipMemcpyAsync(ws->buf, h, stage_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(ws->stage.record(st));

    const bool host_dst = (coef && !rox::is_device(coef)) || (stats && !rox::is_device(stats));
    const size_t lds_pass = sizeof(double) * (kTile * (kMaxJP + kPG + 1) + (size_t)kPG * J);
    const size_t lds_solve = sizeof(double) * ((size_t)J * (J + 1) / 2 + J);
    for (int32_t i0 = 0; i0 < n_items; i0 += per_launch) {
        const int32_t nl = std::min(per_launch, n_items - i0);
        const ItemDev *items = d_items + i0;
        PassArgs a{rows, status, ld, K, i0, J, JP, items, d_terms, d_tc, d_part, d_coef, d_mean, d_spart, d_cpart};
        const dim3 grid((unsigned)kMaxChunks, (unsigned)nl, (unsigned)ngroups);
        const dim3 sgrid((unsigned)((rec + kBlock - 1) / kBlock), (unsigned)nl);
        hipLaunchKernelGGL(zk_pass<kMoments>, grid, dim3(kBlock), lds_pass, st, a);
        hipLaunchKernelGGL(zk_sum, sgrid, dim3(kBlock), 0, st, items, (const double *)d_part, JP, K, 1, d_sums);
        hipLaunchKernelGGL(zk_solve<0>, dim3((unsigned)nl), dim3(kBlock), lds_solve, st, (const double *)d_sums, J, JP,
                           K, d_fac, d_fits, d_coef, d_tmp, d_mean);
        hipLaunchKernelGGL(zk_pass<kRefine>, grid, dim3(kBlock), lds_pass, st, a);
        hipLaunchKernelGGL(zk_sum, sgrid, dim3(kBlock), 0, st, items, (const double *)d_part, JP, K, 0, d_sums);
        hipLaunchKernelGGL(zk_solve<1>, dim3((unsigned)nl), dim3(kBlock), lds_solve, st, (const double *)d_sums, J, JP,
                           K, d_fac, d_fits, d_coef, d_tmp, d_mean);
        hipLaunchKernelGGL(zk_pass<kStats>, grid, dim3(kBlock), lds_pass, st, a);
        hipLaunchKernelGGL(zk_finish, dim3((unsigned)((nl * K + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, items,
                           (const ItemFit *)d_fits, (const double *)d_spart, (const int64_t *)d_cpart, J, K, nl * K,
                           d_stats);
        HIP_TRY(hipGetLastError());
        if (coef)
            HIP_TRY(hipMemcpyAsync(coef + (size_t)i0 * K * J, d_coef, sizeof(double) * (size_t)nl * K * J,
                                   hipMemcpyDefault, st));
        if (stats)
            HIP_TRY(hipMemcpyAsync(stats + (size_t)i0 * K, d_stats, sizeof(rox_zernike_stats) * (size_t)nl * K,
                                   hipMemcpyDefault, st));
    }
    if (host_dst)
        HIP_TRY(hipStreamSynchronize(st));
    return 0;
}
