// ee.hip -- encircled energy through focus, next to the data it reads in HBM:
//   rox_focus_ee      the geometric spot of every plane of a through-focus scan (the rows
//                     rox_trace_through_focus[_grids] writes): exact ray counts within given radii
//                     and exact order statistics of the squared distances (EE50, EE80, ...)
//   rox_focus_psf_ee  the PSF stack rox_focus_psf writes: the fraction of each PSF's sum over the
//                     pixels whose centre lies within given radii, about a given centre or the
//                     PSF's own centroid
//
// Distances: dx = x - cx, dy = y - cy, d2 = dx*dx + dy*dy, each step one IEEE binary64 operation
// (-ffp-contract=off, and the pragma in sq_dist).  A radius r is compared as d2 <= r*r; the
// squares r*r are formed on the host.
//
// Geometric counts (ee_count, ee_count_finish): the plane's r^2 edges sit in LDS; each OK ray finds
// the first edge that holds its d2 by binary search (bin nr = outside every radius), a wave merges
// its lanes per bin before one LDS integer atomic per group, and each workgroup stores its integer
// histogram; a finishing pass per plane sums the workgroups and prefix-sums the bins.  Integer
// sums are exact in any order.
//
// Geometric quantiles (ee_select_*): a radix select on the uint64 bit pattern of d2 (non-negative
// doubles order as their bits), 8 bits per pass from the top, one target rank per fraction,
// m = clamp(ceil(f * n), 1, n).  A pass histograms the digit of the keys that match the target's
// prefix so far; ee_select_pick then fixes the digit that holds rank m.  Once a target's bucket
// holds a single key, the next pass has that key's ray store it and the target is done; ties
// (every ray on one point) run all 8 passes and end with the full key.  The rows are re-read once
// per pass; workgroups of a plane whose targets are all done return at once.
//
// Diffraction (ee_psf_moments, ee_psf_center, ee_psf_bin, ee_psf_finish): pixel (j, l) sits at
// image (X, Y) = (-p (j - M/2), -p (l - M/2)).  Each wave reads whole 64-pixel row pieces once;
// the moments pass forms per-workgroup (sum, sum (j - M/2) v, sum (l - M/2) v) records and a
// finishing pass the centroid.  The binning pass puts each pixel into the first r^2 edge holding
// its centre's d2 (plus an overflow bin): a wave sums the lanes of each bin with a fixed butterfly
// into its own LDS copy, the copies are added in wave order and stored per workgroup, and a
// finishing pass sums the workgroups in order and prefix-sums the bins.  The denominator is the
// same prefix continued over the overflow bin, so a radius covering every pixel gives exactly 1.
// No floating-point atomics anywhere: identical calls give bit-identical results.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "rox_bins.hpp"
#include "rox_host.hpp"

namespace {

constexpr char kHipWhere[] = "rox_focus_ee: ";

constexpr int kBlock = 256;                       // 4 waves
constexpr int kWaves = kBlock / 64;
constexpr int kMaxWgPerPlane = 64;                // workgroups per plane (bounds the partial records)
constexpr int kRaysPerWg = kBlock * 16;           // rays per workgroup before another is added
constexpr int kQGroup = 16;                       // fraction targets one select workgroup histograms
constexpr int kDigits = 256;                      // 8-bit radix digit
constexpr int kMaxBinsPerThread = (ROX_MAX_EE_RADII + 1 + kBlock - 1) / kBlock;

// scratch per launch (partial records, states, per-chunk inputs and outputs) is capped; larger
// jobs run as consecutive launches with the same results
constexpr size_t kEeScratchBytes = size_t(256) << 20;

enum : int32_t { kSelecting = 0, kUnique = 1, kDone = 2, kEmpty = 3 };

// one radix-select target: a fraction of one plane
struct SelState {
    uint64_t prefix;      // the digits fixed so far (bits above the current pass's digit)
    int64_t rank;         // 1-based rank of the target within the keys that match prefix
    int64_t count;        // keys that match prefix
    uint64_t key;         // the result's bit pattern (kDone)
    int32_t phase;
    int32_t pad;
};

__device__ __forceinline__ double sq_dist(double x, double y, double cx, double cy)
{
#pragma clang fp contract(off)
    const double dx = x - cx;
    const double dy = y - cy;
    return dx * dx + dy * dy;
}

// the first edge e[j] >= d2 of the non-decreasing e[0..n); n when there is none (NaN included)
__device__ __forceinline__ int first_edge(const double *e, int n, double d2)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (d2 <= e[mid])
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

using rox::wave_count;

// ---- geometric ----------------------------------------------------------------------------------
struct RayArgs {
    const double *rows;        // [n_items][n_planes][3][ld]
    const uint8_t *status;     // [n_items][ld]
    int64_t ld;
    int64_t n_rays;
    int32_t n_planes;
    int64_t z0;                // first plane (item * n_planes + k) of this launch
    const double *center;      // [chunk][2]
};

// histogram of the chunk's plane blockIdx.y over bins [0, nr]: part[zl][wg][nr + 1]
__global__ __launch_bounds__(kBlock) void ee_count(RayArgs a, const double *__restrict__ r2, int nr,
                                                   uint32_t *__restrict__ part)
{
    extern __shared__ double sm[];
    double *edge = sm;                                   // [nr]
    uint32_t *hist = (uint32_t *)(sm + nr);              // [nr + 1]
    const int64_t zl = blockIdx.y, z = a.z0 + zl;
    for (int j = threadIdx.x; j < nr; j += kBlock)
        edge[j] = r2[zl * nr + j];
    for (int j = threadIdx.x; j <= nr; j += kBlock)
        hist[j] = 0;
    __syncthreads();
    const double *__restrict__ X = a.rows + z * 3 * a.ld;
    const double *__restrict__ Y = X + a.ld;
    const uint8_t *__restrict__ st = a.status + (z / a.n_planes) * a.ld;
    const double cx = a.center[2 * zl], cy = a.center[2 * zl + 1];
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    // every lane of a wave runs the same trip count (the merge needs the whole wave)
    for (int64_t base = (int64_t)blockIdx.x * kBlock; base < a.n_rays; base += stride) {
        const int64_t r = base + threadIdx.x;
        int b = -1;
        if (r < a.n_rays && st[r] == ROX_OK)             // a failed ray's rows are never read
            b = first_edge(edge, nr, sq_dist(X[r], Y[r], cx, cy));
        wave_count(hist, b);
    }
    __syncthreads();
    uint32_t *out = part + (zl * gridDim.x + blockIdx.x) * (int64_t)(nr + 1);
    for (int j = threadIdx.x; j <= nr; j += kBlock)
        out[j] = hist[j];
}

// counts[zl][j] = rays with d2 <= r2[j]; n_ok[zl] = every OK ray (the overflow bin included)
__global__ __launch_bounds__(kBlock) void ee_count_finish(const uint32_t *__restrict__ part, int nwg, int nr,
                                                          int64_t *__restrict__ counts, int64_t *__restrict__ n_ok)
{
    __shared__ int64_t tot[kBlock];
    const int64_t zl = blockIdx.x;
    const int nbins = nr + 1;
    const int per = (nbins + kBlock - 1) / kBlock;
    const int j0 = threadIdx.x * per;
    int64_t loc[kMaxBinsPerThread];
    int64_t s = 0;
#pragma unroll
    for (int i = 0; i < kMaxBinsPerThread; ++i) {
        const int j = j0 + i;
        if (i < per && j < nbins)
            for (int w = 0; w < nwg; ++w)
                s += part[(zl * nwg + w) * (int64_t)nbins + j];
        loc[i] = s;
    }
    tot[threadIdx.x] = s;
    __syncthreads();
    for (int off = 1; off < kBlock; off <<= 1) {         // inclusive scan of the thread totals
        const int64_t v = threadIdx.x >= off ? tot[threadIdx.x - off] : 0;
        __syncthreads();
        tot[threadIdx.x] += v;
        __syncthreads();
    }
    const int64_t before = threadIdx.x ? tot[threadIdx.x - 1] : 0;
#pragma unroll
    for (int i = 0; i < kMaxBinsPerThread; ++i) {
        const int j = j0 + i;
        if (i < per && j < nr && counts)
            counts[zl * nr + j] = before + loc[i];
    }
    if (threadIdx.x == kBlock - 1)
        n_ok[zl] = tot[kBlock - 1];
}

// the target rank of every (plane, fraction) from the plane's OK ray count
__global__ __launch_bounds__(kBlock) void ee_select_init(const int64_t *__restrict__ n_ok,
                                                         const double *__restrict__ frac, int nq, int64_t chunk,
                                                         SelState *__restrict__ st)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= chunk * nq)
        return;
    const int64_t zl = t / nq;
    const int q = (int)(t % nq);
    const int64_t n = n_ok[zl];
    SelState s;
    s.prefix = 0;
    s.key = 0;
    s.pad = 0;
    s.count = n;
    if (n == 0) {
        s.rank = 0;
        s.phase = kEmpty;
    } else {
        const double m = ceil(frac[q] * (double)n);      // one IEEE product, then ceil
        s.rank = m < 1.0 ? 1 : (m > (double)n ? n : (int64_t)m);
        s.phase = n == 1 ? kUnique : kSelecting;
    }
    st[t] = s;
}

// one radix pass at digit (key >> shift) & 255 over the targets of group blockIdx.z:
// part[zl][wg][q][256]
__global__ __launch_bounds__(kBlock) void ee_select_hist(RayArgs a, SelState *__restrict__ st, int nq, int shift,
                                                         uint32_t *__restrict__ part)
{
    __shared__ uint32_t hist[kQGroup][kDigits];
    __shared__ uint64_t pre[kQGroup];
    __shared__ int32_t phase[kQGroup];
    __shared__ int32_t live;
    const int64_t zl = blockIdx.y, z = a.z0 + zl;
    const int q0 = blockIdx.z * kQGroup;
    const int nql = min(kQGroup, nq - q0);
    if (threadIdx.x == 0)
        live = 0;
    for (int i = threadIdx.x; i < kQGroup * kDigits; i += kBlock)
        hist[i / kDigits][i % kDigits] = 0;
    __syncthreads();
    if (threadIdx.x < nql) {
        const SelState s = st[zl * nq + q0 + threadIdx.x];
        pre[threadIdx.x] = s.prefix;
        phase[threadIdx.x] = s.phase;
        if (s.phase == kSelecting || s.phase == kUnique)
            atomicOr(&live, 1);
    }
    __syncthreads();
    if (!live)
        return;                                          // every target of the group is settled
    const uint64_t hi = shift >= 56 ? 0 : ~uint64_t(0) << (shift + 8);
    const double *__restrict__ X = a.rows + z * 3 * a.ld;
    const double *__restrict__ Y = X + a.ld;
    const uint8_t *__restrict__ stat = a.status + (z / a.n_planes) * a.ld;
    const double cx = a.center[2 * zl], cy = a.center[2 * zl + 1];
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t base = (int64_t)blockIdx.x * kBlock; base < a.n_rays; base += stride) {
        const int64_t r = base + threadIdx.x;
        const bool ok = r < a.n_rays && stat[r] == ROX_OK;
        uint64_t key = 0;
        if (ok)
            key = (uint64_t)__double_as_longlong(sq_dist(X[r], Y[r], cx, cy));
        for (int q = 0; q < nql; ++q) {
            const int ph = phase[q];
            if (ph != kSelecting && ph != kUnique)
                continue;
            const bool match = ok && (key & hi) == pre[q];
            if (ph == kUnique) {
                if (match)                               // the bucket's one key, from one lane
                    st[zl * nq + q0 + q].key = key;
                continue;
            }
            wave_count(hist[q], match ? (int)((key >> shift) & (kDigits - 1)) : -1);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nql * kDigits; i += kBlock) {
        const int q = i / kDigits;
        if (phase[q] == kSelecting)
            part[((zl * gridDim.x + blockIdx.x) * nq + q0 + q) * (int64_t)kDigits + i % kDigits] = hist[q][i % kDigits];
    }
}

// fixes the digit of every selecting target of plane blockIdx.x (one thread per digit)
__global__ __launch_bounds__(kDigits) void ee_select_pick(SelState *__restrict__ st,
                                                          const uint32_t *__restrict__ part, int nwg, int nq,
                                                          int shift)
{
    __shared__ int64_t cum[kDigits];
    const int64_t zl = blockIdx.x;
    const int d = threadIdx.x;
    for (int q = 0; q < nq; ++q) {
        SelState *s = st + zl * nq + q;
        const int ph = s->phase;                         // uniform: read before any thread writes
        const int64_t rank = s->rank;
        if (ph == kUnique) {
            if (d == 0)
                s->phase = kDone;                        // the hist pass stored the key
            continue;
        }
        if (ph != kSelecting)
            continue;
        int64_t h = 0;
        for (int w = 0; w < nwg; ++w)
            h += part[((zl * nwg + w) * nq + q) * (int64_t)kDigits + d];
        cum[d] = h;
        __syncthreads();
        for (int off = 1; off < kDigits; off <<= 1) {
            const int64_t v = d >= off ? cum[d - off] : 0;
            __syncthreads();
            cum[d] += v;
            __syncthreads();
        }
        const int64_t below = d ? cum[d - 1] : 0;
        if (h > 0 && below < rank && rank <= cum[d]) {   // exactly one digit holds the rank
            const uint64_t prefix = s->prefix | ((uint64_t)d << shift);
            s->prefix = prefix;
            s->rank = rank - below;
            s->count = h;
            if (shift == 0) {
                s->key = prefix;
                s->phase = kDone;
            } else if (h == 1) {
                s->phase = kUnique;
            }
        }
        __syncthreads();                                 // cum is reused by the next target
    }
}

__global__ __launch_bounds__(kBlock) void ee_select_out(const SelState *__restrict__ st, int64_t n,
                                                        double *__restrict__ radius)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= n)
        return;
    const SelState s = st[t];
    radius[t] = s.phase == kDone ? sqrt(__longlong_as_double((long long)s.key)) : __builtin_nan("");
}

// ---- diffraction --------------------------------------------------------------------------------
struct PsfArgs {
    const double *psf;          // the chunk's first plane
    int M;
    int nwg;                    // workgroups per plane
};

// rows j = global wave index + k * (nwg * 4) of the chunk's plane blockIdx.y: mom[zl][wg][3] =
// (sum v, sum (j - M/2) v, sum (l - M/2) v)
__global__ __launch_bounds__(kBlock) void ee_psf_moments(PsfArgs a, double *__restrict__ mom)
{
    __shared__ double red[kWaves][3];
    const int64_t zl = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int M = a.M, h = M / 2;
    const double *__restrict__ p = a.psf + zl * (int64_t)M * M;
    double s = 0.0, sj = 0.0, sl = 0.0;
    for (int j = blockIdx.x * kWaves + wave; j < M; j += a.nwg * kWaves) {
        const double *__restrict__ row = p + (int64_t)j * M;
        double rs = 0.0;
        for (int l = lane; l < M; l += 64) {
            const double v = row[l];
            rs += v;
            sl += (double)(l - h) * v;
        }
        s += rs;
        sj += (double)(j - h) * rs;
    }
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o);
        sj += __shfl_xor(sj, o);
        sl += __shfl_xor(sl, o);
    }
    if (lane == 0) {
        red[wave][0] = s;
        red[wave][1] = sj;
        red[wave][2] = sl;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double t = 0.0;
        for (int w = 0; w < kWaves; ++w)
            t += red[w][threadIdx.x];
        mom[(zl * a.nwg + blockIdx.x) * 3 + threadIdx.x] = t;
    }
}

// the centroid of every plane of the chunk; the centre used: given (given != 0) or the centroid
__global__ __launch_bounds__(kBlock) void ee_psf_center(const double *__restrict__ mom, int nwg, int64_t chunk,
                                                        const double *__restrict__ pitch, int given,
                                                        double *__restrict__ centroid, double *__restrict__ center)
{
    const int64_t zl = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (zl >= chunk)
        return;
    double s = 0.0, sj = 0.0, sl = 0.0;
    for (int w = 0; w < nwg; ++w) {
        const double *m = mom + (zl * nwg + w) * 3;
        s += m[0];
        sj += m[1];
        sl += m[2];
    }
    const double p = pitch[zl];
    double cx = __builtin_nan(""), cy = cx;
    if (s > 0.0 && s <= DBL_MAX) {
        cx = -p * (sj / s);
        cy = -p * (sl / s);
    }
    centroid[2 * zl] = cx;
    centroid[2 * zl + 1] = cy;
    if (!given) {
        center[2 * zl] = cx;
        center[2 * zl + 1] = cy;
    }
}

// part[zl][wg][nr + 1]: the PSF summed per bin of pixel-centre d2 over this workgroup's rows
__global__ __launch_bounds__(kBlock) void ee_psf_bin(PsfArgs a, const double *__restrict__ r2, int nr,
                                                     const double *__restrict__ pitch,
                                                     const double *__restrict__ center, double *__restrict__ part)
{
    extern __shared__ double sm[];
    double *edge = sm;                                   // [nr]
    double *wb = sm + nr;                                // [kWaves][nr + 1]
    const int64_t zl = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nbins = nr + 1;
    for (int j = threadIdx.x; j < nr; j += kBlock)
        edge[j] = r2[zl * nr + j];
    for (int j = threadIdx.x; j < kWaves * nbins; j += kBlock)
        wb[j] = 0.0;
    __syncthreads();
    const int M = a.M, h = M / 2;
    const double p = pitch[zl], cx = center[2 * zl], cy = center[2 * zl + 1];
    const double *__restrict__ psf = a.psf + zl * (int64_t)M * M;
    double *mine = wb + wave * nbins;
    for (int j = blockIdx.x * kWaves + wave; j < M; j += a.nwg * kWaves) {
        const double *__restrict__ row = psf + (int64_t)j * M;
        const double dx = -(p * (double)(j - h)) - cx;
        for (int l0 = 0; l0 < M; l0 += 64) {
            const int l = l0 + lane;
            double v = 0.0;
            int b = -1;
            if (l < M) {
                v = row[l];
                const double dy = -(p * (double)(l - h)) - cy;
                b = first_edge(edge, nr, sq_dist(dx, dy, 0.0, 0.0));
            }
            // each bin's lanes summed by a fixed butterfly; lane 0 adds the sum to the wave's copy
            uint64_t todo = __ballot(b >= 0);
            while (todo) {
                const int bl = __shfl(b, __builtin_ctzll(todo));
                const bool same = b == bl;
                double t = same ? v : 0.0;
                for (int o = 32; o > 0; o >>= 1)
                    t += __shfl_xor(t, o);
                if (lane == 0)
                    mine[bl] += t;
                todo &= ~__ballot(same);
            }
        }
    }
    __syncthreads();
    double *out = part + (zl * a.nwg + blockIdx.x) * (int64_t)nbins;
    for (int j = threadIdx.x; j < nbins; j += kBlock) {
        double t = wb[j];
        for (int w = 1; w < kWaves; ++w)
            t += wb[w * nbins + j];
        out[j] = t;
    }
}

// ee[zl][j] = prefix_j / prefix_nr over the bins summed in workgroup order
__global__ __launch_bounds__(kBlock) void ee_psf_finish(const double *__restrict__ part, int nwg, int nr,
                                                        double *__restrict__ ee)
{
    __shared__ double off[kBlock + 1];
    const int64_t zl = blockIdx.x;
    const int nbins = nr + 1;
    const int per = (nbins + kBlock - 1) / kBlock;
    const int j0 = threadIdx.x * per;
    double loc[kMaxBinsPerThread];
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < kMaxBinsPerThread; ++i) {
        const int j = j0 + i;
        if (i < per && j < nbins) {
            double b = 0.0;
            for (int w = 0; w < nwg; ++w)
                b += part[(zl * nwg + w) * (int64_t)nbins + j];
            s = i == 0 ? b : s + b;
        }
        loc[i] = s;
    }
    off[threadIdx.x + 1] = s;
    __syncthreads();
    if (threadIdx.x == 0) {                              // one fixed order: off[t + 1] = off[t] + tot[t]
        off[0] = 0.0;
        for (int t = 0; t < kBlock; ++t)
            off[t + 1] = off[t] + off[t + 1];
    }
    __syncthreads();
    const double den = off[kBlock];
    const bool lit = den > 0.0 && den <= DBL_MAX;
#pragma unroll
    for (int i = 0; i < kMaxBinsPerThread; ++i) {
        const int j = j0 + i;
        if (i < per && j < nr)
            ee[zl * nr + j] = lit ? (off[threadIdx.x] + loc[i]) / den : __builtin_nan("");
    }
}

// ---- host ---------------------------------------------------------------------------------------
rox::PerStream<rox::Workspace> g_ee_ws;         // (both entries)

int wgs_for(int64_t work, int64_t per_wg)
{
    return (int)std::max<int64_t>(1, std::min<int64_t>(kMaxWgPerPlane, (work + per_wg - 1) / per_wg));
}

}  // namespace

extern "C" int rox_focus_ee(int32_t n_items, int32_t n_planes, const double *rows, int64_t ld,
                            const uint8_t *status, int64_t n_rays, const double *centers, int32_t n_radii,
                            const double *radii, int64_t *counts, int32_t n_frac, const double *fractions,
                            double *ee_radius, int64_t *n_ok, void *stream)
{
    static const char kE[] = "rox_focus_ee";
    // every argument check comes before anything touches a device
    ROX_TRY(rox::check_range(kE, "n_items", n_items, 1, ROX_MAX_FOCUS_ITEMS));
    ROX_TRY(rox::check_range(kE, "n_planes", n_planes, 1, ROX_MAX_FOCUS_PLANES));
    if (!rows || !status)
        return rox::host_fail(ROX_E_ARG, "%s: null rows or status", kE);
    if (n_rays < 1 || n_rays > ld)
        return rox::host_fail(ROX_E_ARG, "%s: n_rays %lld outside [1, ld = %lld]", kE, (long long)n_rays,
                              (long long)ld);
    ROX_TRY(rox::check_range(kE, "n_radii", n_radii, 0, ROX_MAX_EE_RADII));
    ROX_TRY(rox::check_range(kE, "n_frac", n_frac, 0, ROX_MAX_EE_FRACTIONS));
    if (!counts && !ee_radius)
        return rox::host_fail(ROX_E_ARG, "%s: null counts and ee_radius", kE);
    if (counts && (n_radii < 1 || !radii))
        return rox::host_fail(ROX_E_ARG, "%s: counts needs n_radii >= 1 and radii", kE);
    if (ee_radius && (n_frac < 1 || !fractions))
        return rox::host_fail(ROX_E_ARG, "%s: ee_radius needs n_frac >= 1 and fractions", kE);
    const int64_t total = (int64_t)n_items * n_planes;
    const int nr = counts ? n_radii : 0, nq = ee_radius ? n_frac : 0;
    ROX_TRY(rox::check_radii(kE, total, nr, radii));
    for (int q = 0; q < nq; ++q)
        if (!(fractions[q] > 0.0 && fractions[q] <= 1.0))
            return rox::host_fail(ROX_E_ARG, "%s: fractions[%d] = %g outside (0, 1]", kE, q, fractions[q]);
    ROX_TRY(rox::check_centers(kE, total, centers));

    hipStream_t st = (hipStream_t)stream;
    rox::Turn<> ws;
    ROX_TRY(ws.take(g_ee_ws, st, kHipWhere));

    const int nwg = wgs_for(n_rays, kRaysPerWg);
    const int ngroups = (nq + kQGroup - 1) / kQGroup;
    const size_t per_plane = sizeof(uint32_t) * (size_t)nwg * (nr + 1) + sizeof(uint32_t) * (size_t)nwg * nq * kDigits +
                             sizeof(SelState) * nq + sizeof(double) * (nr + 2 + nq) + sizeof(int64_t) * (nr + 1);
    const int64_t chunk = rox::chunk_for(total, per_plane, kEeScratchBytes);
    double *d_frac, *d_r2, *d_cen, *d_rad;
    uint32_t *cpart, *spart;
    SelState *state;
    int64_t *d_counts, *d_nok;
    rox::Layout L;
    L.add(d_frac, rox::up256(sizeof(double) * (size_t)std::max(nq, 1)));
    L.add(d_r2, rox::up256(sizeof(double) * (size_t)nr * chunk)).add(d_cen, rox::up256(sizeof(double) * 2 * chunk));
    L.add(cpart, rox::up256(sizeof(uint32_t) * (size_t)nwg * (nr + 1) * chunk));
    L.add(spart, rox::up256(sizeof(uint32_t) * (size_t)nwg * nq * kDigits * chunk));
    L.add(state, rox::up256(sizeof(SelState) * (size_t)nq * chunk));
    L.add(d_counts, rox::up256(sizeof(int64_t) * (size_t)nr * chunk)).add(d_nok, rox::up256(sizeof(int64_t) * chunk));
    L.add(d_rad, rox::up256(sizeof(double) * (size_t)nq * chunk));
    HIP_TRY(ws->reserve(L.size()));
    L.carve(ws->buf);
    // staging: [fractions nq][r^2 total * nr][centers total * 2], read by every chunk's uploads
    HIP_TRY(ws->stage.acquire(sizeof(double) * ((size_t)nq + (size_t)total * nr + 2 * (size_t)total)));

    double *h_frac = (double *)ws->stage.h, *h_r2 = h_frac + nq, *h_cen = h_r2 + (size_t)total * nr;
    for (int q = 0; q < nq; ++q)
        h_frac[q] = fractions[q];
    for (int64_t i = 0; i < total * nr; ++i)
        h_r2[i] = radii[i] * radii[i];                   // one IEEE product
    for (int64_t i = 0; i < 2 * total; ++i)
        h_cen[i] = centers ? centers[i] : 0.0;
    if (nq)
        HIP_TRY(hipMemcpyAsync(d_frac, h_frac, sizeof(double) * nq, hipMemcpyHostToDevice, st));

    const bool host_dst = (counts && !rox::is_device(counts)) || (ee_radius && !rox::is_device(ee_radius)) ||
                          (n_ok && !rox::is_device(n_ok));
    for (int64_t z0 = 0; z0 < total; z0 += chunk) {
        const int64_t c = std::min(chunk, total - z0);
        if (nr)
            HIP_TRY(hipMemcpyAsync(d_r2, h_r2 + z0 * nr, sizeof(double) * nr * c, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_cen, h_cen + 2 * z0, sizeof(double) * 2 * c, hipMemcpyHostToDevice, st));
        RayArgs a{rows, status, ld, n_rays, n_planes, z0, d_cen};
        const size_t lds = sizeof(double) * nr + sizeof(uint32_t) * (nr + 1);
        hipLaunchKernelGGL(ee_count, dim3((unsigned)nwg, (unsigned)c), dim3(kBlock), lds, st, a,
                           (const double *)d_r2, nr, cpart);
        hipLaunchKernelGGL(ee_count_finish, dim3((unsigned)c), dim3(kBlock), 0, st, (const uint32_t *)cpart, nwg, nr,
                           nr ? d_counts : nullptr, d_nok);
        if (nq) {
            const int64_t n_t = c * nq;
            hipLaunchKernelGGL(ee_select_init, dim3((unsigned)((n_t + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                               (const int64_t *)d_nok, (const double *)d_frac, nq, c, state);
            for (int shift = 56; shift >= 0; shift -= 8) {
                hipLaunchKernelGGL(ee_select_hist, dim3((unsigned)nwg, (unsigned)c, (unsigned)ngroups), dim3(kBlock),
                                   0, st, a, state, nq, shift, spart);
                hipLaunchKernelGGL(ee_select_pick, dim3((unsigned)c), dim3(kDigits), 0, st, state,
                                   (const uint32_t *)spart, nwg, nq, shift);
            }
            hipLaunchKernelGGL(ee_select_out, dim3((unsigned)((n_t + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                               (const SelState *)state, n_t, d_rad);
        }
        HIP_TRY(hipGetLastError());
        // this chunk's results, copied before the next chunk reuses the scratch
        if (counts)
            HIP_TRY(hipMemcpyAsync(counts + z0 * nr, d_counts, sizeof(int64_t) * nr * c, hipMemcpyDefault, st));
        if (ee_radius)
            HIP_TRY(hipMemcpyAsync(ee_radius + z0 * nq, d_rad, sizeof(double) * nq * c, hipMemcpyDefault, st));
        if (n_ok)
            HIP_TRY(hipMemcpyAsync(n_ok + z0, d_nok, sizeof(int64_t) * c, hipMemcpyDefault, st));
    }
    HIP_TRY(ws->stage.record(st));
    if (host_dst)
        HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

extern "C" int rox_focus_psf_ee(int32_t n_items, int32_t n_planes, const double *psf, int32_t maxdim,
                                const double *pitch, const double *centers, int32_t n_radii, const double *radii,
                                double *ee, double *centroid, void *stream)
{
    static const char kE[] = "rox_focus_psf_ee";
    ROX_TRY(rox::check_range(kE, "n_items", n_items, 1, ROX_MAX_FOCUS_ITEMS));
    ROX_TRY(rox::check_range(kE, "n_planes", n_planes, 1, ROX_MAX_FOCUS_PLANES));
    ROX_TRY(rox::check_range(kE, "maxdim", maxdim, 2, 32768));
    ROX_TRY(rox::check_range(kE, "n_radii", n_radii, 1, ROX_MAX_EE_RADII));
    if (!psf || !pitch || !radii || !ee)
        return rox::host_fail(ROX_E_ARG, "%s: null psf, pitch, radii or ee", kE);
    const int64_t total = (int64_t)n_items * n_planes;
    ROX_TRY(rox::check_pitch(kE, total, pitch));
    ROX_TRY(rox::check_radii(kE, total, n_radii, radii));
    ROX_TRY(rox::check_centers(kE, total, centers));

    hipStream_t st = (hipStream_t)stream;
    rox::Turn<> ws;
    ROX_TRY(ws.take(g_ee_ws, st, kHipWhere));

    const int M = maxdim, nr = n_radii;
    const int nwg = wgs_for(M, 4 * kWaves);              // at least 4 rows per wave
    const size_t per_plane = sizeof(double) * ((size_t)nwg * (nr + 1) + (size_t)nwg * 3 + 2 * (size_t)nr + 6);
    const int64_t chunk = rox::chunk_for(total, per_plane, kEeScratchBytes);
    double *d_r2, *d_pitch, *d_center, *d_centroid, *part, *mom, *d_ee;
    rox::Layout L;
    L.add(d_r2, rox::up256(sizeof(double) * (size_t)nr * chunk)).add(d_pitch, rox::up256(sizeof(double) * chunk));
    L.add(d_center, rox::up256(sizeof(double) * 2 * chunk)).add(d_centroid, rox::up256(sizeof(double) * 2 * chunk));
    L.add(part, rox::up256(sizeof(double) * (size_t)nwg * (nr + 1) * chunk));
    L.add(mom, rox::up256(sizeof(double) * 3 * (size_t)nwg * chunk));
    L.add(d_ee, rox::up256(sizeof(double) * (size_t)nr * chunk));
    HIP_TRY(ws->reserve(L.size()));
    L.carve(ws->buf);
    // staging: [r^2 total * nr][pitch total][centers total * 2], read by every chunk's uploads
    HIP_TRY(ws->stage.acquire(sizeof(double) * ((size_t)total * nr + (size_t)total + 2 * (size_t)total)));

    double *h_r2 = (double *)ws->stage.h, *h_pitch = h_r2 + (size_t)total * nr, *h_cen = h_pitch + total;
    for (int64_t i = 0; i < total * nr; ++i)
        h_r2[i] = radii[i] * radii[i];                   // one IEEE product
    memcpy(h_pitch, pitch, sizeof(double) * (size_t)total);
    if (centers)
        memcpy(h_cen, centers, sizeof(double) * 2 * (size_t)total);

    const bool host_dst = !rox::is_device(ee) || (centroid && !rox::is_device(centroid));
    const PsfArgs base{psf, M, nwg};
    for (int64_t z0 = 0; z0 < total; z0 += chunk) {
        const int64_t c = std::min(chunk, total - z0);
        HIP_TRY(hipMemcpyAsync(d_r2, h_r2 + z0 * nr, sizeof(double) * nr * c, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_pitch, h_pitch + z0, sizeof(double) * c, hipMemcpyHostToDevice, st));
        if (centers)
            HIP_TRY(hipMemcpyAsync(d_center, h_cen + 2 * z0, sizeof(double) * 2 * c, hipMemcpyHostToDevice, st));
        PsfArgs a = base;
        a.psf = psf + z0 * (int64_t)M * M;
        hipLaunchKernelGGL(ee_psf_moments, dim3((unsigned)nwg, (unsigned)c), dim3(kBlock), 0, st, a, mom);
        hipLaunchKernelGGL(ee_psf_center, dim3((unsigned)((c + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                           (const double *)mom, nwg, c, (const double *)d_pitch, centers ? 1 : 0, d_centroid,
                           d_center);
        const size_t lds = sizeof(double) * (nr + (size_t)kWaves * (nr + 1));
        hipLaunchKernelGGL(ee_psf_bin, dim3((unsigned)nwg, (unsigned)c), dim3(kBlock), lds, st, a,
                           (const double *)d_r2, nr, (const double *)d_pitch, (const double *)d_center, part);
        hipLaunchKernelGGL(ee_psf_finish, dim3((unsigned)c), dim3(kBlock), 0, st, (const double *)part, nwg, nr,
                           d_ee);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(ee + z0 * nr, d_ee, sizeof(double) * nr * c, hipMemcpyDefault, st));
        if (centroid)
            HIP_TRY(hipMemcpyAsync(centroid + 2 * z0, d_centroid, sizeof(double) * 2 * c, hipMemcpyDefault, st));
    }
    HIP_TRY(ws->stage.record(st));
    if (host_dst)
        HIP_TRY(hipStreamSynchronize(st));
    return 0;
}
