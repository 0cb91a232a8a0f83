// gmtf.hip -- rox_focus_gmtf: the geometric OTF and the line spread function of every plane of a
// through-focus scan, formed from the transverse ray aberrations where
// rox_trace_through_focus[_grids] leaves them in HBM.
//
// Per OK ray and direction (ex, ey): u = ex*x + ey*y, two IEEE products and one IEEE sum (the
// pragma in project; -ffp-contract=off besides).  (1, 0) and (0, 1) give exactly x and y.
//
// OTF_d(nu) = (1/n) sum_ok exp(-2 pi i nu u): per term t = nu*u (one product), r = t - rint(t)
// (exact, |r| <= 1/2), sincospi(2 r) as mtf_dtft does -- the phase convention of rox_focus_mtf.
//
//   gmtf_accumulate  blockIdx = (ray chunk, plane).  A workgroup owns kRaysPerWg consecutive rays:
//                    each thread reads the status byte, x and y of its kRaysPerThread rays once
//                    (ray = chunk base + i * 256 + thread: coalesced) and keeps them in registers
//                    for every direction and frequency.  Per (direction, frequency) a thread sums
//                    cos and sin over its rays in ray order, the wave reduces both with a fixed
//                    butterfly, the four waves meet in LDS (a tile of kFreqTile frequencies at a
//                    time) and are added in wave order: one partial record (re, im)[D][Q] and one
//                    ray count per workgroup.
//   gmtf_finish      sums the records of a plane in chunk order, negates im, divides by n.
//   gmtf_lsf         blockIdx = (ray slice, direction, plane): the (plane, direction)'s edges in
//                    LDS, bin_of decides as numpy.histogram does, a wave merges equal bins before
//                    one LDS integer atomic, and the workgroup adds its non-empty bins to the
//                    plane's 64-bit counts with global integer atomics (exact in any order).
// No floating-point atomics: identical calls give bit-identical results.  cos(0) = 1 and sin(0) = 0
// exactly, so nu = 0 sums to n and gives exactly (1, 0).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "rox_bins.hpp"
#include "rox_host.hpp"

namespace {

constexpr char kHipWhere[] = "rox_focus_gmtf: ";

constexpr int kBlock = 256;                       // 4 waves
constexpr int kWaves = kBlock / 64;
// 8 rays per thread: x, y and the projected u take 48 VGPRs, and the butterfly, the LDS step and
// the partial record (16 B per (direction, frequency) and workgroup) are paid once per 2048 sincos
constexpr int kRaysPerThread = 8;
constexpr int kRaysPerWg = kBlock * kRaysPerThread;
constexpr int kFreqTile = 64;                     // frequencies between two workgroup barriers
constexpr int kMaxLsfWg = 64;                     // workgroups per (plane, direction) of gmtf_lsf
constexpr int kLsfRaysPerWg = kBlock * 16;

// scratch per launch (partial records, per-chunk inputs and outputs) is capped: larger jobs run
// as consecutive launches over planes, and over frequencies where one plane's records of every
// frequency would not fit, with the same results
constexpr size_t kGmtfScratchBytes = size_t(128) << 20;

struct RowArgs {
    const double *rows;        // [n_items][n_planes][3][ld]
    const uint8_t *status;     // [n_items][ld]
    int64_t ld;
    int64_t n_rays;
    int32_t n_planes;
    int64_t z0;                // first plane (item * n_planes + k) of this launch
};

__device__ __forceinline__ double project(double ex, double ey, double x, double y)
{
#pragma clang fp contract(off)
    const double px = ex * x;
    const double py = ey * y;
    return px + py;
}

// (cos, sin)(2 pi nu u)
__device__ __forceinline__ void phase_term(double nu, double u, double *sn, double *cs)
{
#pragma clang fp contract(off)
    const double t = nu * u;
    const double r = t - rint(t);                        // exact: |r| <= 1/2
    sincospi(2.0 * r, sn, cs);
}

// part[zl][wg][d][q][2] = (sum cos, sum sin) over the workgroup's OK rays at freqs[0..nq);
// cnt[zl][wg] = its OK rays
__global__ __launch_bounds__(kBlock) void gmtf_accumulate(RowArgs a, const double *__restrict__ dirs, int nd,
                                                          const double *__restrict__ freqs, int nq,
                                                          double *__restrict__ part, uint32_t *__restrict__ cnt)
{
    __shared__ double red[kWaves][kFreqTile][2];
    __shared__ uint32_t wcnt[kWaves];
    const int64_t zl = blockIdx.y, z = a.z0 + zl;
    const int64_t item = z / a.n_planes;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double *__restrict__ X = a.rows + z * 3 * a.ld;
    const double *__restrict__ Y = X + a.ld;
    const uint8_t *__restrict__ st = a.status + item * a.ld;
    const int64_t base = (int64_t)blockIdx.x * kRaysPerWg + threadIdx.x;
    double x[kRaysPerThread], y[kRaysPerThread], u[kRaysPerThread];
    unsigned ok = 0;
#pragma unroll
    for (int i = 0; i < kRaysPerThread; ++i) {
        const int64_t r = base + (int64_t)i * kBlock;
        x[i] = y[i] = 0.0;
        if (r < a.n_rays && st[r] == ROX_OK) {           // a failed ray's rows are never read
            ok |= 1u << i;
            x[i] = X[r];
            y[i] = Y[r];
        }
    }
    uint32_t n = (uint32_t)__popc(ok);
    for (int o = 32; o > 0; o >>= 1)
        n += __shfl_xor(n, o);
    if (lane == 0)
        wcnt[wave] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < kWaves; ++w)
            t += wcnt[w];
        cnt[zl * gridDim.x + blockIdx.x] = t;
    }
    double *__restrict__ out = part + (zl * gridDim.x + blockIdx.x) * ((int64_t)nd * nq * 2);
    for (int d = 0; d < nd; ++d) {
        const double ex = dirs[(item * nd + d) * 2], ey = dirs[(item * nd + d) * 2 + 1];
#pragma unroll
        for (int i = 0; i < kRaysPerThread; ++i)
            u[i] = project(ex, ey, x[i], y[i]);
        for (int q0 = 0; q0 < nq; q0 += kFreqTile) {
            const int nt = min(kFreqTile, nq - q0);
            for (int j = 0; j < nt; ++j) {
                const double nu = freqs[q0 + j];
                double re = 0.0, im = 0.0;
#pragma unroll
                for (int i = 0; i < kRaysPerThread; ++i)
                    if (ok >> i & 1u) {
                        double sn, cs;
                        phase_term(nu, u[i], &sn, &cs);
                        re += cs;
                        im += sn;
                    }
                for (int o = 32; o > 0; o >>= 1) {
                    re += __shfl_xor(re, o);
                    im += __shfl_xor(im, o);
                }
                if (lane == 0) {
                    red[wave][j][0] = re;
                    red[wave][j][1] = im;
                }
            }
            __syncthreads();
            if (threadIdx.x < 2 * nt) {
                const int j = threadIdx.x >> 1, c = threadIdx.x & 1;
                double t = red[0][j][c];
                for (int w = 1; w < kWaves; ++w)
                    t += red[w][j][c];
                out[((int64_t)d * nq + q0) * 2 + threadIdx.x] = t;
            }
            __syncthreads();                             // red is reused by the next tile
        }
    }
}

// otf[zl][d][q_first + q][2] for the nq frequencies of this launch: the nwg records summed in
// chunk order, (re, -im) / n; NaN where n == 0.  n_ok[zl] = n.
__global__ __launch_bounds__(kBlock) void gmtf_finish(const double *__restrict__ part,
                                                      const uint32_t *__restrict__ cnt, int nwg, int nd, int nq,
                                                      int n_freq, int q_first, double *__restrict__ otf,
                                                      int64_t *__restrict__ n_ok)
{
    const int64_t zl = blockIdx.y;
    int64_t n = 0;
    for (int w = 0; w < nwg; ++w)
        n += cnt[zl * nwg + w];
    if (blockIdx.x == 0 && threadIdx.x == 0)
        n_ok[zl] = n;
    const int64_t rec = (int64_t)nd * nq * 2;
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= rec)
        return;
    const int d = (int)(e / (2 * nq)), rem = (int)(e % (2 * nq));
    double s = 0.0;
    for (int w = 0; w < nwg; ++w)
        s += part[(zl * nwg + w) * rec + e];
    // exp(-2 pi i t) = cos(2 pi r) - i sin(2 pi r); + 0.0 turns a -0 into +0
    const double v = (rem & 1) ? -s : s;
    otf[((zl * nd + d) * (int64_t)n_freq + q_first) * 2 + rem] = n ? v / (double)n + 0.0 : __builtin_nan("");
}

// lsf[zl][d][b] += the OK rays of this workgroup's slice whose u falls into bin b of
// edges[zl][d][0..nb]
__global__ __launch_bounds__(kBlock) void gmtf_lsf(RowArgs a, const double *__restrict__ dirs, int nd,
                                                   const double *__restrict__ edges, int nb,
                                                   unsigned long long *__restrict__ lsf)
{
    extern __shared__ double sm[];
    double *edge = sm;                                   // [nb + 1]
    uint32_t *hist = (uint32_t *)(sm + nb + 1);          // [nb]
    const int d = blockIdx.y;
    const int64_t zl = blockIdx.z, z = a.z0 + zl;
    const int64_t item = z / a.n_planes;
    const double *__restrict__ e = edges + (zl * nd + d) * (int64_t)(nb + 1);
    for (int j = threadIdx.x; j <= nb; j += kBlock)
        edge[j] = e[j];
    for (int j = threadIdx.x; j < nb; j += kBlock)
        hist[j] = 0;
    __syncthreads();
    const double *__restrict__ X = a.rows + z * 3 * a.ld;
    const double *__restrict__ Y = X + a.ld;
    const uint8_t *__restrict__ st = a.status + item * a.ld;
    const double ex = dirs[(item * nd + d) * 2], ey = dirs[(item * nd + d) * 2 + 1];
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    // every lane of a wave runs the same trip count (the merge needs the whole wave)
    for (int64_t base = (int64_t)blockIdx.x * kBlock; base < a.n_rays; base += stride) {
        const int64_t r = base + threadIdx.x;
        int b = -1;
        if (r < a.n_rays && st[r] == ROX_OK)             // a failed ray's rows are never read
            b = rox::bin_of(edge, nb, project(ex, ey, X[r], Y[r]));
        rox::wave_count(hist, b);
    }
    __syncthreads();
    unsigned long long *out = lsf + (zl * nd + d) * (int64_t)nb;
    for (int j = threadIdx.x; j < nb; j += kBlock)
        if (hist[j])
            atomicAdd(&out[j], (unsigned long long)hist[j]);
}

rox::PerStream<rox::Workspace> g_gmtf_ws;

}  // namespace

extern "C" int rox_focus_gmtf(int32_t n_items, int32_t n_planes, const double *rows, int64_t ld,
                              const uint8_t *status, int64_t n_rays, int32_t n_dir, const double *dirs,
                              int32_t n_freq, const double *freqs, double *otf, int32_t n_bins,
                              const double *edges, int64_t *lsf, int64_t *n_ok, void *stream)
{
    static const char kE[] = "rox_focus_gmtf";
    // every argument check comes before anything touches a device
    ROX_TRY(rox::check_range(kE, "n_items", n_items, 1, ROX_MAX_FOCUS_ITEMS));
    ROX_TRY(rox::check_range(kE, "n_planes", n_planes, 1, ROX_MAX_FOCUS_PLANES));
    if (!rows || !status)
        return rox::host_fail(ROX_E_ARG, "%s: null rows or status", kE);
    if (n_rays < 1 || n_rays > ld)
        return rox::host_fail(ROX_E_ARG, "%s: n_rays %lld outside [1, ld = %lld]", kE, (long long)n_rays,
                              (long long)ld);
    const int64_t nwg64 = (n_rays - 1) / kRaysPerWg + 1;
    if (nwg64 > INT_MAX)
        return rox::host_fail(ROX_E_ARG, "%s: n_rays %lld is more than one launch takes", kE, (long long)n_rays);
    ROX_TRY(rox::check_range(kE, "n_dir", n_dir, 1, ROX_MAX_GMTF_DIRS));
    ROX_TRY(rox::check_range(kE, "n_freq", n_freq, 0, ROX_MAX_MTF_FREQS));
    ROX_TRY(rox::check_range(kE, "n_bins", n_bins, 0, ROX_MAX_LSF_BINS));
    if (!otf && !lsf)
        return rox::host_fail(ROX_E_ARG, "%s: null otf and lsf", kE);
    if (!dirs)
        return rox::host_fail(ROX_E_ARG, "%s: null dirs", kE);
    if (otf && (n_freq < 1 || !freqs))
        return rox::host_fail(ROX_E_ARG, "%s: otf needs n_freq >= 1 and freqs", kE);
    if (lsf && (n_bins < 1 || !edges))
        return rox::host_fail(ROX_E_ARG, "%s: lsf needs n_bins >= 1 and edges", kE);
    const int64_t total = (int64_t)n_items * n_planes;
    const int D = n_dir, Q = otf ? n_freq : 0, B = lsf ? n_bins : 0;
    ROX_TRY(rox::check_dirs(kE, (int64_t)n_items * D, dirs));
    ROX_TRY(rox::check_freqs(kE, Q, freqs));
    if (B)
        ROX_TRY(rox::check_edges(kE, total * D, B, edges));

    hipStream_t st = (hipStream_t)stream;
    rox::Turn<> ws;
    ROX_TRY(ws.take(g_gmtf_ws, st, kHipWhere));

    const int nwg = (int)nwg64;
    // frequencies per launch: one plane's partial records take at most half the scratch
    const size_t rec1 = sizeof(double) * 2 * (size_t)nwg * D;                       // per frequency
    const int Qc = (int)std::min<size_t>((size_t)Q, std::max<size_t>(1, kGmtfScratchBytes / 2 / rec1));
    const int nlw = (int)std::max<int64_t>(1, std::min<int64_t>(kMaxLsfWg, (n_rays - 1) / kLsfRaysPerWg + 1));
    const size_t edge_el = (size_t)D * (B ? B + 1 : 0), lsf_el = (size_t)D * B, otf_el = (size_t)D * Q * 2;
    const size_t per_plane = rec1 * Qc + sizeof(uint32_t) * (size_t)nwg + sizeof(double) * (otf_el + edge_el) +
                             sizeof(int64_t) * (lsf_el + 1);
    const int64_t chunk = rox::chunk_for(total, per_plane, kGmtfScratchBytes);
    double *d_dirs, *d_freq, *part, *d_otf, *d_edges;
    uint32_t *cnt;
    unsigned long long *d_lsf;
    int64_t *d_nok;
    rox::Layout L;
    L.add(d_dirs, rox::up256(sizeof(double) * 2 * (size_t)n_items * D));
    L.add(d_freq, rox::up256(sizeof(double) * (size_t)std::max(Q, 1)));
    L.add(part, rox::up256(rec1 * Qc * chunk)).add(cnt, rox::up256(sizeof(uint32_t) * (size_t)nwg * chunk));
    L.add(d_otf, rox::up256(sizeof(double) * otf_el * chunk)).add(d_edges, rox::up256(sizeof(double) * edge_el * chunk));
    L.add(d_lsf, rox::up256(sizeof(int64_t) * lsf_el * chunk)).add(d_nok, rox::up256(sizeof(int64_t) * chunk));
    HIP_TRY(ws->reserve(L.size()));
    L.carve(ws->buf);

    // dirs and freqs -> pinned block (once the previous call's copies have read it) -> device
    const size_t n_dirs = 2 * (size_t)n_items * D;
    HIP_TRY(ws->stage.acquire(sizeof(double) * (n_dirs + (size_t)Q)));
    double *h = (double *)ws->stage.h;
    memcpy(h, dirs, sizeof(double) * n_dirs);
    if (Q)
        memcpy(h + n_dirs, freqs, sizeof(double) * (size_t)Q);
    HIP_TRY(hipMemcpyAsync(d_dirs, h, sizeof(double) * n_dirs, hipMemcpyHostToDevice, st));
    if (Q)
        HIP_TRY(hipMemcpyAsync(d_freq, h + n_dirs, sizeof(double) * (size_t)Q, hipMemcpyHostToDevice, st));
    HIP_TRY(ws->stage.record(st));

    const bool host_dst = (otf && !rox::is_device(otf)) || (lsf && !rox::is_device(lsf)) ||
                          (n_ok && !rox::is_device(n_ok));
    for (int64_t z0 = 0; z0 < total; z0 += chunk) {
        const int64_t c = std::min(chunk, total - z0);
        const RowArgs a{rows, status, ld, n_rays, n_planes, z0};
        if (otf || n_ok) {
            // (Q == 0: the ray counts alone)
            for (int q0 = 0; q0 == 0 || q0 < Q; q0 += std::max(Qc, 1)) {
                const int nq = std::min(Qc, Q - q0);
                hipLaunchKernelGGL(gmtf_accumulate, dim3((unsigned)nwg, (unsigned)c), dim3(kBlock), 0, st, a,
                                   (const double *)d_dirs, D, (const double *)d_freq + q0, nq, part, cnt);
                const int64_t rec = (int64_t)D * nq * 2;
                hipLaunchKernelGGL(gmtf_finish, dim3((unsigned)std::max<int64_t>(1, (rec + kBlock - 1) / kBlock), (unsigned)c),
                                   dim3(kBlock), 0, st, (const double *)part, (const uint32_t *)cnt, nwg, D, nq, Q,
                                   q0, d_otf, d_nok);
            }
        }
        if (B) {
            // this chunk's edges: through the pinned block, which the previous chunk's copy has left
            const size_t eb = sizeof(double) * edge_el * (size_t)c;
            HIP_TRY(ws->stage.acquire(eb, sizeof(double) * edge_el * (size_t)chunk));
            memcpy(ws->stage.h, edges + z0 * (int64_t)edge_el, eb);
            HIP_TRY(hipMemcpyAsync(d_edges, ws->stage.h, eb, hipMemcpyHostToDevice, st));
            HIP_TRY(ws->stage.record(st));
            HIP_TRY(hipMemsetAsync(d_lsf, 0, sizeof(int64_t) * lsf_el * (size_t)c, st));
            const size_t lds = sizeof(double) * (B + 1) + sizeof(uint32_t) * B;
            hipLaunchKernelGGL(gmtf_lsf, dim3((unsigned)nlw, (unsigned)D, (unsigned)c), dim3(kBlock), lds, st, a,
                               (const double *)d_dirs, D, (const double *)d_edges, B, d_lsf);
        }
        HIP_TRY(hipGetLastError());
        // this chunk's results, copied before the next chunk reuses the scratch
        if (otf)
            HIP_TRY(hipMemcpyAsync(otf + z0 * (int64_t)otf_el, d_otf, sizeof(double) * otf_el * (size_t)c,
                                   hipMemcpyDefault, st));
        if (lsf)
            HIP_TRY(hipMemcpyAsync(lsf + z0 * (int64_t)lsf_el, d_lsf, sizeof(int64_t) * lsf_el * (size_t)c,
                                   hipMemcpyDefault, st));
        if (n_ok)
            HIP_TRY(hipMemcpyAsync(n_ok + z0, d_nok, sizeof(int64_t) * (size_t)c, hipMemcpyDefault, st));
    }
    if (host_dst)
        HIP_TRY(hipStreamSynchronize(st));
    return 0;
}
