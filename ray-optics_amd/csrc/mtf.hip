// rox_focus_mtf: the line OTFs (tangential / sagittal MTF and phase) of a stack of through-focus
// PSFs, read where rox_focus_psf leaves them in HBM.
//
// A PSF is an M x M array; axis 0 is the pupil / image x direction (ray a*n + b of the grid is
// grid[a][b], a stepping pupil x), axis 1 is y, and pixel (M/2, M/2) is the plane's image point.
// With the plane's pitch p, a pixel j sits at image coordinate kSign * p * (j - M/2), and the
// line OTF of direction d at nu cycles per system unit is the DTFT of the PSF's projection:
//     LSF_x[j] = sum_l PSF[j][l],   LSF_y[l] = sum_j PSF[j][l]
//     OTF_d(nu) = sum_j LSF_d[j] exp(-2 pi i kSign nu p (j - M/2)) / sum_j LSF_d[j]
// The signs put the OTF phase in image coordinates: the reference's OPD sign and its
// fftshift(fft2(fftshift(...))) convention image a positive wavefront tilt at negative pixel
// offsets, so with kSign = -1 the PSF's centroid has the sign of the geometric spot centroid
// about the image point (tests/test_through_focus_mtf_reference.py pins this against the
// reference's own spot).
//
//   mtf_project   one 64 x 64 tile per workgroup (many workgroups per plane): each PSF element
//                 is read once; the tile's row sums and column sums go to partial records
//   mtf_lines     LSF_x and LSF_y of each plane: the partial records summed in tile order
//   mtf_dtft      one wave per (plane, direction, frequency): sincospi of the range-reduced
//                 phase, the DTFT and the normaliser reduced in the same fixed order, so that
//                 nu = 0 gives exactly (1, 0)
// No atomics: identical calls give bit-identical results.  An entry is NaN where nu p > 1/2 (above
// the PSF grid's Nyquist frequency) or where the projection's sum is not positive and finite.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "rox_host.hpp"

namespace {

constexpr char kHipWhere[] = "rox_focus_mtf: ";

constexpr int kTile = 64;               // PSF tile edge of mtf_project: one wave reads a 512-B row piece
constexpr int kBlock = 256;             // 4 waves
constexpr int kRowsPerWave = kTile / (kBlock / 64);
// image coordinate = kSign * p * (j - M/2) along x (d = 0) and y (d = 1)
constexpr double kSignX = -1.0, kSignY = -1.0;

// scratch per launch (partial records, projections, a host destination's staging) is capped;
// larger stacks run as consecutive launches with the same results
constexpr size_t kMtfScratchBytes = size_t(256) << 20;

// tile (blockIdx.x = column tile, blockIdx.y = row tile) of plane blockIdx.z of a launch.
// rowpart[z][tx][r] = sum over the tile's columns of row r, colpart[z][ty][c] likewise per column.
__global__ __launch_bounds__(kBlock) void mtf_project(const double *__restrict__ psf, int M, int nt,
                                                      double *__restrict__ rowpart, double *__restrict__ colpart)
{
    __shared__ double tile[kTile][kTile + 1];
    __shared__ double csum[kBlock / 64][kTile];
    const int64_t z = blockIdx.z;
    const double *__restrict__ p = psf + z * (int64_t)M * M;
    const int c0 = blockIdx.x * kTile, r0 = blockIdx.y * kTile;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = c0 + lane;
    // wave w reads rows w, w + 4, ... of the tile: each load is one coalesced row piece
    double v[kRowsPerWave];
#pragma unroll
    for (int i = 0; i < kRowsPerWave; ++i) {
        const int r = r0 + wave + 4 * i;
        v[i] = (r < M && c < M) ? p[(int64_t)r * M + c] : 0.0;
    }
    double col = 0.0;
#pragma unroll
    for (int i = 0; i < kRowsPerWave; ++i) {
        col += v[i];
        tile[wave + 4 * i][lane] = v[i];
    }
    csum[wave][lane] = col;
    __syncthreads();
    // row sums: four threads per row, 16 columns each, then the four in a butterfly
    const int row = threadIdx.x >> 2, q = threadIdx.x & 3;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < kTile / 4; ++k)
        s += tile[row][q * (kTile / 4) + k];
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    if (q == 0 && r0 + row < M)
        rowpart[(z * nt + blockIdx.x) * M + r0 + row] = s;
    if (threadIdx.x < kTile && c < M) {
        double t = 0.0;
        for (int w = 0; w < kBlock / 64; ++w)
            t += csum[w][threadIdx.x];
        colpart[(z * nt + blockIdx.y) * M + c] = t;
    }
}

// lsf[z][d][j]: the nt partial records of plane z, direction d (blockIdx.y) summed in tile order
__global__ __launch_bounds__(kBlock) void mtf_lines(const double *__restrict__ rowpart,
                                                    const double *__restrict__ colpart, int M, int nt,
                                                    double *__restrict__ lsf)
{
    const int j = blockIdx.x * kBlock + threadIdx.x;
    const int d = blockIdx.y;
    const int64_t z = blockIdx.z;
    if (j >= M)
        return;
    const double *__restrict__ part = (d == 0 ? rowpart : colpart) + z * nt * M + j;
    double t = 0.0;
    for (int k = 0; k < nt; ++k)
        t += part[(int64_t)k * M];
    lsf[(z * 2 + d) * M + j] = t;
}

// one wave per (plane z = blockIdx.z, direction d = blockIdx.y, frequency q): plane p0 + z of the
// call, otf[z][d][q] = (re, im)
__global__ __launch_bounds__(kBlock) void mtf_dtft(const double *__restrict__ lsf, int M, int64_t p0,
                                                   const double *__restrict__ pitch, const double *__restrict__ freqs,
                                                   int n_freq, double *__restrict__ otf)
{
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    const int d = blockIdx.y;
    const int64_t z = blockIdx.z;
    if (q >= n_freq)
        return;
    double *out = otf + ((z * 2 + d) * n_freq + q) * 2;
    const double f = freqs[q] * pitch[p0 + z];           // cycles per pixel
    if (!(f <= 0.5)) {                                   // above the PSF grid's Nyquist frequency
        if (lane == 0)
            out[0] = out[1] = __builtin_nan("");
        return;
    }
    const double *__restrict__ L = lsf + (z * 2 + d) * M;
    const int h = M / 2;
    double re = 0.0, im = 0.0, nrm = 0.0;
    for (int j = lane; j < M; j += 64) {
        const double l = L[j];
        const double t = f * (double)(j - h);
        const double r = t - rint(t);                    // exact: |r| <= 1/2
        double sn, cs;
        sincospi(2.0 * r, &sn, &cs);
        re += l * cs;                                    // at f = 0: l * 1.0, the normaliser's terms
        im += l * sn;
        nrm += l;
    }
    for (int off = 32; off; off >>= 1) {
        re += __shfl_xor(re, off);
        im += __shfl_xor(im, off);
        nrm += __shfl_xor(nrm, off);
    }
    if (lane != 0)
        return;
    if (!(nrm > 0.0 && nrm <= DBL_MAX)) {           // no light on the plane (or not finite)
        out[0] = out[1] = __builtin_nan("");
        return;
    }
    // exp(-2 pi i s t) = cos(2 pi r) - i s sin(2 pi r); + 0.0 turns a -0 into +0
    out[0] = re / nrm;
    out[1] = (-(d == 0 ? kSignX : kSignY) * im) / nrm + 0.0;
}

// workspace per (device, stream):
//   [pitch P][freqs Q][row partials][column partials][projections][host-destination staging]
rox::PerStream<rox::Workspace> g_mtf_ws;

}  // namespace

extern "C" int rox_focus_mtf(int32_t n_items, int32_t n_planes, const double *psf, int32_t maxdim,
                             const double *pitch, int32_t n_freq, const double *freqs, double *otf,
                             void *stream)
{
    static const char kE[] = "rox_focus_mtf";
    // every argument check comes before anything touches a device
    ROX_TRY(rox::check_range(kE, "n_items", n_items, 1, ROX_MAX_FOCUS_ITEMS));
    ROX_TRY(rox::check_range(kE, "n_planes", n_planes, 1, ROX_MAX_FOCUS_PLANES));
    ROX_TRY(rox::check_range(kE, "maxdim", maxdim, 2, 32768));
    ROX_TRY(rox::check_range(kE, "n_freq", n_freq, 1, ROX_MAX_MTF_FREQS));
    if (!psf || !pitch || !freqs || !otf)
        return rox::host_fail(ROX_E_ARG, "%s: null psf, pitch, freqs or otf", kE);
    const int64_t total = (int64_t)n_items * n_planes;
    ROX_TRY(rox::check_pitch(kE, total, pitch));
    for (int32_t q = 0; q < n_freq; ++q)
        if (!(std::isfinite(freqs[q]) && freqs[q] >= 0.0))
            return rox::host_fail(ROX_E_ARG, "%s: freqs[%d] = %g is not finite and >= 0", kE, q, freqs[q]);

    hipStream_t st = (hipStream_t)stream;
    rox::Turn<> ws;
    ROX_TRY(ws.take(g_mtf_ws, st, kHipWhere));

    const bool dev_dst = rox::is_device(otf);
    const int M = maxdim, Q = n_freq;
    const int nt = (M + kTile - 1) / kTile;
    const int64_t otf_el = (int64_t)2 * Q * 2;                  // doubles of one plane's result
    const size_t per_plane = sizeof(double) * ((size_t)2 * nt * M + 2 * (size_t)M + (dev_dst ? 0 : otf_el));
    const int64_t chunk = rox::chunk_for(total, per_plane, kMtfScratchBytes);
    double *d_pitch, *d_freq, *rowpart, *colpart, *lsf, *scratch_otf;
    rox::Layout L;
    L.add(d_pitch, rox::up256(sizeof(double) * (size_t)total)).add(d_freq, rox::up256(sizeof(double) * (size_t)Q));
    L.add(rowpart, rox::up256(sizeof(double) * (size_t)nt * M * chunk));
    L.add(colpart, rox::up256(sizeof(double) * (size_t)nt * M * chunk));
    L.add(lsf, rox::up256(sizeof(double) * 2 * (size_t)M * chunk));
    L.add(scratch_otf, dev_dst ? 0 : sizeof(double) * (size_t)otf_el * chunk);
    HIP_TRY(ws->reserve(L.size()));
    L.carve(ws->buf);

    // pitch and freqs -> pinned block (once the previous call's copy has read it) -> device
    HIP_TRY(ws->stage.acquire(sizeof(double) * ((size_t)total + (size_t)Q)));
    double *h_stage = (double *)ws->stage.h;
    memcpy(h_stage, pitch, sizeof(double) * (size_t)total);
    memcpy(h_stage + total, freqs, sizeof(double) * (size_t)Q);
    HIP_TRY(hipMemcpyAsync(d_pitch, h_stage, sizeof(double) * (size_t)total, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_freq, h_stage + total, sizeof(double) * (size_t)Q, hipMemcpyHostToDevice, st));
    HIP_TRY(ws->stage.record(st));

    for (int64_t p0 = 0; p0 < total; p0 += chunk) {
        const int64_t c = std::min(chunk, total - p0);
        double *dst = dev_dst ? otf + p0 * otf_el : scratch_otf;
        hipLaunchKernelGGL(mtf_project, dim3((unsigned)nt, (unsigned)nt, (unsigned)c), dim3(kBlock), 0, st,
                           psf + p0 * (int64_t)M * M, M, nt, rowpart, colpart);
        hipLaunchKernelGGL(mtf_lines, dim3((unsigned)((M + kBlock - 1) / kBlock), 2u, (unsigned)c), dim3(kBlock),
                           0, st, (const double *)rowpart, (const double *)colpart, M, nt, lsf);
        hipLaunchKernelGGL(mtf_dtft, dim3((unsigned)((Q + kBlock / 64 - 1) / (kBlock / 64)), 2u, (unsigned)c),
                           dim3(kBlock), 0, st, (const double *)lsf, M, p0, (const double *)d_pitch,
                           (const double *)d_freq, Q, dst);
        HIP_TRY(hipGetLastError());
        // a host destination: this chunk's results, copied before the next chunk reuses the staging
        if (!dev_dst)
            HIP_TRY(hipMemcpyAsync(otf + p0 * otf_el, scratch_otf, sizeof(double) * (size_t)(otf_el * c),
                                   hipMemcpyDeviceToHost, st));
    }
    if (!dev_dst)
        HIP_TRY(hipStreamSynchronize(st));
    return 0;
}
