// huygens.hip -- rox_huygens_psf (include/roxtrace.h): the Huygens point spread function on the
// detector's pixel grid, through focus.  Every OK ray is a plane wavelet a_r exp(2 pi i (phi_r +
// xi_r X + eta_r Y + zeta_r dz)); their complex sum U at the pixels (X_a, Y_b) of a product grid
// factorises,
//     exp(2 pi i (t_A(r, a) + t_B(r, b)))  =  [a_r exp(2 pi i t_A)] [exp(2 pi i t_B)],
// so U = A B^T is a complex GEMM of shape (K nx x R)(R x ny) on the fp64 matrix cores (cgemm_nt of
// rox_cgemm.hpp, the GEMM of rox_focus_psf): 8 K nx ny R flop, and R (K nx + ny) sincospi to form
// the operands, against K nx ny R sincospi of the direct sum.
//
//   huygens_operands  A [item][plane * nxp + a][r] and B [item][b][r] as real / imaginary planes
//                     with the ray index contiguous; pixel rows are padded with zeros to nxp / nyp
//                     (multiples of 64) and rays to kp (a multiple of 16); a failed ray is a zero
//                     column.  Every element of the padded planes is written, so the scratch needs
//                     no clearing.
//   cgemm_nt<0>       U = A B^T into scratch, one problem per item and slice of 8192 rays (blockIdx.z)
//   huygens_finish    one workgroup per plane: U summed over the slices in order, psf = re^2 + im^2,
//                     the field, and the statistics, every sum and the peak reduced in a fixed order.
// A launch covers whole items (all their planes) or, where one item's operands exceed the scratch
// cap, a run of planes of one item.  An output element is one MFMA accumulation chain over its own
// operand rows (rox_cgemm.hpp), so its bits do not depend on how the job was split.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "rox_cgemm.hpp"
#include "rox_host.hpp"

namespace {

constexpr char kHipWhere[] = "rox_huygens_psf: ";
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxPixels = 4096;                    // nx, ny
constexpr int kSliceRays = 8192;                    // rays of one GEMM problem

// Scratch per launch (the operands and U) is capped; larger jobs run as consecutive launches with
// the same results.  ROX_HUYGENS_SCRATCH_BYTES (read per call) lowers or raises the cap: the tests
// set it so that tiny shapes split.
constexpr size_t kHuygensScratchBytes = size_t(1) << 30;

struct Job {
    const double *rows;         // [n_items][4][ld]: phi xi eta zeta
    const double *amp;          // [n_items][ld] or null
    const uint8_t *status;      // [n_items][ld]
    const double *planes;       // device [n_items][n_planes][3] = x0 y0 dz
    int64_t ld, n_rays;
    int32_t n_planes, nx, ny, nxp, nyp, kp;
    int32_t ks, ns;             // the rays in ns slices of ks (a multiple of 16): kp = ns * ks
    double pitch_x, pitch_y;
    int32_t i0, p0, cp;         // this launch: items from i0 (blockIdx.z), planes p0 .. p0 + cp
    // [ci][ns][cp nxp][ks] x2, [ci][ns][nyp][ks] x2, [ci][ns][cp nxp][ny] x2
    double *are, *aim, *bre, *bim, *cre, *cim;
};

// (cos, sin)(2 pi t): r = t - rint(t) is exact, |r| <= 1/2
__device__ __forceinline__ void wavelet(double t, double *sn, double *cs)
{
    const double r = t - rint(t);
    sincospi(2.0 * r, sn, cs);
}

// blockIdx.x = operand row: cp * nxp rows of A, then (gridDim.x beyond them) nyp rows of B;
// blockIdx.y strides the rays; blockIdx.z = item of the launch.
__global__ __launch_bounds__(kBlock) void huygens_operands(Job j)
{
#pragma clang fp contract(off)
    const int64_t z = blockIdx.z, item = j.i0 + z;
    const int row = blockIdx.x, rows_a = j.cp * j.nxp;
    const bool is_a = row < rows_a;
    const int k = is_a ? row / j.nxp : 0, pix = is_a ? row - k * j.nxp : row - rows_a;
    const double *__restrict__ R0 = j.rows + item * 4 * j.ld;
    const uint8_t *__restrict__ st = j.status + item * j.ld;
    const double *__restrict__ am = j.amp ? j.amp + item * j.ld : nullptr;
    double x0 = 0.0, y0 = 0.0, dz = 0.0;
    if (is_a) {
        const double *pl = j.planes + (item * j.n_planes + j.p0 + k) * 3;
        x0 = pl[0], y0 = pl[1], dz = pl[2];
    }
    const bool live = pix < (is_a ? j.nx : j.ny);       // not a padding row
    const double off = is_a ? (double)pix * j.pitch_x : (double)pix * j.pitch_y;
    // ray r is element r % ks of slice r / ks; a slice holds the rows of all planes of the launch
    const int64_t rows_s = is_a ? rows_a : j.nyp, row_s = is_a ? row : pix;
    double *__restrict__ ore = (is_a ? j.are : j.bre) + z * j.ns * rows_s * j.ks;
    double *__restrict__ oim = (is_a ? j.aim : j.bim) + z * j.ns * rows_s * j.ks;
    for (int64_t r = (int64_t)blockIdx.y * kBlock + threadIdx.x; r < j.kp; r += (int64_t)gridDim.y * kBlock) {
        const int64_t sl = r / j.ks, at = (sl * rows_s + row_s) * j.ks + (r - sl * j.ks);
        double c = 0.0, s = 0.0;
        if (live && r < j.n_rays && st[r] == ROX_OK) {  // a failed ray's rows are never read
            const double eta = R0[2 * j.ld + r];
            if (is_a) {
                const double xi = R0[j.ld + r];
                double t = R0[r] + R0[3 * j.ld + r] * dz;
                t = t + xi * x0;
                t = t + eta * y0;
                t = t + xi * off;
                wavelet(t, &s, &c);
                if (am) {
                    const double a = am[r];
                    c = a * c;
                    s = a * s;
                }
            } else {
                wavelet(eta * off, &s, &c);
            }
        }
        ore[at] = c;
        oim[at] = s;
    }
}

// the pixel of an axis nearest the plane's origin: x0 + a pitch = 0
__device__ __forceinline__ int origin_pixel(double x0, double pitch, int n)
{
    const double a = rint(-x0 / pitch);
    return a < 0.0 ? 0 : a > (double)(n - 1) ? n - 1 : (int)a;
}

// blockIdx = (plane of the launch, item of the launch).  Thread t takes pixels t, t + 256, ... in
// row-major order and rays t, t + 256, ...; then a butterfly in each wave and the waves in order.
__global__ __launch_bounds__(kBlock) void huygens_finish(Job j, double *__restrict__ psf, double *__restrict__ field,
                                                         rox_huygens_stats *__restrict__ stats)
{
#pragma clang fp contract(off)
    __shared__ double red[kWaves][4];
    __shared__ long long red_at[kWaves];
    const int64_t z = blockIdx.y, item = j.i0 + z, q = blockIdx.x, gp = item * j.n_planes + j.p0 + q;
    const int64_t n_pix = (int64_t)j.nx * j.ny;
    // slice s of the plane's block of U is sl doubles after slice s - 1: summed in slice order
    const int64_t sl = (int64_t)j.cp * j.nxp * j.ny;
    const double *__restrict__ cre = j.cre + (z * j.ns * j.cp + q) * (int64_t)j.nxp * j.ny;
    const double *__restrict__ cim = j.cim + (z * j.ns * j.cp + q) * (int64_t)j.nxp * j.ny;
    auto u_at = [&](int64_t p, double &re, double &im) {
        re = cre[p], im = cim[p];
        for (int s = 1; s < j.ns; ++s) {
            re += cre[s * sl + p];
            im += cim[s * sl + p];
        }
    };
    double sum = 0.0, best = -1.0;
    long long at = -1;
    for (int64_t p = threadIdx.x; p < n_pix; p += kBlock) {
        double re, im;                                  // the first nx rows of the plane's block: [a][b] = p
        u_at(p, re, im);
        const double v = re * re + im * im;
        if (psf)
            psf[gp * n_pix + p] = v;
        if (field) {
            field[(gp * n_pix + p) * 2] = re;
            field[(gp * n_pix + p) * 2 + 1] = im;
        }
        sum += v;
        if (v > best) {
            best = v;
            at = p;
        }
    }
    if (!stats)
        return;
    const uint8_t *__restrict__ st = j.status + item * j.ld;
    const double *__restrict__ am = j.amp ? j.amp + item * j.ld : nullptr;
    double cnt = 0.0, sa = 0.0;
    for (int64_t r = threadIdx.x; r < j.n_rays; r += kBlock)
        if (st[r] == ROX_OK) {
            cnt += 1.0;
            sa += am ? am[r] : 1.0;
        }
    for (int o = 32; o; o >>= 1) {
        sum += __shfl_xor(sum, o);
        cnt += __shfl_xor(cnt, o);
        sa += __shfl_xor(sa, o);
        const double ob = __shfl_xor(best, o);
        const long long oa = __shfl_xor(at, o);
        if (ob > best || (ob == best && oa >= 0 && (at < 0 || oa < at))) {     // the first of equal peaks
            best = ob;
            at = oa;
        }
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[wave][0] = sum;
        red[wave][1] = cnt;
        red[wave][2] = sa;
        red[wave][3] = best;
        red_at[wave] = at;
    }
    __syncthreads();
    if (threadIdx.x != 0)
        return;
    sum = cnt = sa = 0.0;
    best = -1.0;
    at = -1;
    for (int w = 0; w < kWaves; ++w) {
        sum += red[w][0];
        cnt += red[w][1];
        sa += red[w][2];
        if (red[w][3] > best || (red[w][3] == best && red_at[w] >= 0 && (at < 0 || red_at[w] < at))) {
            best = red[w][3];
            at = red_at[w];
        }
    }
    const double *pl = j.planes + gp * 3;
    const int a0 = origin_pixel(pl[0], j.pitch_x, j.nx), b0 = origin_pixel(pl[1], j.pitch_y, j.ny);
    double re0, im0;
    u_at((int64_t)a0 * j.ny + b0, re0, im0);
    const double nan = __builtin_nan("");
    rox_huygens_stats s;
    s.n = (int64_t)cnt;
    const bool any = cnt > 0.0 && at >= 0;
    s.norm = any ? sa * sa : nan;
    s.sum = any ? sum : nan;
    s.peak = any ? best : nan;
    s.strehl = any ? (re0 * re0 + im0 * im0) / s.norm : nan;
    s.peak_ix = any ? (int32_t)(at / j.ny) : -1;
    s.peak_iy = any ? (int32_t)(at % j.ny) : -1;
    stats[gp] = s;
}

rox::PerStream<rox::Workspace> g_huygens_ws;

}  // namespace

extern "C" int rox_huygens_psf(int32_t n_items, int32_t n_planes, int64_t n_rays, const double *rows, int64_t ld,
                               const double *amp, const uint8_t *status, const double *planes, int32_t nx, int32_t ny,
                               double pitch_x, double pitch_y, double *psf, double *field, rox_huygens_stats *stats,
                               void *stream)
{
    static const char kE[] = "rox_huygens_psf";
    // every argument check comes before anything touches a device
    ROX_TRY(rox::check_range(kE, "n_items", n_items, 1, ROX_MAX_FOCUS_ITEMS));
    ROX_TRY(rox::check_range(kE, "n_planes", n_planes, 1, ROX_MAX_FOCUS_PLANES));
    ROX_TRY(rox::check_range(kE, "nx", nx, 1, kMaxPixels));
    ROX_TRY(rox::check_range(kE, "ny", ny, 1, kMaxPixels));
    if (ld < 1 || ld > (int64_t(1) << 28))
        return rox::host_fail(ROX_E_ARG, "%s: ld %lld outside [1, 2^28]", kE, (long long)ld);
    if (n_rays < 1 || n_rays > ld)
        return rox::host_fail(ROX_E_ARG, "%s: n_rays %lld outside [1, ld = %lld]", kE, (long long)n_rays,
                              (long long)ld);
    if (!(std::isfinite(pitch_x) && pitch_x > 0.0))
        return rox::host_fail(ROX_E_ARG, "%s: pitch_x = %g is not finite and > 0", kE, pitch_x);
    if (!(std::isfinite(pitch_y) && pitch_y > 0.0))
        return rox::host_fail(ROX_E_ARG, "%s: pitch_y = %g is not finite and > 0", kE, pitch_y);
    if (!rows || !status || !planes)
        return rox::host_fail(ROX_E_ARG, "%s: null rows, status or planes", kE);
    const int64_t total = (int64_t)n_items * n_planes;
    for (int64_t i = 0; i < 3 * total; ++i)
        if (!std::isfinite(planes[i]))
            return rox::host_fail(ROX_E_ARG, "%s: planes[%lld] = %g is not finite", kE, (long long)i, planes[i]);
    if (!psf && !field && !stats)
        return rox::host_fail(ROX_E_ARG, "%s: psf, field and stats are all null", kE);

    Job j{};
    j.rows = rows, j.amp = amp, j.status = status, j.ld = ld, j.n_rays = n_rays;
    j.n_planes = n_planes, j.nx = nx, j.ny = ny, j.pitch_x = pitch_x, j.pitch_y = pitch_y;
    j.nxp = (int32_t)round_up(nx, kTile), j.nyp = (int32_t)round_up(ny, kTile), j.kp = (int32_t)round_up(n_rays, kKBlock);
    // The rays go in slices of at most kSliceRays, each a GEMM problem of its own (blockIdx.z) whose
    // U the finish sums in slice order: a sum over 256 x 256 rays into 128 x 128 pixels is 4 to 16
    // workgroups per plane otherwise.  The slicing depends on n_rays alone, so the bits do too.
    j.ns = (int32_t)((j.kp + kSliceRays - 1) / kSliceRays);
    j.ks = (int32_t)round_up((j.kp + j.ns - 1) / j.ns, kKBlock);
    j.kp = j.ns * j.ks;
    // what a plane (its rows of A and of U) and an item (its B) take of the scratch
    const size_t b_plane = sizeof(double) * 2 * (size_t)j.nxp * ((size_t)j.kp + (size_t)j.ns * ny);
    const size_t b_item = sizeof(double) * 2 * (size_t)j.nyp * j.kp;
    const size_t cap = (size_t)std::max<long long>(1, rox::env_int("ROX_HUYGENS_SCRATCH_BYTES", (long long)kHuygensScratchBytes));
    const size_t b_whole = b_plane * n_planes + b_item;
    int64_t ci = 1, cp = n_planes;
    if (b_whole <= cap)
        ci = std::min<int64_t>(rox::chunk_for(n_items, b_whole, cap), std::max(1, 65535 / j.ns));   // grid z
    else if (b_plane + b_item <= cap)
        cp = rox::chunk_for(n_planes, b_plane, cap - b_item);
    else        // one plane's operands beside the item's B are the least a launch holds
        return rox::host_fail(ROX_E_ARG, "%s: n_rays %lld with nx %d, ny %d needs %zu bytes of scratch for one plane, "
                              "the bound is %zu", kE, (long long)n_rays, nx, ny, b_plane + b_item, cap);
    hipStream_t st = (hipStream_t)stream;
    rox::Turn<> ws;
    ROX_TRY(ws.take(g_huygens_ws, st, kHipWhere));

    const size_t a_el = (size_t)ci * cp * j.nxp * j.kp, b_el = (size_t)ci * j.nyp * j.kp;
    const size_t c_el = (size_t)ci * j.ns * cp * j.nxp * ny;
    const size_t b_tab = sizeof(double) * 3 * (size_t)total;
    double *d_planes, *h_planes;
    rox_huygens_stats *d_stats;
    rox::Layout L;
    L.add(j.are, sizeof(double) * a_el).add(j.aim, sizeof(double) * a_el);
    L.add(j.bre, sizeof(double) * b_el).add(j.bim, sizeof(double) * b_el);
    L.add(j.cre, sizeof(double) * c_el).add(j.cim, rox::up256(sizeof(double) * c_el));
    L.add(d_planes, rox::up256(b_tab)).add(d_stats, rox::up256(sizeof(rox_huygens_stats) * (size_t)total));
    ROX_TRY(ws.carve(L, b_tab, &h_planes));
    memcpy(h_planes, planes, b_tab);
    ROX_TRY(ws.upload(d_planes, b_tab));
    j.planes = d_planes;

    const bool dev_dst = stats && rox::is_device(stats);
    rox_huygens_stats *out_stats = !stats ? nullptr : dev_dst ? stats : d_stats;
    const unsigned ray_blocks = (unsigned)std::min<int64_t>((j.kp + kBlock - 1) / kBlock, 1024);
    for (int64_t i0 = 0; i0 < n_items; i0 += ci)
        for (int64_t p0 = 0; p0 < n_planes; p0 += cp) {
            const int64_t ni = std::min<int64_t>(ci, n_items - i0), np = std::min<int64_t>(cp, n_planes - p0);
            j.i0 = (int32_t)i0, j.p0 = (int32_t)p0, j.cp = (int32_t)np;
            // an item's B is formed with its first planes and stays for its later launches
            const int64_t op_rows = np * j.nxp + (p0 == 0 ? j.nyp : 0);
            hipLaunchKernelGGL(huygens_operands, dim3((unsigned)op_rows, ray_blocks, (unsigned)ni), dim3(kBlock), 0,
                               st, j);
            const int64_t I = np * j.nxp;
            // 64 x 64 workgroup tiles once they fill the device twice over, else 32 x 32 (the same bits)
            const bool big = (I / kTile) * (j.nyp / kTile) * ni * j.ns >= 512;
            const int W = big ? kTile : 32;
            const auto gemm = big ? cgemm_nt<0, 2> : cgemm_nt<0, 1>;
            hipLaunchKernelGGL(gemm, dim3((unsigned)(j.nyp / W), (unsigned)(I / W), (unsigned)(ni * j.ns)), dim3(256),
                               0, st, (const double *)j.are, (const double *)j.aim, I * j.ks, (const double *)j.bre,
                               (const double *)j.bim, (int64_t)j.nyp * j.ks, (int)j.ks, (int)I, (int)ny, j.cre, j.cim,
                               I * ny, (int)ny, (unsigned long long *)nullptr);
            hipLaunchKernelGGL(huygens_finish, dim3((unsigned)np, (unsigned)ni), dim3(kBlock), 0, st, j, psf, field,
                               out_stats);
            HIP_TRY(hipGetLastError());
        }
    if (!stats || dev_dst)
        return 0;
    HIP_TRY(hipMemcpyAsync(stats, d_stats, sizeof(rox_huygens_stats) * (size_t)total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}
