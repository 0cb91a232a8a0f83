// rox_calc_psf: analyses.calc_psf (rayoptics/raytr/analyses.py:848-875) on the
// device.
//
// The reference embeds the ndim x ndim OPD grid (waves; NaN = no data) in the
// middle of a maxdim x maxdim zero array W, forms exp(i 2 pi W) with the
// entries that equal 1 (W == 0: padding and missing data) zeroed, and takes
//     AP = |fftshift(fft2(fftshift(phase)))|^2 / max.
// Only the central n x n block of `phase` is non-zero, so the transform is the
// pruned DFT   out = F P F^T   with P the n x n block and F the M x n slice of
// the (shifted) DFT matrix: two complex GEMMs of shapes (M x n)(n x n) and
// (M x n)(n x M).  That is GEMM-shaped fp64 work, so it runs on the matrix
// cores (v_mfma_f64_16x16x4_f64), for any M -- no power-of-two restriction --
// and costs 8 M n (n + M) flop instead of a full M x M FFT's passes over HBM.
//
//   psf_prepare   P^T (phase of the block, transposed) and F (twiddles: once per shape)
//   cgemm_nt<0>   T = F P            C[i][j] = sum_k A[i][k] B[j][k], complex
//   cgemm_nt<1>   AP = |T F^T|^2 and its maximum (epilogue)
//   psf_scale     AP / max
// rox_focus_psf runs the same steps over a batch of through-focus planes (blockIdx.y / .z =
// plane): focus_psf_prepare reads the rows and adds the Strehl partials, cgemm_nt_batch is
// cgemm_nt per plane, focus_psf_scale and focus_psf_finish close each plane.
// Up to maxdim 512 (the sizes figures use) the GEMMs take 32 x 32 workgroup tiles; the padded
// planes are zeroed and F is formed once per shape, not per call.
//
// Matrices are kept as separate real / imaginary planes, row-major with the
// reduction index contiguous and padded with zeros to a multiple of 16 (rows
// to a multiple of 64), so the GEMM loads need no guards.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "rox_host.hpp"

namespace {

constexpr char kHipWhere[] = "rox_calc_psf: ";

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int kTile = 64;           // workgroup tile (4 waves, 32 x 32 each)
constexpr int kKBlock = 16;         // reduction step of the main loop

__host__ __device__ inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

// P^T and F.  n = ndim, M = maxdim, kp = padded n.
//   block origin o = M/2 - (n/2 - 1)                       (analyses.py:861-863)
//   fftshift = roll by h = M/2 on input and output          (numpy.fft.fftshift)
//   F[u][a]  = exp(-2 pi i ((u - h) mod M) ((o + a + h) mod M) / M)
// exp(i 2 pi W) of one OPD entry with the entries that equal 1 zeroed (analyses.py:864-870)
__device__ __forceinline__ void pupil_phase(double w, double &c, double &s)
{
    if (w != w)                                     // np.nan_to_num
        w = 0.0;
    else if (w == __builtin_inf())
        w = DBL_MAX;
    else if (w == -__builtin_inf())
        w = -DBL_MAX;
    // 1j*2*np.pi*W: the imaginary part is the single product 2 pi W
    const double x = 6.283185307179586 * w;
    sincos(x, &s, &c);
    if (c == 1.0 && s == 0.0)                       // phase[i][j] == 1 -> 0 (:867-870)
        c = s = 0.0;
}

// P^T (per call) and, when `twiddles`, F (per shape: it depends on (n, M) only)
__global__ void psf_prepare(const double *opd, int n, int M, int kp, double *ptr, double *pti,
                            double *fr, double *fi, unsigned long long *maxbits, int phases, int twiddles)
{
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx == 0 && phases)
        *maxbits = 0;               // this call's maximum starts from zero (the second GEMM folds into it)
    if (phases && idx < (int64_t)n * n) {
        const int a = (int)(idx / n), b = (int)(idx % n);
        double s, c;
        pupil_phase(opd[idx], c, s);
        ptr[(int64_t)b * kp + a] = c;
        pti[(int64_t)b * kp + a] = s;
    }
    if (twiddles && idx < (int64_t)M * n) {
        const int u = (int)(idx / n), a = (int)(idx % n);
        const int h = M / 2, o = M / 2 - (n / 2 - 1);
        const int64_t uu = (u - h + M) % M, ii = (o + a + h) % M;
        const int64_t e = (uu * ii) % M;
        double s, c;
        sincospi(2.0 * (double)e / (double)M, &s, &c);
        fr[(int64_t)u * kp + a] = c;
        fi[(int64_t)u * kp + a] = -s;
    }
}

template <int EPI, int TM>      // TM x TM MFMA tiles per wave: 2 (32 x 32, large problems) or 1 (figure sizes)
__global__ __launch_bounds__(256) void cgemm_nt(const double *__restrict__ ar_, const double *__restrict__ ai_,
                                                const double *__restrict__ br_, const double *__restrict__ bi_,
                                                int kp, int I, int J, double *c0, double *c1, int ldc,
                                                unsigned long long *maxbits)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 15, g = lane >> 4;
    constexpr int WT = 16 * TM;             // rows / columns of the wave's tile; the block's is 2 WT
    const int i0 = blockIdx.y * (2 * WT) + (wave >> 1) * WT;
    const int j0 = blockIdx.x * (2 * WT) + (wave & 1) * WT;
    d4 cr[TM][TM], ci[TM][TM];
    for (int a = 0; a < TM; ++a)
        for (int b = 0; b < TM; ++b)
            cr[a][b] = ci[a][b] = d4{0., 0., 0., 0.};
    const double *pa_r = ar_ + (size_t)(i0 + r) * kp + 4 * g;
    const double *pa_i = ai_ + (size_t)(i0 + r) * kp + 4 * g;
    const double *pb_r = br_ + (size_t)(j0 + r) * kp + 4 * g;
    const double *pb_i = bi_ + (size_t)(j0 + r) * kp + 4 * g;
    const size_t t16 = (size_t)16 * kp;
    // software pipeline: the operands of k block i + 1 are in flight while the 64 MFMAs of
    // block i issue (a lone wave per SIMD has nobody else to hide the load latency behind)
    d4 xr[TM], xi[TM], yr[TM], yi[TM];
    for (int t = 0; t < TM; ++t) {
        xr[t] = *(const d4 *)(pa_r + t * t16);
        xi[t] = *(const d4 *)(pa_i + t * t16);
        yr[t] = *(const d4 *)(pb_r + t * t16);
        yi[t] = *(const d4 *)(pb_i + t * t16);
    }
    for (int k0 = 0; k0 < kp; k0 += kKBlock) {
        d4 nxr[TM], nxi[TM], nyr[TM], nyi[TM], xn[TM];
        const int kn = (k0 + kKBlock < kp) ? k0 + kKBlock : k0;     // last block: a harmless reload
        for (int t = 0; t < TM; ++t) {
            nxr[t] = *(const d4 *)(pa_r + t * t16 + kn);
            nxi[t] = *(const d4 *)(pa_i + t * t16 + kn);
            nyr[t] = *(const d4 *)(pb_r + t * t16 + kn);
            nyi[t] = *(const d4 *)(pb_i + t * t16 + kn);
            xn[t] = -xi[t];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int a = 0; a < TM; ++a)
#pragma unroll
                for (int b = 0; b < TM; ++b) {
                    cr[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(xr[a][e], yr[b][e], cr[a][b], 0, 0, 0);
                    cr[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(xn[a][e], yi[b][e], cr[a][b], 0, 0, 0);
                    ci[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(xr[a][e], yi[b][e], ci[a][b], 0, 0, 0);
                    ci[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(xi[a][e], yr[b][e], ci[a][b], 0, 0, 0);
                }
        for (int t = 0; t < TM; ++t) {
            xr[t] = nxr[t]; xi[t] = nxi[t]; yr[t] = nyr[t]; yi[t] = nyi[t];
        }
    }
    double vmax = 0.0;
    for (int a = 0; a < TM; ++a)
        for (int b = 0; b < TM; ++b)
            for (int q = 0; q < 4; ++q) {
                const int row = i0 + 16 * a + g + 4 * q, col = j0 + 16 * b + r;
                if (row >= I || col >= J)
                    continue;
                const size_t at = (size_t)row * ldc + col;
                if (EPI == 0) {
                    c0[at] = cr[a][b][q];
                    c1[at] = ci[a][b][q];
                } else {
                    const double m = hypot(cr[a][b][q], ci[a][b][q]);     // abs(z)
                    const double v = m * m;                               // ... ** 2
                    c0[at] = v;
                    vmax = fmax(vmax, v);                                 // nanmax
                }
            }
    if (EPI == 1) {
        for (int off = 32; off; off >>= 1)
            vmax = fmax(vmax, __shfl_xor(vmax, off));
        if (lane == 0)
            atomicMax(maxbits, (unsigned long long)__double_as_longlong(vmax));
    }
}

// rox_focus_psf: cgemm_nt on problem z = blockIdx.z, its operands sa / sb / sc doubles after
// problem 0's (a stride 0 shares F) and its maximum in maxbits[z].  The body is cgemm_nt's, line
// for line, so a plane of a batch is computed exactly as a single call computes it (a shared
// inline body changes the register allocation of cgemm_nt's own instances; these stay as they are).
// KEEP THE TWO BODIES IN STEP: a change to one is made to the other.  The bit-identity test of
// rox_focus_psf against rox_calc_psf (tests/test_gpu_through_focus_psf.py) is what checks it.
template <int EPI, int TM>
__global__ __launch_bounds__(256) void cgemm_nt_batch(const double *__restrict__ ar0, const double *__restrict__ ai0,
                                                      int64_t sa, const double *__restrict__ br0,
                                                      const double *__restrict__ bi0, int64_t sb, int kp, int I,
                                                      int J, double *c00, double *c10, int64_t sc, int ldc,
                                                      unsigned long long *maxbits0)
{
    const int64_t z = blockIdx.z;
    const double *__restrict__ ar_ = ar0 + z * sa, *__restrict__ ai_ = ai0 + z * sa;
    const double *__restrict__ br_ = br0 + z * sb, *__restrict__ bi_ = bi0 + z * sb;
    double *c0 = c00 + z * sc, *c1 = EPI == 0 ? c10 + z * sc : nullptr;
    unsigned long long *maxbits = maxbits0 + z;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 15, g = lane >> 4;
    constexpr int WT = 16 * TM;             // rows / columns of the wave's tile; the block's is 2 WT
    const int i0 = blockIdx.y * (2 * WT) + (wave >> 1) * WT;
    const int j0 = blockIdx.x * (2 * WT) + (wave & 1) * WT;
    d4 cr[TM][TM], ci[TM][TM];
    for (int a = 0; a < TM; ++a)
        for (int b = 0; b < TM; ++b)
            cr[a][b] = ci[a][b] = d4{0., 0., 0., 0.};
    const double *pa_r = ar_ + (size_t)(i0 + r) * kp + 4 * g;
    const double *pa_i = ai_ + (size_t)(i0 + r) * kp + 4 * g;
    const double *pb_r = br_ + (size_t)(j0 + r) * kp + 4 * g;
    const double *pb_i = bi_ + (size_t)(j0 + r) * kp + 4 * g;
    const size_t t16 = (size_t)16 * kp;
    // software pipeline: the operands of k block i + 1 are in flight while the 64 MFMAs of
    // block i issue (a lone wave per SIMD has nobody else to hide the load latency behind)
    d4 xr[TM], xi[TM], yr[TM], yi[TM];
    for (int t = 0; t < TM; ++t) {
        xr[t] = *(const d4 *)(pa_r + t * t16);
        xi[t] = *(const d4 *)(pa_i + t * t16);
        yr[t] = *(const d4 *)(pb_r + t * t16);
        yi[t] = *(const d4 *)(pb_i + t * t16);
    }
    for (int k0 = 0; k0 < kp; k0 += kKBlock) {
        d4 nxr[TM], nxi[TM], nyr[TM], nyi[TM], xn[TM];
        const int kn = (k0 + kKBlock < kp) ? k0 + kKBlock : k0;     // last block: a harmless reload
        for (int t = 0; t < TM; ++t) {
            nxr[t] = *(const d4 *)(pa_r + t * t16 + kn);
            nxi[t] = *(const d4 *)(pa_i + t * t16 + kn);
            nyr[t] = *(const d4 *)(pb_r + t * t16 + kn);
            nyi[t] = *(const d4 *)(pb_i + t * t16 + kn);
            xn[t] = -xi[t];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int a = 0; a < TM; ++a)
#pragma unroll
                for (int b = 0; b < TM; ++b) {
                    cr[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(xr[a][e], yr[b][e], cr[a][b], 0, 0, 0);
                    cr[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(xn[a][e], yi[b][e], cr[a][b], 0, 0, 0);
                    ci[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(xr[a][e], yi[b][e], ci[a][b], 0, 0, 0);
                    ci[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(xi[a][e], yr[b][e], ci[a][b], 0, 0, 0);
                }
        for (int t = 0; t < TM; ++t) {
            xr[t] = nxr[t]; xi[t] = nxi[t]; yr[t] = nyr[t]; yi[t] = nyi[t];
        }
    }
    double vmax = 0.0;
    for (int a = 0; a < TM; ++a)
        for (int b = 0; b < TM; ++b)
            for (int q = 0; q < 4; ++q) {
                const int row = i0 + 16 * a + g + 4 * q, col = j0 + 16 * b + r;
                if (row >= I || col >= J)
                    continue;
                const size_t at = (size_t)row * ldc + col;
                if (EPI == 0) {
                    c0[at] = cr[a][b][q];
                    c1[at] = ci[a][b][q];
                } else {
                    const double m = hypot(cr[a][b][q], ci[a][b][q]);     // abs(z)
                    const double v = m * m;                               // ... ** 2
                    c0[at] = v;
                    vmax = fmax(vmax, v);                                 // nanmax
                }
            }
    if (EPI == 1) {
        for (int off = 32; off; off >>= 1)
            vmax = fmax(vmax, __shfl_xor(vmax, off));
        if (lane == 0)
            atomicMax(maxbits, (unsigned long long)__double_as_longlong(vmax));
    }
}


__global__ void psf_scale(double *ap, int64_t count, const unsigned long long *maxbits)
{
    const double m = __longlong_as_double((long long)*maxbits);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count;
         i += (int64_t)gridDim.x * blockDim.x)
        ap[i] = ap[i] / m;                                                // AP / AP_max
}

// ---- rox_focus_psf ----------------------------------------------------------------------------
// Plane q = blockIdx.y of a launch is plane p0 + q of the call, item (p0 + q) / n_planes.
constexpr int kFocusBlock = 256;

// P^T of plane q from the through-focus rows (the OPD grid in waves is one product, NaN where a
// ray failed, exactly what the host hands rox_calc_psf), the Strehl partial record of this
// workgroup (ok rays, sum cos, sum sin of 2 pi W -- of the OPD, not the zeroed phase), and the
// plane's maximum reset for the second GEMM.
__global__ __launch_bounds__(kFocusBlock) void focus_psf_prepare(
    const double *__restrict__ rows, int64_t ld, const uint8_t *__restrict__ status,
    const double *__restrict__ scale, int32_t n_planes, int64_t p0, int n, int kp, int64_t plane,
    double *ptr, double *pti, double *partial, unsigned long long *maxbits)
{
    __shared__ double red[kFocusBlock / 64][3];
    const int64_t q = blockIdx.y, gp = p0 + q, item = gp / n_planes;
    const int64_t idx = (int64_t)blockIdx.x * kFocusBlock + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x == 0)
        maxbits[q] = 0;
    double cnt = 0.0, sc = 0.0, ss = 0.0;
    if (idx < (int64_t)n * n) {
        const int a = (int)(idx / n), b = (int)(idx % n);
        double w = __builtin_nan("");
        if (status[item * ld + idx] == ROX_OK) {
            w = scale[item] * rows[(gp * 3 + 2) * ld + idx];
            sincos(6.283185307179586 * w, &ss, &sc);
            cnt = 1.0;
        }
        double s, c;
        pupil_phase(w, c, s);
        ptr[q * plane + (int64_t)b * kp + a] = c;
        pti[q * plane + (int64_t)b * kp + a] = s;
    }
    // fixed-order reduction: a butterfly in each wave, then the waves in order
    for (int off = 32; off; off >>= 1) {
        cnt += __shfl_xor(cnt, off);
        sc += __shfl_xor(sc, off);
        ss += __shfl_xor(ss, off);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[wave][0] = cnt;
        red[wave][1] = sc;
        red[wave][2] = ss;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t[3] = {0.0, 0.0, 0.0};
        for (int w = 0; w < kFocusBlock / 64; ++w)
            for (int j = 0; j < 3; ++j)
                t[j] += red[w][j];
        double *rec = partial + (q * gridDim.x + blockIdx.x) * 3;
        rec[0] = t[0];
        rec[1] = t[1];
        rec[2] = t[2];
    }
}

// plane q's PSF divided by its maximum (psf_scale per plane)
__global__ void focus_psf_scale(double *ap, int64_t count, int64_t stride, const unsigned long long *maxbits)
{
    const double m = __longlong_as_double((long long)maxbits[blockIdx.y]);
    double *p = ap + (int64_t)blockIdx.y * stride;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count;
         i += (int64_t)gridDim.x * blockDim.x)
        p[i] = p[i] / m;                                                  // AP / AP_max
}

// one thread per plane: the workgroups' partial records in order -> rox_focus_psf_stats
__global__ void focus_psf_finish(const double *partial, int64_t n_rec, int32_t count,
                                 const unsigned long long *maxbits, rox_focus_psf_stats *out)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= count)
        return;
    double cnt = 0.0, sc = 0.0, ss = 0.0;
    for (int64_t r = 0; r < n_rec; ++r) {
        const double *rec = partial + ((int64_t)q * n_rec + r) * 3;
        cnt += rec[0];
        sc += rec[1];
        ss += rec[2];
    }
    rox_focus_psf_stats st;
    st.n = (int64_t)cnt;
    st.strehl = cnt > 0.0 ? (sc * sc + ss * ss) / (cnt * cnt) : __builtin_nan("");
    st.psf_peak = __longlong_as_double((long long)maxbits[q]);
    st.reserved = 0.0;
    out[q] = st;
}

// grow-only workspace per (device, stream)
struct Workspace {
    char *buf = nullptr;
    size_t cap = 0;
    int64_t zeroed_for[3] = {0, 0, 0};      // (n, M, bytes) the padded planes were last zeroed for
};
rox::PerStream<Workspace> g_ws;

}  // namespace

extern "C" int rox_calc_psf(const double *opd, int32_t ndim, int32_t maxdim, double *psf,
                            uint32_t flags, void *stream)
{
    if (!opd || !psf)
        return rox::host_fail(ROX_E_ARG, "rox_calc_psf: null argument");
    if (flags & ~(uint32_t)ROX_HOST_POINTERS)
        return rox::host_fail(ROX_E_ARG, "rox_calc_psf: unknown flag");
    // the reference's slice assignment (analyses.py:861-863) only has a matching shape
    // for an even ndim whose block fits inside the maxdim array
    if (ndim < 2 || (ndim & 1))
        return rox::host_fail(ROX_E_ARG, "rox_calc_psf: ndim must be even and >= 2");
    const int n = ndim, M = maxdim;
    const int o = M / 2 - (n / 2 - 1);
    if (M < 2 || o < 0 || o + n > M)
        return rox::host_fail(ROX_E_ARG, "rox_calc_psf: the ndim block does not fit in maxdim");
    if (M > 32768)
        return rox::host_fail(ROX_E_ARG, "rox_calc_psf: maxdim > 32768");
    hipStream_t st = (hipStream_t)stream;
    int device = 0;
    HIP_TRY(hipGetDevice(&device));
    auto *slot = g_ws.get(device, st);
    if (!slot)
        return rox::host_fail(ROX_E_NOMEM, "rox_calc_psf: out of host memory");
    // calls on one stream share the workspace: enqueue them whole, one after the other
    // (stream order then keeps their kernels apart); host-pointer calls hold it until done
    std::lock_guard<std::mutex> turn(slot->mu);
    Workspace *ws = &slot->data;

    const bool host = (flags & ROX_HOST_POINTERS) != 0;
    const int64_t kp = round_up(n, kKBlock), mp = round_up(M, kTile), np_ = round_up(n, kTile);
    const size_t pl_f = sizeof(double) * (size_t)mp * kp, pl_p = sizeof(double) * (size_t)np_ * kp;
    const size_t b_opd = host ? sizeof(double) * (size_t)n * n : 0;
    const size_t b_psf = host ? sizeof(double) * (size_t)M * M : 0;
    const size_t zeroed = 4 * pl_f + 2 * pl_p + 64;         // F, T, P^T planes + the maximum
    const size_t total = zeroed + b_opd + b_psf + 64;
    if (ws->cap < total) {
        HIP_TRY(rox::regrow(ws->buf, ws->cap, total, total));
        ws->zeroed_for[0] = ws->zeroed_for[1] = ws->zeroed_for[2] = 0;
    }
    char *p = ws->buf;
    double *fr = (double *)p;               p += pl_f;
    double *fi = (double *)p;               p += pl_f;
    double *tr = (double *)p;               p += pl_f;
    double *ti = (double *)p;               p += pl_f;
    double *ptr = (double *)p;              p += pl_p;
    double *pti = (double *)p;              p += pl_p;
    unsigned long long *maxbits = (unsigned long long *)p;  p += 64;
    double *d_opd = (double *)p;            p += (b_opd + 63) & ~size_t(63);
    double *d_psf = (double *)p;
    // The planes are zero-padded to the GEMM tiles.  Every element inside the (n, M) shape is
    // rewritten by each call and the padding is never written, so the planes need zeroing only
    // when the workspace is new or the shape changes; the twiddles F depend on the shape alone
    // and are formed then too (at figure sizes a call is little but stream operations and
    // sincospi).  Forming the phases inside the first product instead -- three launches --
    // measured slower from (64, 256) up: every block row repeats the n^2 sincos.
    const bool new_shape = ws->zeroed_for[0] != n || ws->zeroed_for[1] != M ||
                           ws->zeroed_for[2] != (int64_t)zeroed;
    if (new_shape) {
        HIP_TRY(hipMemsetAsync(ws->buf, 0, zeroed, st));
        ws->zeroed_for[0] = n; ws->zeroed_for[1] = M; ws->zeroed_for[2] = (int64_t)zeroed;
    }
    const double *src = opd;
    double *dst = psf;
    if (host) {
        HIP_TRY(hipMemcpyAsync(d_opd, opd, b_opd, hipMemcpyHostToDevice, st));
        src = d_opd;
        dst = d_psf;
    }
    const int64_t work = (int64_t)M * n;        // >= n * n
    const bool small = M <= 512;
    hipLaunchKernelGGL(psf_prepare, dim3((unsigned)(((new_shape ? work : (int64_t)n * n) + 255) / 256)), dim3(256), 0,
                       st, src, n, M, (int)kp, ptr, pti, fr, fi, maxbits, 1, new_shape ? 1 : 0);
    // T[u][b] = sum_a F[u][a] P[a][b];  AP[u][v] = |sum_b T[u][b] F[v][b]|^2.
    // 64 x 64 workgroup tiles give a (64, 256) problem 4 and 16 workgroups on 256 CUs: up to
    // maxdim 512 the 32 x 32 instance is used (one MFMA tile per wave, four times the workgroups)
    if (small) {
        hipLaunchKernelGGL((cgemm_nt<0, 1>), dim3((unsigned)(np_ / 32), (unsigned)(mp / 32)), dim3(256), 0, st,
                           fr, fi, ptr, pti, (int)kp, M, n, tr, ti, (int)kp, maxbits);
        hipLaunchKernelGGL((cgemm_nt<1, 1>), dim3((unsigned)(mp / 32), (unsigned)(mp / 32)), dim3(256), 0, st,
                           tr, ti, fr, fi, (int)kp, M, M, dst, (double *)nullptr, M, maxbits);
    } else {
        hipLaunchKernelGGL((cgemm_nt<0, 2>), dim3((unsigned)(np_ / kTile), (unsigned)(mp / kTile)), dim3(256), 0, st,
                           fr, fi, ptr, pti, (int)kp, M, n, tr, ti, (int)kp, maxbits);
        hipLaunchKernelGGL((cgemm_nt<1, 2>), dim3((unsigned)(mp / kTile), (unsigned)(mp / kTile)), dim3(256), 0, st,
                           tr, ti, fr, fi, (int)kp, M, M, dst, (double *)nullptr, M, maxbits);
    }
    hipLaunchKernelGGL(psf_scale, dim3(1024), dim3(256), 0, st, dst, (int64_t)M * M, maxbits);
    HIP_TRY(hipGetLastError());
    if (host) {
        HIP_TRY(hipMemcpyAsync(psf, d_psf, b_psf, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return 0;
}

namespace {

constexpr char kFocusWhere[] = "rox_focus_psf: ";

// scratch per launch (T and P^T of each plane, the PSF when psf is NULL) is capped; larger
// batches run as consecutive launches (as rox_trace_through_focus_grids caps its partials)
constexpr size_t kFocusPsfScratchBytes = size_t(256) << 20;

// grow-only workspace per (device, stream):
//   [F: fr fi] [plane blocks: tr ti ptr pti, one per plane of a launch] [per call: maximums,
//   partial records, statistics, wave scales, PSF scratch]
// F and the plane blocks are zero-padded to the GEMM tiles, so they sit at offsets that depend
// on the shape alone; the per-call region behind them may overwrite plane blocks a later, larger
// call then zeroes again (`clean` counts the plane blocks known to be zero-padded).
struct FocusWorkspace : rox::Workspace {
    int64_t shape[2] = {0, 0};      // (n, M) F was formed for
    int64_t clean = 0;
};
rox::PerStream<FocusWorkspace> g_focus_ws;

}  // namespace

extern "C" int rox_focus_psf(int32_t n_items, int32_t n_planes, const double *rows, int64_t ld,
                             const uint8_t *status, const double *wave_scale, int32_t ndim, int32_t maxdim,
                             double *psf, rox_focus_psf_stats *stats, void *stream)
{
    static const char kE[] = "rox_focus_psf";
    const char *const kHipWhere = kFocusWhere;
    // every argument check comes before anything touches a device
    ROX_TRY(rox::check_range(kE, "n_items", n_items, 1, ROX_MAX_FOCUS_ITEMS));
    ROX_TRY(rox::check_range(kE, "n_planes", n_planes, 1, ROX_MAX_FOCUS_PLANES));
    if (ndim < 2 || (ndim & 1))
        return rox::host_fail(ROX_E_ARG, "%s: ndim %d must be even and >= 2", kE, ndim);
    const int n = ndim, M = maxdim;
    const int o = M / 2 - (n / 2 - 1);
    if (M < 2 || o < 0 || o + n > M)
        return rox::host_fail(ROX_E_ARG, "%s: the ndim %d block does not fit in maxdim %d", kE, n, M);
    if (M > 32768)
        return rox::host_fail(ROX_E_ARG, "%s: maxdim %d > 32768", kE, M);
    if (ld < (int64_t)n * n)
        return rox::host_fail(ROX_E_ARG, "%s: ld %lld < ndim*ndim %lld", kE, (long long)ld, (long long)n * n);
    if (!rows || !status || !wave_scale)
        return rox::host_fail(ROX_E_ARG, "%s: null rows, status or wave_scale", kE);
    for (int32_t i = 0; i < n_items; ++i)
        if (!std::isfinite(wave_scale[i]))
            return rox::host_fail(ROX_E_ARG, "%s: wave_scale[%d] = %g is not finite", kE, i, wave_scale[i]);
    if (!psf && !stats)
        return rox::host_fail(ROX_E_ARG, "%s: psf and stats are both null", kE);

    hipStream_t st = (hipStream_t)stream;
    rox::PerStream<FocusWorkspace>::Slot *slot;
    ROX_TRY(g_focus_ws.take(st, kHipWhere, &slot));
    std::lock_guard<std::mutex> turn(slot->mu);
    FocusWorkspace *ws = &slot->data;

    // the shapes of rox_calc_psf, per plane
    const int64_t kp = round_up(n, kKBlock), mp = round_up(M, kTile), np_ = round_up(n, kTile);
    const int64_t f_el = mp * kp, p_el = np_ * kp;              // doubles of an F / T and a P^T plane
    const int64_t blk_el = 2 * f_el + 2 * p_el;                 // one plane block: tr ti ptr pti
    const int64_t psf_el = (int64_t)M * M;
    const int64_t nblk = ((int64_t)n * n + kFocusBlock - 1) / kFocusBlock;
    const int64_t total = (int64_t)n_items * n_planes;
    const size_t per_plane = sizeof(double) * (size_t)(blk_el + (psf ? 0 : psf_el) + 3 * nblk) + 8;
    const int64_t chunk = rox::chunk_for(total, per_plane, kFocusPsfScratchBytes);
    double *fr, *blocks, *partial, *d_scale, *scratch_psf;
    unsigned long long *maxbits;
    rox_focus_psf_stats *d_stats;
    const size_t b_f = sizeof(double) * 2 * (size_t)f_el;
    rox::Layout L;
    L.add(fr, b_f).add(blocks, sizeof(double) * (size_t)blk_el * chunk);
    L.add(maxbits, rox::up256(sizeof(unsigned long long) * chunk));
    L.add(partial, rox::up256(sizeof(double) * 3 * (size_t)nblk * chunk));
    L.add(d_stats, rox::up256(sizeof(rox_focus_psf_stats) * (size_t)total));
    L.add(d_scale, rox::up256(sizeof(double) * (size_t)n_items));
    L.add(scratch_psf, psf ? 0 : sizeof(double) * (size_t)psf_el * chunk);
    if (ws->cap < L.size()) {
        HIP_TRY(rox::regrow(ws->buf, ws->cap, L.size(), L.size()));
        ws->shape[0] = ws->shape[1] = 0;
        ws->clean = 0;
    }
    L.carve(ws->buf);
    double *fi = fr + f_el;

    // F (and zeroed plane blocks) for this shape; plane blocks beyond `clean` are zeroed first
    const bool new_shape = ws->shape[0] != n || ws->shape[1] != M;
    if (new_shape) {
        HIP_TRY(hipMemsetAsync(ws->buf, 0, b_f, st));
        ws->clean = 0;
    }
    if (ws->clean < chunk)
        HIP_TRY(hipMemsetAsync(blocks + ws->clean * blk_el, 0,
                               sizeof(double) * (size_t)blk_el * (chunk - ws->clean), st));
    ws->clean = chunk;                      // the per-call region starts right behind the chunk
    if (new_shape) {
        hipLaunchKernelGGL(psf_prepare, dim3((unsigned)(((int64_t)M * n + 255) / 256)), dim3(256), 0, st,
                           (const double *)nullptr, n, M, (int)kp, (double *)nullptr, (double *)nullptr, fr, fi,
                           (unsigned long long *)nullptr, 0, 1);
        HIP_TRY(hipGetLastError());
        ws->shape[0] = n;
        ws->shape[1] = M;
    }

    // wave_scale -> pinned block (once the previous call's copy has read it) -> device
    const size_t b_scale = sizeof(double) * (size_t)n_items;
    HIP_TRY(ws->stage.acquire(b_scale));
    memcpy(ws->stage.h, wave_scale, b_scale);
    HIP_TRY(hipMemcpyAsync(d_scale, ws->stage.h, b_scale, hipMemcpyHostToDevice, st));
    HIP_TRY(ws->stage.record(st));

    const bool dev_dst = stats && rox::is_device(stats);
    rox_focus_psf_stats *out_stats = dev_dst ? stats : d_stats;
    const bool small = M <= 512;
    const int W = small ? 32 : kTile;
    for (int64_t p0 = 0; p0 < total; p0 += chunk) {
        const int64_t c = std::min(chunk, total - p0);
        double *tr = blocks, *ti = blocks + f_el, *ptr = blocks + 2 * f_el, *pti = ptr + p_el;
        double *dst = psf ? psf + p0 * psf_el : scratch_psf;
        hipLaunchKernelGGL(focus_psf_prepare, dim3((unsigned)nblk, (unsigned)c), dim3(kFocusBlock), 0, st,
                           rows, ld, status, (const double *)d_scale, n_planes, p0, n, (int)kp, blk_el, ptr, pti,
                           partial, maxbits);
        // T = F P per plane, then AP = |T F^T|^2 with each plane's maximum: the tile instance
        // rox_calc_psf takes for this maxdim
        const dim3 g1((unsigned)(np_ / W), (unsigned)(mp / W), (unsigned)c);
        const dim3 g2((unsigned)(mp / W), (unsigned)(mp / W), (unsigned)c);
        if (small) {
            hipLaunchKernelGGL((cgemm_nt_batch<0, 1>), g1, dim3(256), 0, st, fr, fi, (int64_t)0, ptr, pti, blk_el,
                               (int)kp, M, n, tr, ti, blk_el, (int)kp, maxbits);
            hipLaunchKernelGGL((cgemm_nt_batch<1, 1>), g2, dim3(256), 0, st, tr, ti, blk_el, fr, fi, (int64_t)0,
                               (int)kp, M, M, dst, (double *)nullptr, psf_el, M, maxbits);
        } else {
            hipLaunchKernelGGL((cgemm_nt_batch<0, 2>), g1, dim3(256), 0, st, fr, fi, (int64_t)0, ptr, pti, blk_el,
                               (int)kp, M, n, tr, ti, blk_el, (int)kp, maxbits);
            hipLaunchKernelGGL((cgemm_nt_batch<1, 2>), g2, dim3(256), 0, st, tr, ti, blk_el, fr, fi, (int64_t)0,
                               (int)kp, M, M, dst, (double *)nullptr, psf_el, M, maxbits);
        }
        if (psf) {
            const int64_t bx = std::min<int64_t>((psf_el + 255) / 256, 1024);
            hipLaunchKernelGGL(focus_psf_scale, dim3((unsigned)bx, (unsigned)c), dim3(256), 0, st, dst, psf_el,
                               psf_el, (const unsigned long long *)maxbits);
        }
        if (stats)
            hipLaunchKernelGGL(focus_psf_finish, dim3((unsigned)((c + 63) / 64)), dim3(64), 0, st,
                               (const double *)partial, nblk, (int32_t)c, (const unsigned long long *)maxbits,
                               out_stats + p0);
        HIP_TRY(hipGetLastError());
    }
    if (!stats || dev_dst)
        return 0;
    HIP_TRY(hipMemcpyAsync(stats, d_stats, sizeof(rox_focus_psf_stats) * (size_t)total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}
