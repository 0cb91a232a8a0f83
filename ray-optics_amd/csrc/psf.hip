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
//   psf_twiddles     F (twiddles: once per shape)
//   psf_phases       P^T (phase of the block, transposed)
//   cgemm_nt<0>      T = F P            C[i][j] = sum_k A[i][k] B[j][k], complex (rox_cgemm.hpp)
//   cgemm_nt<1>      AP = |T F^T|^2 and its maximum (epilogue)
//   focus_psf_scale  AP / max
// rox_focus_psf runs the same steps over a batch of through-focus planes (blockIdx.y / .z =
// plane): focus_psf_prepare reads the rows and adds the Strehl partials in place of psf_phases,
// and focus_psf_finish closes each plane.  rox_calc_psf is the batch of one plane.
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

#include "rox_cgemm.hpp"
#include "rox_host.hpp"

namespace {

constexpr char kHipWhere[] = "rox_calc_psf: ";

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

// P^T of the OPD grid, and the call's maximum reset for the second GEMM
__global__ void psf_phases(const double *opd, int n, int kp, double *ptr, double *pti, unsigned long long *maxbits)
{
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx == 0)
        *maxbits = 0;               // this call's maximum starts from zero (the second GEMM folds into it)
    if (idx < (int64_t)n * n) {
        const int a = (int)(idx / n), b = (int)(idx % n);
        double s, c;
        pupil_phase(opd[idx], c, s);
        ptr[(int64_t)b * kp + a] = c;
        pti[(int64_t)b * kp + a] = s;
    }
}

// F (per shape: it depends on (n, M) only).  n = ndim, M = maxdim, kp = padded n.
//   block origin o = M/2 - (n/2 - 1)                       (analyses.py:861-863)
//   fftshift = roll by h = M/2 on input and output          (numpy.fft.fftshift)
//   F[u][a]  = exp(-2 pi i ((u - h) mod M) ((o + a + h) mod M) / M)
__global__ void psf_twiddles(int n, int M, int kp, double *fr, double *fi)
{
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < (int64_t)M * n) {
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

// plane blockIdx.y's PSF divided by its maximum
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

// ---- host side ---------------------------------------------------------------------------------

// The sizes of one PSF, Shape{ndim, maxdim}: n and M padded to the GEMM tiles.
struct Shape {
    int n, M;
    int64_t kp = round_up(n, kKBlock);                      // n to the k block
    int64_t mp = round_up(M, kTile), np_ = round_up(n, kTile);     // M and n to the workgroup tile
    int64_t f_el = mp * kp, p_el = np_ * kp;                // doubles of an F / T plane and of a P^T plane
    int64_t blk_el = 2 * f_el + 2 * p_el;                   // ... of a plane block: tr ti ptr pti
    int64_t psf_el = (int64_t)M * M;
    bool small = M <= 512;                                  // the 32 x 32 workgroup tile
};

// the shape of entry e's (ndim, maxdim), or ROX_E_ARG
int psf_shape(const char *e, int32_t ndim, int32_t maxdim, Shape *s)
{
    // the reference's slice assignment (analyses.py:861-863) only has a matching shape
    // for an even ndim whose block fits inside the maxdim array
    if (ndim < 2 || (ndim & 1))
        return rox::host_fail(ROX_E_ARG, "%s: ndim %d must be even and >= 2", e, ndim);
    const int n = ndim, M = maxdim;
    const int o = M / 2 - (n / 2 - 1);
    if (M < 2 || o < 0 || o + n > M)
        return rox::host_fail(ROX_E_ARG, "%s: the ndim %d block does not fit in maxdim %d", e, n, M);
    if (M > 32768)
        return rox::host_fail(ROX_E_ARG, "%s: maxdim %d > 32768", e, M);
    *s = Shape{n, M};
    return 0;
}

// T[u][b] = sum_a F[u][a] P[a][b], then AP[u][v] = |sum_b T[u][b] F[v][b]|^2 with its maximum, for
// c planes: plane z's block is z * blk doubles after `block`, its PSF z * sd doubles after dst.
// 64 x 64 workgroup tiles give a (64, 256) problem 4 and 16 workgroups on 256 CUs: up to
// maxdim 512 the 32 x 32 instance is used (one MFMA tile per wave, four times the workgroups)
void launch_gemms(const Shape &s, int64_t c, const double *fr, double *block, int64_t blk, double *dst,
                  int64_t sd, unsigned long long *maxbits, hipStream_t st)
{
    const double *fi = fr + s.f_el;
    double *tr = block, *ti = tr + s.f_el, *ptr = ti + s.f_el, *pti = ptr + s.p_el;
    const int W = s.small ? 32 : kTile;
    const dim3 g1((unsigned)(s.np_ / W), (unsigned)(s.mp / W), (unsigned)c);
    const dim3 g2((unsigned)(s.mp / W), (unsigned)(s.mp / W), (unsigned)c);
    const auto first = s.small ? cgemm_nt<0, 1> : cgemm_nt<0, 2>;
    const auto second = s.small ? cgemm_nt<1, 1> : cgemm_nt<1, 2>;
    hipLaunchKernelGGL(first, g1, dim3(256), 0, st, fr, fi, (int64_t)0, ptr, pti, blk, (int)s.kp, s.M, s.n, tr, ti,
                       blk, (int)s.kp, maxbits);
    hipLaunchKernelGGL(second, g2, dim3(256), 0, st, tr, ti, blk, fr, fi, (int64_t)0, (int)s.kp, s.M, s.M, dst,
                       (double *)nullptr, sd, s.M, maxbits);
}

// each of c PSFs, sd doubles apart, divided by its maximum
void launch_scale(const Shape &s, int64_t c, double *dst, int64_t sd, const unsigned long long *maxbits,
                  hipStream_t st)
{
    const int64_t bx = std::min<int64_t>((s.psf_el + 255) / 256, 1024);
    hipLaunchKernelGGL(focus_psf_scale, dim3((unsigned)bx, (unsigned)c), dim3(256), 0, st, dst, s.psf_el, sd, maxbits);
}

// The grow-only workspace of an entry per (device, stream):
//   [F: fr fi] [plane blocks: tr ti ptr pti, one per plane of a launch] [per call: maximums, host
//   copies; rox_focus_psf: partial records, statistics, wave scales, PSF scratch]
// F and the plane blocks are zero-padded to the GEMM tiles, so they sit at offsets that depend on
// the shape alone; the per-call region behind them may overwrite plane blocks a later, larger
// rox_focus_psf call then zeroes again (`clean` counts the plane blocks known to be zero-padded).
// The two entries keep a workspace each: a figure's rox_calc_psf and a through-focus call of
// another shape on one stream would otherwise evict each other's twiddles.
struct PsfWorkspace : rox::Workspace {
    int64_t shape[2] = {0, 0};      // (n, M) F was formed for
    int64_t clean = 0;

    // at least `need` bytes; a new block has no F and no clean plane block
    hipError_t grow(size_t need)
    {
        if (cap < need)
            shape[0] = shape[1] = clean = 0;
        return reserve(need);
    }

    // F at fr and `chunk` zero-padded plane blocks at `blocks` for shape s.  Every element inside
    // the (n, M) shape is rewritten by each call and the padding is never written, so the planes
    // need zeroing only when the workspace is new or the shape changes; the twiddles F depend on
    // the shape alone and are formed then too (at figure sizes a call is little but stream
    // operations and sincospi).  Forming the phases inside the first product instead -- three
    // launches -- measured slower from (64, 256) up: every block row repeats the n^2 sincos.
    hipError_t prepare(const Shape &s, int64_t chunk, double *fr, double *blocks, hipStream_t st)
    {
        const bool formed = shape[0] == s.n && shape[1] == s.M;
        hipError_t e = hipSuccess;
        if (!formed) {
            clean = 0;
            e = hipMemsetAsync(fr, 0, sizeof(double) * 2 * (size_t)s.f_el, st);
        }
        if (e == hipSuccess && clean < chunk)
            e = hipMemsetAsync(blocks + clean * s.blk_el, 0, sizeof(double) * (size_t)(s.blk_el * (chunk - clean)), st);
        if (e != hipSuccess)
            return e;
        clean = chunk;                  // the per-call region starts right behind the chunk
        if (formed)
            return hipSuccess;
        hipLaunchKernelGGL(psf_twiddles, dim3((unsigned)(((int64_t)s.M * s.n + 255) / 256)), dim3(256), 0, st, s.n,
                           s.M, (int)s.kp, fr, fr + s.f_el);
        if ((e = hipGetLastError()) == hipSuccess) {
            shape[0] = s.n;
            shape[1] = s.M;
        }
        return e;
    }
};
rox::PerStream<PsfWorkspace> g_ws, g_focus_ws;

constexpr char kFocusWhere[] = "rox_focus_psf: ";

// scratch per launch (T and P^T of each plane, the PSF when psf is NULL) is capped; larger
// batches run as consecutive launches (as rox_trace_through_focus_grids caps its partials)
constexpr size_t kFocusPsfScratchBytes = size_t(256) << 20;

}  // namespace

extern "C" int rox_calc_psf(const double *opd, int32_t ndim, int32_t maxdim, double *psf,
                            uint32_t flags, void *stream)
{
    static const char kE[] = "rox_calc_psf";
    if (!opd || !psf)
        return rox::host_fail(ROX_E_ARG, "%s: null argument", kE);
    if (flags & ~(uint32_t)ROX_HOST_POINTERS)
        return rox::host_fail(ROX_E_ARG, "%s: unknown flag", kE);
    Shape s{};
    ROX_TRY(psf_shape(kE, ndim, maxdim, &s));
    hipStream_t st = (hipStream_t)stream;
    // calls on one stream share the workspace: enqueue them whole, one after the other
    // (stream order then keeps their kernels apart); host-pointer calls hold it until done
    rox::Turn<PsfWorkspace> ws;
    ROX_TRY(ws.take(g_ws, st, kHipWhere));

    const bool host = (flags & ROX_HOST_POINTERS) != 0;
    const size_t b_opd = host ? sizeof(double) * (size_t)s.n * s.n : 0;
    const size_t b_psf = host ? sizeof(double) * (size_t)s.psf_el : 0;
    double *fr, *block, *d_opd, *d_psf;
    unsigned long long *maxbits;
    rox::Layout L;
    L.add(fr, sizeof(double) * 2 * (size_t)s.f_el).add(block, sizeof(double) * (size_t)s.blk_el);
    L.add(maxbits, 256).add(d_opd, rox::up256(b_opd)).add(d_psf, b_psf);
    HIP_TRY(ws->grow(L.size()));
    L.carve(ws->buf);
    HIP_TRY(ws->prepare(s, 1, fr, block, st));
    const double *src = opd;
    double *dst = psf;
    if (host) {
        HIP_TRY(hipMemcpyAsync(d_opd, opd, b_opd, hipMemcpyHostToDevice, st));
        src = d_opd;
        dst = d_psf;
    }
    hipLaunchKernelGGL(psf_phases, dim3((unsigned)(((int64_t)s.n * s.n + 255) / 256)), dim3(256), 0, st, src, s.n,
                       (int)s.kp, block + 2 * s.f_el, block + 2 * s.f_el + s.p_el, maxbits);
    launch_gemms(s, 1, fr, block, 0, dst, 0, maxbits, st);
    launch_scale(s, 1, dst, 0, maxbits, st);
    HIP_TRY(hipGetLastError());
    if (host) {
        HIP_TRY(hipMemcpyAsync(psf, d_psf, b_psf, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return 0;
}

extern "C" int rox_focus_psf(int32_t n_items, int32_t n_planes, const double *rows, int64_t ld,
                             const uint8_t *status, const double *wave_scale, int32_t ndim, int32_t maxdim,
                             double *psf, rox_focus_psf_stats *stats, void *stream)
{
    static const char kE[] = "rox_focus_psf";
    const char *const kHipWhere = kFocusWhere;
    // every argument check comes before anything touches a device
    ROX_TRY(rox::check_range(kE, "n_items", n_items, 1, ROX_MAX_FOCUS_ITEMS));
    ROX_TRY(rox::check_range(kE, "n_planes", n_planes, 1, ROX_MAX_FOCUS_PLANES));
    Shape s{};
    ROX_TRY(psf_shape(kE, ndim, maxdim, &s));
    const int n = s.n;
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
    rox::Turn<PsfWorkspace> ws;
    ROX_TRY(ws.take(g_focus_ws, st, kHipWhere));

    const int64_t nblk = ((int64_t)n * n + kFocusBlock - 1) / kFocusBlock;
    const int64_t total = (int64_t)n_items * n_planes;
    const size_t per_plane = sizeof(double) * (size_t)(s.blk_el + (psf ? 0 : s.psf_el) + 3 * nblk) + 8;
    const int64_t chunk = rox::chunk_for(total, per_plane, kFocusPsfScratchBytes);
    double *fr, *blocks, *partial, *d_scale, *scratch_psf;
    unsigned long long *maxbits;
    rox_focus_psf_stats *d_stats;
    rox::Layout L;
    L.add(fr, sizeof(double) * 2 * (size_t)s.f_el).add(blocks, sizeof(double) * (size_t)s.blk_el * chunk);
    L.add(maxbits, rox::up256(sizeof(unsigned long long) * chunk));
    L.add(partial, rox::up256(sizeof(double) * 3 * (size_t)nblk * chunk));
    L.add(d_stats, rox::up256(sizeof(rox_focus_psf_stats) * (size_t)total));
    L.add(d_scale, rox::up256(sizeof(double) * (size_t)n_items));
    L.add(scratch_psf, psf ? 0 : sizeof(double) * (size_t)s.psf_el * chunk);
    HIP_TRY(ws->grow(L.size()));
    L.carve(ws->buf);
    HIP_TRY(ws->prepare(s, chunk, fr, blocks, st));

    // wave_scale -> pinned block (once the previous call's copy has read it) -> device
    const size_t b_scale = sizeof(double) * (size_t)n_items;
    HIP_TRY(ws->stage.acquire(b_scale));
    memcpy(ws->stage.h, wave_scale, b_scale);
    HIP_TRY(hipMemcpyAsync(d_scale, ws->stage.h, b_scale, hipMemcpyHostToDevice, st));
    HIP_TRY(ws->stage.record(st));

    const bool dev_dst = stats && rox::is_device(stats);
    rox_focus_psf_stats *out_stats = dev_dst ? stats : d_stats;
    for (int64_t p0 = 0; p0 < total; p0 += chunk) {
        const int64_t c = std::min(chunk, total - p0);
        double *ptr = blocks + 2 * s.f_el, *pti = ptr + s.p_el;
        double *dst = psf ? psf + p0 * s.psf_el : scratch_psf;
        hipLaunchKernelGGL(focus_psf_prepare, dim3((unsigned)nblk, (unsigned)c), dim3(kFocusBlock), 0, st,
                           rows, ld, status, (const double *)d_scale, n_planes, p0, n, (int)s.kp, s.blk_el, ptr, pti,
                           partial, maxbits);
        launch_gemms(s, c, fr, blocks, s.blk_el, dst, s.psf_el, maxbits, st);
        if (psf)
            launch_scale(s, c, dst, s.psf_el, maxbits, st);
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
