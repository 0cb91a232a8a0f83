// imgsim.hip -- image simulation (include/roxtrace.h): rox_varying_blur, a convolution whose
// kernel is interpolated between the nodes of a rectilinear grid, and rox_image_warp, the bilinear
// resampling of a picture under a displacement field given on the same kind of grid.
//
// Both entries reduce the node grid to one record per image row and per image column on the host:
// the cell k the row lies in and its fraction t, so that the row's hat weight is 1 - t at node k,
// t at node k + 1 and zero everywhere else (the host divides: the device only subtracts and
// multiplies).  The records go to the device as one staged block.
//
// blur_kernel: a workgroup of 256 threads owns a tile of 32 rows x 64 columns of one channel; a
// lane owns a column, a wave 8 consecutive rows, the 8 accumulators of a thread stay in registers.
// k is monotone along an axis, so the nodes whose hat support meets the tile's halo are a box
// [kylo, kyhi] x [kxlo, kxhi] read off the records of the halo's first and last row and column;
// the box is walked in row-major order, which is the order the header prescribes, and a node
// outside it has weight zero on every source the tile reads.  Per node the weighted halo
// scene * (wy * wx) is staged in LDS, edge handling included (a source outside the picture is a
// zero term, or the clamped pixel), so that the tap loop has no branch: per tap one ds_read_b64
// per accumulator, consecutive lanes on consecutive doubles (conflict-free at any pitch), the tap
// itself a uniform load from the PSF stack, one multiply and one add.  The halo a tile needs for
// all S tap rows would be (32 + S - 1) x (64 + S - 1) doubles, 98 KiB at S = 65; the tap rows are
// therefore taken in bands of A rows, A sized at launch so that a band's (32 + A - 1) halo rows
// fit 64 KiB.  Per output the order of the additions is the header's whatever A is.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "rox_host.hpp"

namespace {

constexpr int kBlock = 256, kTileW = 64, kRows = 8, kTileH = (kBlock / 64) * kRows;
constexpr int kTapUnroll = 8;
constexpr size_t kLdsBytes = size_t(64) << 10;
constexpr int kMaxDim = 16384, kMaxChan = 16, kMaxTaps = 65;

// the cell and fraction of an image row or column (see the head of this file)
struct AxisRec {
    double t;
    int32_t k;
    int32_t pad;
};

struct BlurArgs {
    const double *scene;
    const double *psf;
    const AxisRec *row;                         // [H]
    const AxisRec *col;                         // [W]
    double *out;
    int32_t H, W, S, GY, GX;
    int32_t band;                               // A: tap rows per staged halo
    int32_t replicate;
};

__device__ __forceinline__ double hat(const AxisRec &r, int k)
{
    return k == r.k ? 1.0 - r.t : (k == r.k + 1 ? r.t : 0.0);
}

__global__ __launch_bounds__(kBlock) void blur_kernel(const BlurArgs a)
{
    extern __shared__ double s_halo[];

    const int H = a.H, W = a.W, S = a.S, r = (S - 1) / 2, A = a.band;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ti0 = blockIdx.y * kTileH, tj0 = blockIdx.x * kTileW, c = blockIdx.z;
    const int pitch = kTileW + S - 1;
    const double *__restrict__ scene = a.scene + (size_t)c * H * W;
    const size_t nn = (size_t)S * S;
    const double *__restrict__ psf_c = a.psf + (size_t)c * a.GY * a.GX * nn;

    // the sources the tile reads, inside the picture with either edge rule
    const int s_lo = max(ti0 - r, 0), s_hi = min(ti0 + kTileH - 1 + r, H - 1);
    const int c_lo = max(tj0 - r, 0), c_hi = min(tj0 + kTileW - 1 + r, W - 1);
    const int kylo = a.row[s_lo].k, kyhi = min(a.row[s_hi].k + 1, a.GY - 1);
    const int kxlo = a.col[c_lo].k, kxhi = min(a.col[c_hi].k + 1, a.GX - 1);

    double acc[kRows];
#pragma unroll
    for (int k = 0; k < kRows; ++k)
        acc[k] = 0.0;

    for (int ky = kylo; ky <= kyhi; ++ky)
        for (int kx = kxlo; kx <= kxhi; ++kx) {
            const double *__restrict__ taps = psf_c + ((size_t)ky * a.GX + kx) * nn;
            for (int a0 = 0; a0 < S; a0 += A) {
                const int a1 = min(a0 + A, S);                      // tap rows [a0, a1)
                // local row l holds source row base_row + l, local column m source column tj0 - r + m
                const int base_row = ti0 - (a1 - 1) + r, n_rows = kTileH + (a1 - a0) - 1;
                __syncthreads();
                for (int e = threadIdx.x; e < n_rows * pitch; e += kBlock) {
                    const int l = e / pitch, m = e - l * pitch;
                    int si = base_row + l, sj = tj0 - r + m;
                    double v = 0.0;
                    const bool inside = si >= 0 && si < H && sj >= 0 && sj < W;
                    if (inside || a.replicate) {
                        si = min(max(si, 0), H - 1);
                        sj = min(max(sj, 0), W - 1);
                        const double w = hat(a.row[si], ky) * hat(a.col[sj], kx);
                        if (w != 0.0)
                            v = scene[(size_t)si * W + sj] * w;
                    }
                    s_halo[e] = v;
                }
                __syncthreads();
                // output row ti0 + wave*kRows + k and tap row ta read local row wave*kRows + k + (a1 - 1 - ta)
                for (int ta = a0; ta < a1; ++ta) {
                    const double *__restrict__ src = s_halo + (wave * kRows + (a1 - 1 - ta)) * pitch + lane + (S - 1);
                    const double *__restrict__ trow = taps + (size_t)ta * S;
                    // kTapUnroll taps per step: one wide uniform load, the next step's issued before
                    // this step's arithmetic, and LDS reads at immediate offsets of one address
                    int tb = 0;
                    double t[kTapUnroll];
                    if (S >= kTapUnroll) {
#pragma unroll
                        for (int u = 0; u < kTapUnroll; ++u)
                            t[u] = trow[u];
                    }
                    for (; tb + kTapUnroll <= S; tb += kTapUnroll) {
                        // (the last step loads its own taps again: no read past the stack)
                        const int nb = tb + 2 * kTapUnroll <= S ? tb + kTapUnroll : tb;
                        double tn[kTapUnroll];
#pragma unroll
                        for (int u = 0; u < kTapUnroll; ++u)
                            tn[u] = trow[nb + u];
#pragma unroll
                        for (int u = 0; u < kTapUnroll; ++u) {
#pragma unroll
                            for (int k = 0; k < kRows; ++k)
                                acc[k] = acc[k] + src[k * pitch - tb - u] * t[u];
                        }
#pragma unroll
                        for (int u = 0; u < kTapUnroll; ++u)
                            t[u] = tn[u];
                    }
                    for (; tb < S; ++tb) {
                        const double tap = trow[tb];
#pragma unroll
                        for (int k = 0; k < kRows; ++k)
                            acc[k] = acc[k] + src[k * pitch - tb] * tap;
                    }
                }
            }
        }

    const int j = tj0 + lane;
    if (j < W) {
        double *__restrict__ out = a.out + (size_t)c * H * W;
#pragma unroll
        for (int k = 0; k < kRows; ++k) {
            const int i = ti0 + wave * kRows + k;
            if (i < H)
                out[(size_t)i * W + j] = acc[k];
        }
    }
}

struct WarpArgs {
    const double *in;
    const double *disp;                         // [GY][GX][2]
    const AxisRec *row;
    const AxisRec *col;
    double *out;
    int32_t H, W, GY, GX;
};

// I[y][x], 0 outside the picture; yd and xd are integers held in doubles
__device__ __forceinline__ double warp_tap(const double *__restrict__ I, int H, int W, double yd, double xd)
{
    if (!(yd >= 0.0 && yd <= (double)(H - 1) && xd >= 0.0 && xd <= (double)(W - 1)))
        return 0.0;
    return I[(size_t)(int)yd * W + (int)xd];
}

__global__ __launch_bounds__(kBlock) void warp_kernel(const WarpArgs a)
{
    const int j = blockIdx.x * 64 + (threadIdx.x & 63), i = blockIdx.y * 4 + (threadIdx.x >> 6), c = blockIdx.z;
    if (i >= a.H || j >= a.W)
        return;
    const AxisRec ry = a.row[i], rx = a.col[j];
    const int k0 = ry.k, k1 = min(ry.k + 1, a.GY - 1), l0 = rx.k, l1 = min(rx.k + 1, a.GX - 1);
    const double ty = ry.t, tx = rx.t;
    const double *d00 = a.disp + 2 * ((size_t)k0 * a.GX + l0), *d01 = a.disp + 2 * ((size_t)k0 * a.GX + l1);
    const double *d10 = a.disp + 2 * ((size_t)k1 * a.GX + l0), *d11 = a.disp + 2 * ((size_t)k1 * a.GX + l1);
    const double dy = (1.0 - ty) * ((1.0 - tx) * d00[0] + tx * d01[0]) + ty * ((1.0 - tx) * d10[0] + tx * d11[0]);
    const double dx = (1.0 - ty) * ((1.0 - tx) * d00[1] + tx * d01[1]) + ty * ((1.0 - tx) * d10[1] + tx * d11[1]);
    const double y = (double)i + dy, x = (double)j + dx;
    const double y0 = floor(y), x0 = floor(x);
    const double fy = y - y0, fx = x - x0;
    const double *__restrict__ I = a.in + (size_t)c * a.H * a.W;
    const double v00 = warp_tap(I, a.H, a.W, y0, x0), v01 = warp_tap(I, a.H, a.W, y0, x0 + 1.0);
    const double v10 = warp_tap(I, a.H, a.W, y0 + 1.0, x0), v11 = warp_tap(I, a.H, a.W, y0 + 1.0, x0 + 1.0);
    a.out[((size_t)c * a.H + i) * a.W + j] =
        (1.0 - fy) * ((1.0 - fx) * v00 + fx * v01) + fy * ((1.0 - fx) * v10 + fx * v11);
}

// ---- the host side

// nodes [n]: finite and strictly increasing
int check_nodes(const char *e, const char *name, const double *node, int32_t n)
{
    if (!node)
        return rox::host_fail(ROX_E_ARG, "%s: null %s", e, name);
    for (int32_t k = 0; k < n; ++k) {
        if (!std::isfinite(node[k]))
            return rox::host_fail(ROX_E_ARG, "%s: %s[%d] = %g is not finite", e, name, k, node[k]);
        if (k && !(node[k] > node[k - 1]))
            return rox::host_fail(ROX_E_ARG, "%s: %s[%d] = %g does not increase", e, name, k, node[k]);
    }
    return 0;
}

// the checks the two entries share: the picture, the node grid, the two buffers
int check_picture(const char *e, int32_t C, int32_t H, int32_t W, int32_t GY, int32_t GX, const double *node_y,
                  const double *node_x, const char *in_name, const double *in, const double *out)
{
    ROX_TRY(rox::check_range(e, "C", C, 1, kMaxChan));
    ROX_TRY(rox::check_range(e, "H", H, 1, kMaxDim));
    ROX_TRY(rox::check_range(e, "W", W, 1, kMaxDim));
    ROX_TRY(rox::check_range(e, "GY", GY, 1, ROX_MAX_FOCUS_ITEMS));
    ROX_TRY(rox::check_range(e, "GX", GX, 1, ROX_MAX_FOCUS_ITEMS));
    if ((int64_t)GY * GX > ROX_MAX_FOCUS_ITEMS)
        return rox::host_fail(ROX_E_ARG, "%s: GY*GX = %lld nodes outside [1, %d]", e, (long long)GY * GX,
                              ROX_MAX_FOCUS_ITEMS);
    ROX_TRY(check_nodes(e, "node_y", node_y, GY));
    ROX_TRY(check_nodes(e, "node_x", node_x, GX));
    if (!in)
        return rox::host_fail(ROX_E_ARG, "%s: null %s", e, in_name);
    if (!out)
        return rox::host_fail(ROX_E_ARG, "%s: null out", e);
    const uintptr_t b = sizeof(double) * (uintptr_t)C * H * W, pi = (uintptr_t)in, po = (uintptr_t)out;
    if (pi < po + b && po < pi + b)
        return rox::host_fail(ROX_E_ARG, "%s: out overlaps %s", e, in_name);
    return 0;
}

// rec[i], i = 0 .. n - 1, from the nodes [g]: the header's hat weights
void axis_records(AxisRec *rec, int32_t n, const double *node, int32_t g)
{
    int32_t k = 0;
    for (int32_t i = 0; i < n; ++i) {
        const double x = (double)i;
        AxisRec &o = rec[i];
        o.pad = 0;
        if (g == 1 || x < node[0]) {
            o.k = 0;
            o.t = 0.0;
        } else if (x >= node[g - 1]) {
            o.k = g - 1;
            o.t = 0.0;
        } else {
            while (!(x < node[k + 1]))
                ++k;                                // node[k] <= x < node[k + 1]
            o.k = k;
            o.t = (x - node[k]) / (node[k + 1] - node[k]);
        }
    }
}

rox::PerStream<rox::Workspace> g_is_ws;

// What the two entries do around their kernel: the records and a small host table (the
// displacements) staged as one block, host pictures mirrored in the workspace.
struct Plan {
    rox::Turn<> ws;
    AxisRec *d_rec = nullptr;
    double *d_tab = nullptr;                    // the table, behind the records
    double *d_in = nullptr, *d_stack = nullptr, *d_out = nullptr;
    bool in_host = false, stack_host = false, out_host = false;

    // in [in_b bytes] and the optional stack [stack_b] are host or device, tab [tab_b] is HOST
    int prepare(const char *where, hipStream_t st, int32_t H, int32_t W, int32_t GY, int32_t GX, const double *node_y,
                const double *node_x, const double *in, size_t in_b, const double *stack, size_t stack_b,
                const double *tab, size_t tab_b, double *out, size_t out_b)
    {
        const char *const kHipWhere = where;
        ROX_TRY(ws.take(g_is_ws, st, where));
        in_host = !rox::is_device(in);
        stack_host = stack && !rox::is_device(stack);
        out_host = !rox::is_device(out);
        const size_t o_tab = sizeof(AxisRec) * ((size_t)H + W), b_tab = o_tab + tab_b;
        char *d_block;
        rox::Layout L;
        L.add(d_block, rox::up256(b_tab));
        L.add(d_in, in_host ? rox::up256(in_b) : 0);
        L.add(d_stack, stack_host ? rox::up256(stack_b) : 0);
        L.add(d_out, out_host ? rox::up256(out_b) : 0);
        char *h;
        ROX_TRY(ws.carve(L, b_tab, &h));
        axis_records((AxisRec *)h, H, node_y, GY);
        axis_records((AxisRec *)h + H, W, node_x, GX);
        if (tab_b)
            memcpy(h + o_tab, tab, tab_b);
        ROX_TRY(ws.upload(d_block, b_tab));
        d_rec = (AxisRec *)d_block;
        d_tab = (double *)(d_block + o_tab);
        if (in_host)
            HIP_TRY(hipMemcpyAsync(d_in, in, in_b, hipMemcpyDefault, st));
        else
            d_in = const_cast<double *>(in);
        if (stack_host)
            HIP_TRY(hipMemcpyAsync(d_stack, stack, stack_b, hipMemcpyDefault, st));
        else
            d_stack = const_cast<double *>(stack);
        if (!out_host)
            d_out = out;
        return 0;
    }

    // after the kernel: a host destination is copied, and host memory of the caller's is waited for
    int finish(const char *where, hipStream_t st, double *out, size_t out_b)
    {
        const char *const kHipWhere = where;
        HIP_TRY(hipGetLastError());
        if (out_host)
            HIP_TRY(hipMemcpyAsync(out, d_out, out_b, hipMemcpyDefault, st));
        if (in_host || stack_host || out_host)
            HIP_TRY(hipStreamSynchronize(st));
        return 0;
    }
};

}  // namespace

extern "C" int rox_varying_blur(int32_t C, int32_t H, int32_t W, const double *scene, int32_t S, int32_t GY,
                                int32_t GX, const double *psf, const double *node_y, const double *node_x,
                                double *out, uint32_t flags, void *stream)
{
    static const char kE[] = "rox_varying_blur", kHipWhere[] = "rox_varying_blur: ";
    // every argument check comes before anything touches a device
    ROX_TRY(rox::check_range(kE, "S", S, 1, kMaxTaps));
    if (!(S & 1))
        return rox::host_fail(ROX_E_ARG, "%s: S %d is even", kE, S);
    ROX_TRY(check_picture(kE, C, H, W, GY, GX, node_y, node_x, "scene", scene, out));
    if (!psf)
        return rox::host_fail(ROX_E_ARG, "%s: null psf", kE);
    if (flags & ~(uint32_t)ROX_BLUR_EDGE_REPLICATE)
        return rox::host_fail(ROX_E_ARG, "%s: flags 0x%x: unknown bits", kE, flags);

    hipStream_t st = (hipStream_t)stream;
    const size_t pic_b = sizeof(double) * (size_t)C * H * W, psf_b = sizeof(double) * (size_t)C * GY * GX * S * S;
    Plan p;
    ROX_TRY(p.prepare(kHipWhere, st, H, W, GY, GX, node_y, node_x, scene, pic_b, psf, psf_b, nullptr, 0, out, pic_b));

    BlurArgs a{};
    a.scene = p.d_in;
    a.psf = p.d_stack;
    a.row = p.d_rec;
    a.col = p.d_rec + H;
    a.out = p.d_out;
    a.H = H; a.W = W; a.S = S; a.GY = GY; a.GX = GX;
    a.replicate = (flags & ROX_BLUR_EDGE_REPLICATE) != 0;
    // the tap rows of one staged halo: (kTileH + A - 1) rows of (kTileW + S - 1) doubles in kLdsBytes
    const int pitch = kTileW + S - 1;
    a.band = std::min<int>(S, (int)(kLdsBytes / (sizeof(double) * pitch)) - (kTileH - 1));
    const size_t lds = sizeof(double) * (size_t)(kTileH + a.band - 1) * pitch;
    const dim3 grid((unsigned)((W + kTileW - 1) / kTileW), (unsigned)((H + kTileH - 1) / kTileH), (unsigned)C);
    hipLaunchKernelGGL(blur_kernel, grid, dim3(kBlock), lds, st, a);
    return p.finish(kHipWhere, st, out, pic_b);
}

extern "C" int rox_image_warp(int32_t C, int32_t H, int32_t W, const double *in, int32_t GY, int32_t GX,
                              const double *node_y, const double *node_x, const double *disp, double *out,
                              void *stream)
{
    static const char kE[] = "rox_image_warp", kHipWhere[] = "rox_image_warp: ";
    ROX_TRY(check_picture(kE, C, H, W, GY, GX, node_y, node_x, "in", in, out));
    if (!disp)
        return rox::host_fail(ROX_E_ARG, "%s: null disp", kE);
    for (int64_t i = 0; i < 2 * (int64_t)GY * GX; ++i)
        if (!std::isfinite(disp[i]))
            return rox::host_fail(ROX_E_ARG, "%s: disp[%lld] = %g is not finite", kE, (long long)i, disp[i]);

    hipStream_t st = (hipStream_t)stream;
    const size_t pic_b = sizeof(double) * (size_t)C * H * W, disp_b = sizeof(double) * 2 * (size_t)GY * GX;
    Plan p;
    ROX_TRY(p.prepare(kHipWhere, st, H, W, GY, GX, node_y, node_x, in, pic_b, nullptr, 0, disp, disp_b, out, pic_b));

    WarpArgs a{};
    a.in = p.d_in;
    a.disp = p.d_tab;
    a.row = p.d_rec;
    a.col = p.d_rec + H;
    a.out = p.d_out;
    a.H = H; a.W = W; a.GY = GY; a.GX = GX;
    const dim3 grid((unsigned)((W + 63) / 64), (unsigned)((H + 3) / 4), (unsigned)C);
    hipLaunchKernelGGL(warp_kernel, grid, dim3(kBlock), 0, st, a);
    return p.finish(kHipWhere, st, out, pic_b);
}
