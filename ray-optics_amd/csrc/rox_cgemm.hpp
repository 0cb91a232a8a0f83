// rox_cgemm.hpp -- the batched complex fp64 GEMM on the matrix cores (v_mfma_f64_16x16x4_f64)
// that psf.hip (the pruned DFT of rox_calc_psf and rox_focus_psf) and huygens.hip (the wavelet sum
// of rox_huygens_psf) both run: C[i][j] = sum_k A[i][k] B[j][k], complex.
//
// Matrices are kept as separate real / imaginary planes, row-major with the
// reduction index contiguous and padded with zeros to a multiple of 16 (rows
// to a multiple of 64), so the GEMM loads need no guards.
//
// Every output element is its own chain of MFMA accumulations over k in ascending order, the
// same chain in both tile shapes: an element's bits depend on its operand rows alone, not on the
// tile shape, on where the row sits in the matrix or on what else the launch computes.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int kTile = 64;           // workgroup tile (4 waves, 32 x 32 each)
constexpr int kKBlock = 16;         // reduction step of the main loop

__host__ __device__ inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

// The complex GEMM of problem z = blockIdx.z, its operands sa / sb / sc doubles after problem 0's
// (a stride 0 shares F) and its maximum in maxbits[z].  A plane of a batch and a single call
// (gridDim.z = 1) run the same instance.
template <int EPI, int TM>      // TM x TM MFMA tiles per wave: 2 (32 x 32, large problems) or 1 (figure sizes)
__global__ __launch_bounds__(256) void cgemm_nt(const double *__restrict__ ar0, const double *__restrict__ ai0,
                                                int64_t sa, const double *__restrict__ br0,
                                                const double *__restrict__ bi0, int64_t sb, int kp, int I, int J,
                                                double *c00, double *c10, int64_t sc, int ldc,
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

}  // namespace
