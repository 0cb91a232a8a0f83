// selftest.hip -- rox_selftest_fp64 (include/roxtrace_diag.h): the slim fp64 paths of rox_math.hpp
// against the plain operators, on the device.
#include <hip/hip_runtime.h>

#include "rox_math.hpp"
#include "rox_host.hpp"
#include "../../include/roxtrace_diag.h"

#pragma clang fp contract(off)

using namespace rox;

namespace {

constexpr char kHipWhere[] = "";

// Diagnostic: the slim fp64 paths against the plain operators on pseudo-random
// operands spanning the whole exponent range (zeros, denormals, band edges,
// inf and nan included).  counts[0] = sqrt mismatches, counts[1] = division
// mismatches, counts[2] = operand sets that took a slim path, counts[3] = the
// same for the band-edge classes.
__device__ __forceinline__ uint64_t mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ double with_exponent(uint64_t bits, uint64_t e)
{
    return __longlong_as_double((long long)((bits & 0x800fffffffffffffull) | (e << 52)));
}

// operand `slot` (0..2 numerators, 3 divisor) of class `kind`; every class is
// wave-uniform, so that the wave-uniform slim branch is decided by the class
__device__ __forceinline__ double test_operand(uint64_t bits, int kind, int slot)
{
    switch (kind) {
    case 0:                                         // any bit pattern
        return __longlong_as_double((long long)bits);
    case 1:                                         // 2^-40 .. 2^40 (the common case)
        return with_exponent(bits, 1023 - 40 + (bits >> 52) % 80);
    case 2: {                                       // specials
        const double sp[] = {0.0, -0.0, 1.0, -1.0, 4.9e-324, 2.2250738585072014e-308,
                             0x1p-383, 0x1.fffffffffffffp-384, 0x1p385, 0x1.fffffffffffffp384,
                             1.7976931348623157e308, __builtin_inf(), -__builtin_inf(),
                             __builtin_nan(""), 0x1p-767, 3.0};
        return sp[bits % 16];
    }
    case 3:                                         // every lane at the band's edges
        return with_exponent(bits, (bits >> 52) & 1 ? ((bits >> 53) & 1 ? 640 : 641)
                                                    : ((bits >> 53) & 1 ? 1406 : 1407));
    case 4:                                         // exponent spread 767: numerators at the
        if (slot < 3)                               // bottom, divisor at the top (and +-0 mixed in)
            return (bits >> 60) == 0 ? ((bits >> 59) & 1 ? -0.0 : 0.0) : with_exponent(bits, 640);
        return with_exponent(bits, 1407);
    case 5:                                         // the other way round
        if (slot < 3)
            return (bits >> 60) == 0 ? ((bits >> 59) & 1 ? -0.0 : 0.0) : with_exponent(bits, 1407);
        return with_exponent(bits, 640);
    default:                                        // one step outside the band: must fall back
        return with_exponent(bits, (bits >> 52) & 1 ? 639 : 1408);
    }
}

__device__ __forceinline__ bool same_bits(double a, double b)
{
    return __double_as_longlong(a) == __double_as_longlong(b) || (a != a && b != b);
}

__global__ void __launch_bounds__(kBlock) selftest_kernel(uint64_t n, uint64_t seed,
                                                           unsigned long long *counts)
{
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * kBlock) {
        // one operand class per wave: half the waves the common case, the rest
        // cycling through the other classes
        const uint64_t wv = i / 64;
        const int kind = (wv & 1) ? 1 : (int)((wv >> 1) % 7);
        const uint64_t k = i * 4 + seed * 0x9e3779b97f4a7c15ull;
        const double a0 = test_operand(mix64(k), kind, 0), a1 = test_operand(mix64(k + 1), kind, 1);
        const double a2 = test_operand(mix64(k + 2), kind, 2), b = test_operand(mix64(k + 3), kind, 3);
        const double x = fabs(a0);
        if (!same_bits(slim_sqrt(x), sqrt(x)))
            atomicAdd(&counts[0], 1ull);
        const v3 q = slim_div3(v3{a0, a1, a2}, b);
        if (!same_bits(q.x, a0 / b) || !same_bits(q.y, a1 / b) || !same_bits(q.z, a2 / b))
            atomicAdd(&counts[1], 1ull);
        if (!same_bits(slim_div(a1, b), a1 / b))
            atomicAdd(&counts[1], 1ull);
        if (__all(in_band(b) && in_band_or_zero(a0) && in_band_or_zero(a1) && in_band_or_zero(a2))) {
            atomicAdd(&counts[2], 1ull);
            if (kind >= 3)
                atomicAdd(&counts[3], 1ull);
        }
        // unit(): one decision for its sqrt and quotients (the numerators' upper edge is
        // implied by |v_i| <= |v|).  Components of very different magnitudes, some scaled
        // down to the band's lower edge and below, zeros included.
        {
            const double sc[4] = {1.0, 0x1p-200, 0x1p-381, 0x1p-390};
            // (scales are wave-uniform so that whole waves sit on either side of the edge)
            const double k0 = sc[(wv >> 4) & 3], k1 = sc[(wv >> 6) & 3], k2 = sc[(wv >> 8) & 3];
            const v3 w{a0 * k0, (mix64(k + 9) & 7) == 0 ? 0.0 : a1 * k1, a2 * k2};
            const v3 u = unit(w);
            const double len = sqrt(dot3(w, w));
            const v3 r = (len == 0.0) ? w : v3{w.x / len, w.y / len, w.z / len};
            if (!same_bits(u.x, r.x) || !same_bits(u.y, r.y) || !same_bits(u.z, r.z))
                atomicAdd(&counts[1], 1ull);
        }
        // the sqrt-free aperture test: (sqrt(s) <= t) == (s <= sqrt_le_threshold(t)) for s
        // within a few ulps of t*t and far from it (mismatches are counted as sqrt mismatches)
        {
            const double t = (kind == 2) ? a1 : fabs(a1);
            const double thr = sqrt_le_threshold(t);
            const long long k9 = (long long)(mix64(k + 7) % 9) - 4;
            double s2 = t * t;
            if (s2 > 0 && s2 < 1e300)
                s2 = __longlong_as_double(__double_as_longlong(s2) + k9);
            const double cand[3] = {s2, fabs(a2), fabs(a0) * fabs(a0)};
            for (int q = 0; q < 3; ++q)
                if ((sqrt(cand[q]) <= t) != (cand[q] <= thr))
                    atomicAdd(&counts[0], 1ull);
        }
    }
}

}  // namespace

extern "C" int rox_selftest_fp64(uint64_t n, uint64_t seed, uint64_t counts[4])
{
    if (!counts)
        return host_fail(ROX_E_ARG, "null argument");
    unsigned long long *d = nullptr;
    HIP_TRY(hipMalloc(&d, 4 * sizeof(unsigned long long)));
    HIP_TRY(hipMemset(d, 0, 4 * sizeof(unsigned long long)));
    hipLaunchKernelGGL(selftest_kernel, dim3(2048), dim3(kBlock), 0, nullptr, n, seed, d);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = hipMemcpy(counts, d, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess)
        return host_fail(ROX_E_HIP, "selftest: %s", hipGetErrorString(e));
    return 0;
}
