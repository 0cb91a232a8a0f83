// rox_math.hpp -- the exact arithmetic of the trace kernels: 3-vectors, the table pointer types,
// NumPy's dot / dgemv sites as explicit fma chains, the wave votes and the slim fp64 square root
// and division that are bit-identical to sqrt() and `/`.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rox_config.hpp"

namespace rox {

struct v3 { double x, y, z; };
typedef double d2 __attribute__((ext_vector_type(2)));

typedef const double *tblp;     // LDS (generic pointer into __shared__)
typedef const int32_t *tbli;
// The same table left in GLOBAL memory and read through the constant address space (the F_GTAB
// instances): a wave-uniform address in that space is a scalar load (s_load_dwordx2..x16 through
// the scalar cache), the value lands in SGPRs and no LDS is involved -- so a table has no size
// limit (SequentialModel has none: rayoptics/seq/sequential.py:167-202) and the tolerance-mode
// kernels, which issue one LDS broadcast per five VALU instructions otherwise, keep the LDS
// pipe out of their way.  Every function below that reads the table is a template over the
// pointer type; ints_of() / pairs_of() reinterpret within the pointer's own address space.
typedef const __attribute__((address_space(4))) double *ctblp;
typedef const __attribute__((address_space(4))) int32_t *ctbli;
typedef const __attribute__((address_space(4))) d2 *ctbl2;
__device__ __forceinline__ tbli ints_of(tblp p) { return reinterpret_cast<tbli>(p); }
__device__ __forceinline__ ctbli ints_of(ctblp p) { return (ctbli)p; }
__device__ __forceinline__ const d2 *pairs_of(tblp p) { return reinterpret_cast<const d2 *>(p); }
__device__ __forceinline__ ctbl2 pairs_of(ctblp p) { return (ctbl2)p; }

// ---------------------------------------------------------------- arithmetic
// np.dot / ndarray.dot / np.linalg.norm on float64[3] = OpenBLAS ddot:
// acc = 0; acc = fma(a_i, b_i, acc), i = 0, 1, 2.
__device__ __forceinline__ double dot3(const v3 &a, const v3 &b)
{
    double acc = fma(a.x, b.x, 0.0);
    acc = fma(a.y, b.y, acc);
    return fma(a.z, b.z, acc);
}

// Rt.dot(v) = OpenBLAS dgemv: an fma chain per output row; the column order is
// 0,1,2 for the F-ordered transpose view and 1,0,2 for a C-ordered array
// (include/roxtrace.h ROX_RT_*).  `order` is wave-uniform.
template <class P>
__device__ __forceinline__ v3 rotate(P rt, int order, const v3 &v)
{
    v3 r;
    if (order == ROX_RT_C_ORDER) {
        r.x = fma(rt[2], v.z, fma(rt[0], v.x, fma(rt[1], v.y, 0.0)));
        r.y = fma(rt[5], v.z, fma(rt[3], v.x, fma(rt[4], v.y, 0.0)));
        r.z = fma(rt[8], v.z, fma(rt[6], v.x, fma(rt[7], v.y, 0.0)));
    } else {
        r.x = fma(rt[2], v.z, fma(rt[1], v.y, fma(rt[0], v.x, 0.0)));
        r.y = fma(rt[5], v.z, fma(rt[4], v.y, fma(rt[3], v.x, 0.0)));
        r.z = fma(rt[8], v.z, fma(rt[7], v.y, fma(rt[6], v.x, 0.0)));
    }
    return r;
}

// np.cross on float64[3]: each component is multiply, multiply, subtract
__device__ __forceinline__ v3 cross3(const v3 &a, const v3 &b)
{
    return v3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}

// ---------------------------------------------------------------- slim fp64
// hipcc expands an f64 sqrt into v_rsq_f64 + 9 mul/fma (correctly rounded) wrapped
// in input scaling (v_ldexp x2), a class test and selects; and every f64 `/` into
// v_div_scale x2 + v_rcp_f64 + two Newton steps + q, residual, v_div_fmas,
// v_div_fixup.  The scaling and fix-up only act on operands outside a band of
// exponents (or zero / inf / nan).  Inside the band the functions below execute
// the SAME instruction sequence minus those wrappers, so the results are
// bit-identical; three quotients by one divisor share the refined reciprocal.
// A wave takes the slim path only when every active lane passes the exponent
// test (one wave-uniform branch); otherwise it falls back to the plain operators.
//   band: biased exponent in [640, 1408)  <=>  2^-383 <= |x| < 2^385
//   (v_div_scale scales when exponents differ by >= 768 or the numerator's
//   exponent <= 53; the sqrt expansion scales below 2^-767)
// every active lane of the wave passes `p`.  __all() goes through an integer (v_cndmask 0/1,
// v_cmp_ne, s_cmp vcc == exec); the ballot of the failing lanes is the compare mask itself
// (inactive lanes read 0): two VALU instructions fewer per test site.
__device__ __forceinline__ bool wave_all(bool p)
{
    return __builtin_amdgcn_ballot_w64(!p) == 0;
}

__device__ __forceinline__ bool in_band(double x)
{
    const uint32_t h = (uint32_t)__double2hiint(x) & 0x7fffffffu;
    return (h - 0x28000000u) < 0x30000000u;
}

// numerators may also be exactly +-0 (the sign is restored below)
__device__ __forceinline__ bool in_band_or_zero(double x) { return in_band(x) || x == 0.0; }

// sqrt for x in the band: the expansion of llvm.sqrt.f64 without scaling/selects
__device__ __forceinline__ double sqrt_band(double x)
{
    const double y = __builtin_amdgcn_rsq(x);
    double s = x * y;
    double h = y * 0.5;
    const double r0 = fma(-h, s, 0.5);
    s = fma(s, r0, s);
    h = fma(h, r0, h);
    const double d0 = fma(-s, s, x);
    s = fma(d0, h, s);
    const double d1 = fma(-s, s, x);
    return fma(d1, h, s);
}

__device__ __forceinline__ double slim_sqrt(double x)
{
#if ROX_SLIM_FP64
    if (wave_all(in_band(x)))
        return sqrt_band(x);
#endif
    return sqrt(x);
}

// refined reciprocal exactly as the division expansion builds it (no scaling)
__device__ __forceinline__ double rcp_band(double b)
{
    double r = __builtin_amdgcn_rcp(b);
    r = fma(r, fma(-b, r, 1.0), r);
    r = fma(r, fma(-b, r, 1.0), r);
    return r;
}

// a / b given r = rcp_band(b): quotient, exact residual, correction; v_div_fixup's
// only effect inside the band is forcing the sign, which also covers a == +-0
__device__ __forceinline__ double div_band(double a, double b, double r)
{
    const double q = a * r;
    const double q1 = fma(fma(-b, q, a), r, q);
    return copysign(q1, q);
}

// a / b
__device__ __forceinline__ double slim_div(double a, double b)
{
#if ROX_SLIM_FP64
    if (wave_all(in_band(b) && in_band_or_zero(a)))
        return div_band(a, b, rcp_band(b));
#endif
    return a / b;
}

// (a.x / b, a.y / b, a.z / b)
__device__ __forceinline__ v3 slim_div3(const v3 &a, double b)
{
#if ROX_SLIM_FP64
    if (wave_all(in_band(b) && in_band_or_zero(a.x) && in_band_or_zero(a.y) && in_band_or_zero(a.z))) {
        const double r = rcp_band(b);
        return v3{div_band(a.x, b, r), div_band(a.y, b, r), div_band(a.z, b, r)};
    }
#endif
    return v3{a.x / b, a.y / b, a.z / b};
}

// Largest s with sqrt(s) <= t.  The aperture test of the reference is
// `sqrt(x*x + y*y) <= max_aperture + fuzz` (interface.py:113-122); the correctly
// rounded sqrt is monotonic, so that is the same predicate as `x*x + y*y <= u(t)`
// with u = this threshold -- computed once per surface per workgroup, it takes the
// square root out of the per-ray path without changing a single outcome (NaN and
// infinities included).
__device__ __forceinline__ double sqrt_le_threshold(double t)
{
    if (!(t >= 0.0))
        return (t != t) ? t : -1.0;             // NaN: never true; negative: never true
    if (t == __builtin_inf())
        return t;
    double s = t * t;
    if (s == __builtin_inf())
        s = 1.7976931348623157e308;
    while (sqrt(s) > t)                         // at most a few steps either way
        s = __longlong_as_double(__double_as_longlong(s) - 1);
    for (;;) {
        if (s >= 1.7976931348623157e308)
            break;
        const double n = __longlong_as_double(__double_as_longlong(s) + 1);
        if (sqrt(n) > t)
            break;
        s = n;
    }
    return s;
}

// numerator test of unit(): zero, or not below the band (the upper edge is implied there)
__device__ __forceinline__ bool zero_or_not_tiny(double x)
{
    const uint32_t h = (uint32_t)__double2hiint(x) & 0x7fffffffu;
    return h >= 0x28000000u || x == 0.0;
}

// misc_math.py:48-54 normalize
__device__ __forceinline__ v3 unit(const v3 &v)
{
    const double l2 = dot3(v, v);
#if ROX_SLIM_FP64
    // One decision for the sqrt and the three quotients (against slim_sqrt() then slim_div3():
    // 6 fewer band-test instructions per surface, HITS 120.5 -> 117.1 us).  l2 in the band puts
    // len = sqrt(l2) in [2^-192, 2^193) -- inside the band and non-zero, no test needed --
    // and every |v_i| <= len (1 + 2^-51) < 2^385, so only the lower edge of the numerators
    // is tested.  The instruction sequences are those of slim_sqrt / slim_div3.
    if (wave_all(in_band(l2) && zero_or_not_tiny(v.x) && zero_or_not_tiny(v.y) && zero_or_not_tiny(v.z))) {
        const double len = sqrt_band(l2);
        const double r = rcp_band(len);
        return v3{div_band(v.x, len, r), div_band(v.y, len, r), div_band(v.z, len, r)};
    }
    const double len = sqrt(l2);
    if (len == 0.0)
        return v;
    return v3{v.x / len, v.y / len, v.z / len};
#else
    const double len = slim_sqrt(l2);
    if (len == 0.0)
        return v;
    return slim_div3(v, len);
#endif
}

// raytrace.py:19-30.  false = TIR (math.sqrt ValueError)
__device__ __forceinline__ bool refract(const v3 &d, const v3 &nrm, double n_in,
                                        double n_out, v3 &out)
{
    const double nlen = slim_sqrt(dot3(nrm, nrm));
    const double cosI = dot3(d, nrm) / nlen;
    const double sin2 = 1.0 - cosI * cosI;
    const double rad = n_out * n_out - n_in * n_in * sin2;
    if (rad < 0.0)
        return false;
    const double n_cosIp = copysign(slim_sqrt(rad), cosI);
    const double alpha = n_cosIp - n_in * cosI;
    const v3 num{n_in * d.x + alpha * nrm.x, n_in * d.y + alpha * nrm.y, n_in * d.z + alpha * nrm.z};
    out = slim_div3(num, n_out);
    return true;
}

// raytrace.py:33-38 (not renormalised)
__device__ __forceinline__ v3 mirror(const v3 &d, const v3 &nrm)
{
    const double nlen = slim_sqrt(dot3(nrm, nrm));
    const double cosI = dot3(d, nrm) / nlen;
    const double k = 2.0 * cosI;
    return v3{d.x - k * nrm.x, d.y - k * nrm.y, d.z - k * nrm.z};
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        v += __shfl_xor(v, o);
    return v;
}

}  // namespace rox
