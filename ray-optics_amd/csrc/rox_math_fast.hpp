// rox_math_fast.hpp -- the arithmetic of the tolerance-mode (F_FAST) instances
#pragma once
#include "rox_math.hpp"

namespace rox {

// ================================================================ tolerance mode
// ROX_FAST_FP64 (rox_opts.flags, include/roxtrace.h): the caller accepts results within the
// tolerance BASELINE's north star states -- 1e-10 on ray intercepts, scaled by max(1, |ref|) --
// instead of the reference's bits.  The reduced-output modes (HITS, HITS_COMPACT, LAST, OPD, FAN)
// are bound by VALU issue, and 2.4 x their algorithmic flop count is the price of bit parity:
// every `/` and `sqrt` a 10-25-instruction correctly rounded expansion behind an exponent-band
// test, every product and sum separately rounded in NumPy's order, |n| re-measured where it is
// 1 by construction.  The F_FAST instances below are still IEEE binary64 throughout, with
//   * v_rcp_f64 / v_rsq_f64 (2^-23 .. 2^-24 relative) + two Newton-Raphson steps (<= ~1.5 ulp)
//     instead of the correctly rounded expansions, no band tests, no fall-back paths;
//   * fused multiply-adds wherever the formula has a*b + c;
//   * refraction through mu = n_in / n_out staged per (wavelength, interface): no division
//     per ray; the surface normal is taken as the unit vector it is (raytrace.py:19-30 divides
//     by its length again), and a sphere's gradient (-cv x, -cv y, 1 - cv z) is not normalised
//     at all: its squared length is 1 + cv F(hit) with F the surface function, i.e. 1 up to
//     the residual of the intersection;
//   * Horner evaluation of the asphere series (profiles.py:849-885, 1070-1113 accumulate
//     powers forward), 1/sqrt from the same iteration that gives the sqrt;
//   * the Spencer-Murty iteration itself as the reference runs it (same start, same
//     convergence test, the penultimate iterate returned): the iterates differ from the
//     reference's by rounding only, so both stop within eps of the same point.
// Ray-failure decisions (miss, TIR, aperture) are taken on values that differ from the
// reference's in the last bits: a ray whose radicand / aperture margin is within rounding of
// zero may be decided the other way (tests/test_gpu_fast.py counts such rays and shows each
// of them on its boundary).  Degenerate operands keep the reference's outcomes where those are
// defined (den == 0 in Spherical.intersect, r == 0 in RadialPolynomial.df, a zero-length
// gradient); NaN and infinity propagate as NaN.

// 1 / b, b != 0 and finite
__device__ __forceinline__ double rcp_f(double b)
{
    double r = __builtin_amdgcn_rcp(b);
    r = fma(r, fma(-b, r, 1.0), r);
#if ROX_FAST_NR >= 2
    r = fma(r, fma(-b, r, 1.0), r);
#endif
    return r;
}

// s = sqrt(x), h = 0.5 / sqrt(x) by the coupled iteration on (x y, y / 2), y = v_rsq_f64(x).
// The seed is taken of x + 2^-1000 (= x for every x >= 2^-947): x = 0 gives s = 0 (a finite y
// times 0) instead of the NaN of 0 * inf -- an on-axis ray has r^2 = 0 exactly -- and NaN stays
// NaN.  (One v_add; fmax() costs two v_max in IEEE mode, the first to quiet a signalling NaN.)
__device__ __forceinline__ void sqrt_half_rsqrt_f(double x, double &s, double &h)
{
    const double y = __builtin_amdgcn_rsq(x + 0x1p-1000);
    s = x * y;
    h = 0.5 * y;
    const double e = fma(-h, s, 0.5);
    s = fma(s, e, s);
    h = fma(h, e, h);
#if ROX_FAST_NR >= 2
    const double e1 = fma(-h, s, 0.5);
    s = fma(s, e1, s);
    h = fma(h, e1, h);
#endif
}

__device__ __forceinline__ double sqrt_f(double x)
{
    const double y = __builtin_amdgcn_rsq(x + 0x1p-1000);
    double s = x * y;
    const double h = 0.5 * y;
    s = fma(s, fma(-h, s, 0.5), s);
#if ROX_FAST_NR >= 2
    s = fma(fma(-s, s, x), h, s);       // (the residual form: h need not be refined for it)
#endif
    return s;
}

__device__ __forceinline__ double dot3_f(const v3 &a, const v3 &b)
{
    return fma(a.z, b.z, fma(a.y, b.y, a.x * b.x));
}

// v / |v|; the zero vector stays the zero vector (misc_math.py:48-54)
__device__ __forceinline__ v3 unit_f(const v3 &v)
{
    double s, h;
    sqrt_half_rsqrt_f(dot3_f(v, v), s, h);
    const double y = h + h;
    return v3{v.x * y, v.y * y, v.z * y};
}

template <class P>
__device__ __forceinline__ v3 rotate_f(P rt, const v3 &v)
{
    return v3{fma(rt[2], v.z, fma(rt[1], v.y, rt[0] * v.x)),
              fma(rt[5], v.z, fma(rt[4], v.y, rt[3] * v.x)),
              fma(rt[8], v.z, fma(rt[7], v.y, rt[6] * v.x))};
}

// raytrace.py:19-38 with a unit normal, ONE formula for every interact mode, straight-line:
//   d_out = mu d + (sg sign(cosI) sqrt(1 - mu^2 (1 - cosI^2)) - mu cosI) n
//   transmit  mu = n_in / n_out, sg = +1          (bend)
//   reflect   mu = 1, sg = -1: the root is |cosI|, d_out = d - 2 cosI n   (reflect)
//   (mu = 1, sg = +1 would pass the direction through -- the bracket is |cosI| sign(cosI) - cosI
//   = 0 -- but dummy and phantom interfaces copy it instead, as the reference does: a NaN normal
//   of a degenerate ray must not reach the direction)
// (mu, mu^2, sg) are staged per (wavelength, interface) by the workgroup.  Returns false where
// the radicand is negative (total internal reflection; out is NaN there).
__device__ __forceinline__ bool interact_f(const v3 &d, const v3 &n, double mu, double mu2, double sg,
                                           v3 &out)
{
    const double c = dot3_f(d, n);
    const double rad = fma(mu2, fma(c, c, -1.0), 1.0);
    const double alpha = fma(sg, copysign(sqrt_f(rad), c), -(mu * c));
    out = v3{fma(alpha, n.x, mu * d.x), fma(alpha, n.y, mu * d.y), fma(alpha, n.z, mu * d.z)};
    return !(rad < 0.0);
}

}  // namespace rox
