// rox_profiles.hpp -- surface profiles: the closed-form quadric intersection, the polynomial
// aspheres and toroids with their Spencer-Murty iteration, the tolerance-mode twins (_f) and the
// straight-line form (_sl) of the reduced-output loop; clear-aperture lists.
#pragma once
#include <cstddef>

#include "rox_args.hpp"
#include "rox_math.hpp"
#include "rox_math_fast.hpp"

namespace rox {

// profiles.py:321-336 / 580-593: s = cx2 / (z_dir*sqrt(b*b - ax2*cx2) - b)
__device__ __forceinline__ bool quadric_root(double ax2, double cx2, double b,
                                             double z_dir, double &s)
{
    if ((b != 0) || (cx2 != 0) || (ax2 != 0)) {
        const double rad = b * b - ax2 * cx2;
        if (rad < 0.0)
            return false;                       // TraceMissedSurfaceError
        const double den = z_dir * slim_sqrt(rad) - b;
        // np.errstate(divide='raise') -> FloatingPointError -> s = 0 only for a
        // finite non-zero numerator; 0/0 and nan/0 stay NaN
        if (den == 0.0 && cx2 != 0.0 && isfinite(cx2))
            s = 0.0;
        else
            s = cx2 / den;
    } else {
        s = 0.0;
    }
    return true;
}

// Spherical (conic == false) / Conic closed-form intersection
__device__ __forceinline__ bool quadric_hit(bool conic, double cv, double cc, double ec,
                                            const v3 &p, const v3 &d, double z_dir,
                                            double &s, v3 &hit)
{
    double ax2, cx2, b;
    if (!conic) {
        ax2 = cv;
        cx2 = cv * dot3(p, p) - 2 * p.z;
        b = cv * dot3(d, p) - d.z;
    } else {
        ax2 = cv * (1. + cc * d.z * d.z);
        cx2 = cv * (p.x * p.x + p.y * p.y + ec * p.z * p.z) - 2.0 * p.z;
        b = cv * (d.x * p.x + d.y * p.y + ec * d.z * p.z) - d.z;
    }
    if (!quadric_root(ax2, cx2, b, z_dir, s))
        return false;
    hit = v3{p.x + s * d.x, p.y + s * d.y, p.z + s * d.z};
    return true;
}

// One evaluation of f(p) and df(p) for the polynomial aspheres
// (profiles.py:849-885 even, 1070-1113 radial; forward accumulation of the
// powers, not Horner).  Returns false when the sag square root goes negative.
// kind = ROX_EVENPOLY | ROX_RADIALPOLY | ROX_YTOROID | ROX_XTOROID (wave-uniform);
// The sag and slope series of the polynomial profiles in one pass: two independent chains,
//   z_asp += coef_i * z_pow;  z_pow *= m;     e_asp += (c_i * coef_i) * e_pow;  e_pow *= m
// -- the same operations in the same order as the reference's two loops (forward power
// accumulation, every product and sum separately rounded).  cd = the row's interleaved
// (coef_i, c_i * coef_i) pairs, one 16-byte LDS word per term.
//
// A full-length series in the RadialPolynomial instance (all eight aspheres of the phone lens
// carry ten coefficients) is straight-line code: the ten LDS words are requested before the
// first product needs one, where the generic loop -- unrolled by eight plus a one-term
// remainder loop by the compiler -- waits for most words one at a time.  Phone lens HITS 249
// -> 232 us, FULL 284.5 -> 264 us per 2^20 rays, bit-identical.  Measured and not kept
// (gpurun_out/r04e, r04f): the same for every instance (the EvenPolynomial instance pays for
// the extra code: Nikkor HITS 319 -> 330 us), straight-line for every length with a scalar
// branch per term (Nikkor 330, .zmx zoom 161 -> 171, phone lens 242), and prefetching the next
// term's word in the loop (phone lens 253).
//
// SHARED (the EvenPolynomial and toroid call sites: z_pow = m, e_pow = 1): the slope loop's power
// 1 * m * m ... and the sag loop's m * m ... are the same numbers one term apart (1 * m is m
// exactly, and from there both chains multiply the same value by m), so one chain serves both --
// five operations per term instead of six, every result the one the two loops produce.
template <int FEAT, bool SHARED = false, class CD>
__device__ __forceinline__ void series2(CD cd, int ncoef, double m, double z_pow, double e_pow,
                                        double &z_asp, double &e_asp)
{
    z_asp = 0.0;
    e_asp = 0.0;
    if (SHARED) {
        double pw = 1.0;                    // e_pow of term i; pw * m = z_pow of term i
        for (int i = 0; i < ncoef; ++i) {
            const d2 c = cd[i];
            e_asp += c.y * pw;
            pw *= m;
            z_asp += c.x * pw;
        }
        return;
    }
    if ((FEAT & F_RADIAL) && !(FEAT & F_EVEN) && ncoef == ROX_MAX_COEF) {
        d2 c[ROX_MAX_COEF];
#pragma unroll
        for (int i = 0; i < ROX_MAX_COEF; ++i)
            c[i] = cd[i];
#pragma unroll
        for (int i = 0; i < ROX_MAX_COEF; ++i) {
            z_asp += c[i].x * z_pow;
            z_pow *= m;
            e_asp += c[i].y * e_pow;
            e_pow *= m;
        }
        return;
    }
    for (int i = 0; i < ncoef; ++i) {
        const d2 c = cd[i];
        z_asp += c.x * z_pow;
        z_pow *= m;
        e_asp += c.y * e_pow;           // (c_coef*coefs[i])*r_pow
        e_pow *= m;
    }
}

// FEAT says which of the three families this kernel instance carries code for.
template <int FEAT, bool WANT_F, class TP>
__device__ __forceinline__ bool poly_eval(int kind, double cv, double cc1, double ec, double cR,
                                          int ncoef, TP coefs,
                                          const v3 &p, double &f, v3 &df)
{
    // (coefs[i], dcoefs[i]) pairs of the device row
    const auto cd = pairs_of(coefs + (offsetof(dev_surface, cd) - offsetof(rox_surface, coefs)) / 8);
    if ((FEAT & F_TOROID) && (!(FEAT & (F_EVEN | F_RADIAL)) || kind >= ROX_YTOROID)) {
        // profiles.py:1337-1377 YToroid.fY/f/df; XToroid swaps x and y (:1429-1434)
        const bool xt = (kind == ROX_XTOROID);
        const double px = xt ? p.y : p.x, py = xt ? p.x : p.y;
        const double y2 = py * py;
        const double rad = 1. - cc1 * cv * cv * y2;
        if (rad < 0.0)
            return false;
        const double srad = slim_sqrt(rad);
        double z_asp, e_asp;
        series2<FEAT, true>(cd, ncoef, y2, y2, 1, z_asp, e_asp);
        const double fY = slim_div(cv * y2, 1. + srad) + z_asp;
        if (WANT_F)
            f = p.z - fY - cR * (px * px + p.z * p.z - fY * fY) / 2;
        const double dfdY = slim_div(cv, srad) + e_asp;
        const double Fx = -cR * px;
        const double Fy = (cR * fY - 1) * (dfdY) * py;
        df = xt ? v3{Fy, Fx, 1 - cR * p.z} : v3{Fx, Fy, 1 - cR * p.z};
        return true;
    }
    const bool radial = (FEAT & F_RADIAL) && (!(FEAT & F_EVEN) || kind == ROX_RADIALPOLY);
    const double r2 = p.x * p.x + p.y * p.y;
    double e_tot;
    // sag() and df() take the square root of the same radicand when
    // (cc + 1.0) and ec are the same number (they are, unless a caller fills the
    // table otherwise): evaluate it once.  `same` is wave-uniform.
    const bool same = (cc1 == ec) || radial;
    const double rad_e = 1. - ec * cv * cv * r2;
    if (!radial) {
        double srad_e;
        if (WANT_F) {
            const double rad = 1. - cc1 * cv * cv * r2;     // (cc + 1.0)*cv*cv*r2
            if (rad < 0.0)
                return false;
            const double srad = slim_sqrt(rad);
            srad_e = srad;
            if (!same) {
                // (a real wave-uniform branch, kept one by the empty asm: written as the select
                // `same ? srad : sqrt(rad_e)` hipcc evaluated the second square root -- the full
                // expansion, ~23 VALU incl. a quarter-rate v_rsq_f64 -- in EVERY evaluation)
                asm volatile("" ::: "memory");
                srad_e = sqrt(rad_e);
            }
            const double z = slim_div(cv * r2, 1. + srad);
            const double e = slim_div(cv, srad_e);
            double z_asp, e_asp;
            series2<FEAT, true>(cd, ncoef, r2, r2, 1, z_asp, e_asp);
            f = p.z - (z + z_asp);
            e_tot = e + e_asp;
        } else {
            srad_e = sqrt(rad_e);
            const double e = slim_div(cv, srad_e);
            double r_pow = 1, e_asp = 0.0;
            for (int i = 0; i < ncoef; ++i) {
                e_asp += cd[i].y * r_pow;       // (c_coef*coefs[i])*r_pow
                r_pow *= r2;
            }
            e_tot = e + e_asp;
        }
    } else {
        const double r = slim_sqrt(r2);
        if (WANT_F && rad_e < 0.0)
            return false;
        const double srad_e = WANT_F ? slim_sqrt(rad_e) : sqrt(rad_e);   // NaN when negative
        const double e = slim_div(cv, srad_e);
        double e_asp = 0.0;
        double e_pow = (r == 0.0) ? 1.0 : slim_div(1.0, r);
        if (WANT_F) {
            const double z = slim_div(cv * r2, 1. + srad_e);
            double z_asp;
            series2<FEAT>(cd, ncoef, r, r, e_pow, z_asp, e_asp);
            f = p.z - (z + z_asp);
        } else {
            for (int i = 0; i < ncoef; ++i) {
                e_asp += cd[i].y * e_pow;
                e_pow *= r;
            }
        }
        e_tot = e + e_asp;
    }
    df = v3{-e_tot * p.x, -e_tot * p.y, 1.0};
    return true;
}

// profiles.py:155-186 Spencer & Murty Newton iteration.  Returns the last
// *evaluated* iterate as the hit point (p0 itself when |s1| <= eps at once).
template <int FEAT, class TP>
__device__ __forceinline__ bool newton_hit(int kind, double cv, double cc1, double ec, double cR,
                                           int ncoef, TP coefs,
                                           const v3 &p0, const v3 &d, double eps,
                                           double &s, v3 &hit, v3 &df)
{
    v3 p = p0;
    double f;
    if (!poly_eval<FEAT, true>(kind, cv, cc1, ec, cR, ncoef, coefs, p, f, df))
        return false;
    double s1 = slim_div(-f, dot3(d, df));      // (the quotient through slim_div(), bit for bit `/`)
    double delta = fabs(s1);
    int iter = 0;
    bool ok = true;
    // one Spencer-Murty step for the lanes that have not converged
    auto step = [&]() {
        p = v3{p0.x + s1 * d.x, p0.y + s1 * d.y, p0.z + s1 * d.z};
        if (!poly_eval<FEAT, true>(kind, cv, cc1, ec, cR, ncoef, coefs, p, f, df)) {
            ok = false;
            delta = 0.0;            // leave the iteration; the caller reports the miss
            return;
        }
        const double s2 = s1 - slim_div(f, dot3(d, df));
        delta = fabs(s2 - s1);
        s1 = s2;
        ++iter;
    };
    // measured on the reference's even-asphere zoom: 2 steps 20 %, 3 steps 73 %,
    // 4 steps 6 %, more < 1 %.  The plain loop (cap 1000 as in the reference).
    // Rounds 1-4 spelled four steps straight-line in front of it (six inlined evaluations per
    // asphere site); the loop alone -- two -- is a third of the code and faster: Nikkor HITS
    // 329 -> 314 us, .zmx 143.2 -> 141.5
    while (delta > eps && iter < 1000)
        step();
    if (!ok)
        return false;
    s = s1;
    hit = p;        // df already holds df(hit): normal() re-evaluates the same expression
    return true;
}

// profiles.py:321-336 / 580-593.  The reference's outcomes for a vanishing denominator
// (FloatingPointError -> s = 0 for a finite non-zero numerator, NaN for 0/0 unless all three
// coefficients vanish) are kept by one wave-uniform test.
// Straight-line: a negative radicand does not leave -- the lane's s and hit become NaN (the
// seed of sqrt_f is NaN for it) and the caller reads the returned flag.  A branch here costs a
// saved exec mask and, where the paths meet again, a register copy per live value.
__device__ __forceinline__ bool quadric_hit_f(bool conic, double cv, double cc, double ec,
                                              const v3 &p, const v3 &d, double z_dir,
                                              double &s, v3 &hit)
{
    double ax2, cx2, b;
    if (!conic) {
        ax2 = cv;
        cx2 = fma(cv, dot3_f(p, p), -(p.z + p.z));
        b = fma(cv, dot3_f(d, p), -d.z);
    } else {
        ax2 = cv * fma(cc * d.z, d.z, 1.0);
        const double ez = ec * p.z;
        cx2 = fma(cv, fma(ez, p.z, fma(p.y, p.y, p.x * p.x)), -(p.z + p.z));
        b = fma(cv, fma(ez, d.z, fma(d.y, p.y, d.x * p.x)), -d.z);
    }
    const double rad = fma(-ax2, cx2, b * b);
    const double den = fma(z_dir, sqrt_f(rad), -b);
    s = cx2 * rcp_f(den);
    if (__builtin_amdgcn_ballot_w64(den == 0.0) != 0) {
        if (den == 0.0) {
            if (cx2 != 0.0 && isfinite(cx2))
                s = 0.0;
            else if (b == 0.0 && cx2 == 0.0 && ax2 == 0.0)
                s = 0.0;
            else
                s = __builtin_nan("");
        }
    }
    hit = v3{fma(s, d.x, p.x), fma(s, d.y, p.y), fma(s, d.z, p.z)};
    return !(rad < 0.0);                        // false: TraceMissedSurfaceError
}

// f(p), df(p) of EvenPolynomial / RadialPolynomial (profiles.py:849-885, 1070-1113), Horner
// form.  Toroids keep the exact evaluation (poly_eval): no workload of BASELINE carries one.
template <int FEAT, class TP>
__device__ __forceinline__ bool poly_eval_f(int kind, double cv, double cc1, double ec, double cR,
                                            int ncoef, TP coefs, const v3 &p, double &f, v3 &df)
{
    if ((FEAT & F_TOROID) && kind >= ROX_YTOROID)
        return poly_eval<FEAT & ~F_FAST, true>(kind, cv, cc1, ec, cR, ncoef, coefs, p, f, df);
    const auto cd = pairs_of(coefs + (offsetof(dev_surface, cd) - offsetof(rox_surface, coefs)) / 8);
    const bool radial = (FEAT & F_RADIAL) && (!(FEAT & F_EVEN) || kind == ROX_RADIALPOLY);
    const double r2 = fma(p.y, p.y, p.x * p.x);
    const double cv2 = cv * cv;
    double z_asp = 0.0, e_asp = 0.0, e_tot;
    if (!radial) {
        // sag: z = cv r2 / (1 + sqrt(1 - (cc+1) cv^2 r2)) + sum coef_i r2^(i+1)
        // df:  e = cv / sqrt(1 - ec cv^2 r2)               + sum 2(i+1) coef_i r2^i
        const double rad = fma(-cc1 * cv2, r2, 1.0);
        if (rad < 0.0)
            return false;
        double srad, hrad;
        sqrt_half_rsqrt_f(rad, srad, hrad);
        double he = hrad;                       // 0.5 / sqrt(rad_e)
        if (cc1 != ec) {                        // (wave-uniform; equal unless a caller fills ec otherwise)
            double se;
            const double rad_e = fma(-ec * cv2, r2, 1.0);
            sqrt_half_rsqrt_f(rad_e, se, he);
            if (rad_e < 0.0)
                he = __builtin_nan("");         // np.sqrt of a negative: NaN, no exception
        }
        for (int i = ncoef - 1; i >= 0; --i) {
            const d2 c = cd[i];
            z_asp = fma(z_asp, r2, c.x);
            e_asp = fma(e_asp, r2, c.y);
        }
        const double z = (cv * r2) * rcp_f(1.0 + srad);
        f = p.z - fma(z_asp, r2, z);
        e_tot = fma(cv + cv, he, e_asp);
    } else {
        // sag: z = cv r2 / (1 + sqrt(1 - ec cv^2 r2)) + sum coef_i r^(i+1)
        // df:  e = cv / sqrt(.)                         + sum (i+1) coef_i r^(i-1)
        const double rad = fma(-ec * cv2, r2, 1.0);
        if (rad < 0.0)
            return false;
        double srad, hrad, r, hr;
        sqrt_half_rsqrt_f(rad, srad, hrad);
        sqrt_half_rsqrt_f(r2, r, hr);
        const double rinv = (r2 == 0.0) ? 1.0 : hr + hr;    // profiles.py:1104: r_pow = 1 at r = 0
        for (int i = ncoef - 1; i >= 1; --i) {
            const d2 c = cd[i];
            z_asp = fma(z_asp, r, c.x);
            e_asp = fma(e_asp, r, c.y);
        }
        const d2 c0 = cd[0];
        z_asp = fma(z_asp, r, ncoef > 0 ? c0.x : 0.0);
        e_asp = fma(ncoef > 0 ? c0.y : 0.0, rinv, e_asp);
        const double z = (cv * r2) * rcp_f(1.0 + srad);
        f = p.z - fma(z_asp, r, z);
        e_tot = fma(cv + cv, hrad, e_asp);
    }
    df = v3{-e_tot * p.x, -e_tot * p.y, 1.0};
    return true;
}

// profiles.py:155-186, as newton_hit() runs it
template <int FEAT, class TP>
__device__ __forceinline__ bool newton_hit_f(int kind, double cv, double cc1, double ec, double cR,
                                             int ncoef, TP coefs, const v3 &p0, const v3 &d,
                                             double eps, double &s, v3 &hit, v3 &df)
{
    v3 p = p0;
    double f;
    if (!poly_eval_f<FEAT>(kind, cv, cc1, ec, cR, ncoef, coefs, p, f, df))
        return false;
    double s1 = -f * rcp_f(dot3_f(d, df));
    double delta = fabs(s1);
    int iter = 0;
    bool ok = true;
    while (delta > eps && iter < 1000) {
        p = v3{fma(s1, d.x, p0.x), fma(s1, d.y, p0.y), fma(s1, d.z, p0.z)};
        if (!poly_eval_f<FEAT>(kind, cv, cc1, ec, cR, ncoef, coefs, p, f, df)) {
            ok = false;
            break;
        }
        const double s2 = fma(-f, rcp_f(dot3_f(d, df)), s1);
        delta = fabs(s2 - s1);
        s1 = s2;
        ++iter;
    }
    if (!ok)
        return false;
    s = s1;
    hit = p;
    return true;
}

// profiles.py:321-336 / 580-593 as quadric_root() / quadric_hit() compute them, without the early exit
__device__ __forceinline__ bool quadric_hit_sl(bool conic, double cv, double cc, double ec,
                                               const v3 &p, const v3 &d, double z_dir,
                                               double &s, v3 &hit)
{
    double ax2, cx2, b;
    if (!conic) {
        ax2 = cv;
        cx2 = cv * dot3(p, p) - 2 * p.z;
        b = cv * dot3(d, p) - d.z;
    } else {
        ax2 = cv * (1. + cc * d.z * d.z);
        cx2 = cv * (p.x * p.x + p.y * p.y + ec * p.z * p.z) - 2.0 * p.z;
        b = cv * (d.x * p.x + d.y * p.y + ec * d.z * p.z) - d.z;
    }
    const double rad = b * b - ax2 * cx2;
    const double den = z_dir * slim_sqrt(rad) - b;      // (NaN where rad < 0: flagged below)
    double sq = cx2 / den;      // (through slim_div(): measured slower, EXPERIMENTS.md round 6)
    // np.errstate(divide='raise') -> FloatingPointError -> s = 0 only for a finite non-zero
    // numerator; 0/0 and nan/0 stay NaN; all three coefficients zero: s = 0 without dividing
    if (den == 0.0 && cx2 != 0.0 && isfinite(cx2))
        sq = 0.0;
    if (!((b != 0) || (cx2 != 0) || (ax2 != 0)))
        sq = 0.0;
    s = sq;
    hit = v3{p.x + s * d.x, p.y + s * d.y, p.z + s * d.z};
    return !(rad < 0.0) || !((b != 0) || (cx2 != 0) || (ax2 != 0));
}

// surface.py:198-208 (+ surface.py:416-419, 453-457): the AND over an interface's
// clear_apertures.  A circular aperture's radius slot of the STAGED row holds
// sqrt_le_threshold(radius + fuzz) (stage_aperture_thresholds() below), so that
// `sqrt(xx*xx + yy*yy) <= radius + fuzz` is decided without the square root, outcome for
// outcome; interfaces without a list take the max_aperture threshold (Ctx.apthr).
// thr != nullptr (the F_GTAB instances, whose table is read-only): the interface's circular
// thresholds, staged in LDS beside the table instead of inside it.
template <class TP>
__device__ __forceinline__ bool inside_aperture_list(TP row, int n_ap, double x, double y, double fuzz,
                                                     tblp thr = nullptr)
{
    auto ap = row + (offsetof(rox_surface, ap) / sizeof(double));
    for (int k = 0; k < n_ap; ++k, ap += sizeof(rox_aperture) / sizeof(double)) {
        const int2 ki{ints_of(ap)[0], ints_of(ap)[1]};            // kind, is_obscuration
        const double xx = x - ap[1];
        const double yy = y - ap[2];
        bool ans;
        if (ki.x == ROX_AP_CIRCULAR)
            ans = (xx * xx + yy * yy) <= (thr ? thr[k] : ap[3]);    // the staged threshold
        else if (ki.x == ROX_AP_RECTANGULAR)
            ans = (fabs(xx) <= ap[3] + fuzz) && (fabs(yy) <= ap[4] + fuzz);
        else
            return false;               // Elliptical: point_inside() returns None
        if (ki.y)
            ans = !ans;
        if (!ans)
            return false;
    }
    return true;
}

// Post-pass over the table a workgroup has staged in LDS (instances with aperture lists; call
// between two workgroup barriers): the radius of every circular clear aperture becomes the
// largest s with sqrt(s) <= radius + fuzz.  `fuzz` is the launch's pt_inside_fuzz.
template <int FEAT>
__device__ __forceinline__ void stage_aperture_thresholds(double *tbl_w, int N, double fuzz, int tid,
                                                          int nthreads)
{
    if (!(FEAT & F_APLIST))
        return;
    for (int i = tid; i < N * ROX_MAX_AP; i += nthreads) {
        double *row = tbl_w + (size_t)(i / ROX_MAX_AP) * kRowDoubles;
        const int k = i % ROX_MAX_AP;
        if (k < reinterpret_cast<const int32_t *>(row)[3]) {
            double *ap = row + offsetof(rox_surface, ap) / sizeof(double) +
                         (size_t)k * (sizeof(rox_aperture) / sizeof(double));
            if (reinterpret_cast<const int32_t *>(ap)[0] == ROX_AP_CIRCULAR)
                ap[3] = sqrt_le_threshold(ap[3] + fuzz);
        }
    }
}

}  // namespace rox
