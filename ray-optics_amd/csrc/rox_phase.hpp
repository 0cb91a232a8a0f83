// rox_phase.hpp -- phase elements: diffraction gratings, radial DOEs, holograms / thin lenses
#pragma once
#include <cstddef>

#include "rox_math.hpp"

namespace rox {

// ------------------------------------------------------------------ phase
// x**n as the reference's `r_sqr**(i+1)` evaluates it: libm pow(), which is
// correctly rounded except for ~1e-3 of its arguments.  Here: the product in
// double-double (error ~2^-100), rounded once -- the correctly rounded power.
__device__ __forceinline__ double pow_int(double x, int n)
{
    if (n == 0)
        return 1.0;
    double hi = x, lo = 0.0;
    for (int k = 1; k < n; ++k) {
        const double ph = hi * x;
        const double pl = fma(hi, x, -ph);
        const double t = fma(lo, x, pl);
        hi = ph + t;
        lo = t - (hi - ph);
    }
    return hi;
}

enum { PHASE_OK = 0, PHASE_EVANESCENT = 1, PHASE_TIR = 2 };

// raytrace.py:41-48 phase() over the phase element of the row.  ph points at
// rox_surface.ph of the row; pc at the (wavelength, interface) grating
// constants.  Returns PHASE_*; `out` = after_dir, `dW` = phs.
template <class TP>
__device__ __forceinline__ int apply_phase(TP ph, TP pc, const v3 &pt, const v3 &in_dir,
                                           const v3 &srf_nrml, double z_dir, double wvl,
                                           double n_in, double n_out, int mode, v3 &out,
                                           double &dW)
{
    constexpr int O_ORDER = offsetof(rox_phase, order) / 8, O_REFWL = offsetof(rox_phase, ref_wl) / 8,
                  O_SPACING = offsetof(rox_phase, spacing_nm) / 8, O_A = offsetof(rox_phase, a) / 8,
                  O_B = offsetof(rox_phase, b) / 8, O_COEF = offsetof(rox_phase, coefs) / 8;
    const int kind = ints_of(ph)[0];
    if (kind == ROX_PH_GRATING) {               // doe.py:124-175 phase_ludwig
        const double refl = (mode == ROX_REFLECT) ? -1.0 : 1.0;
        const v3 un = unit(srf_nrml);
        const v3 normal{z_dir * un.x, z_dir * un.y, z_dir * un.z};
        const v3 G{ph[O_A], ph[O_A + 1], ph[O_A + 2]};
        const v3 P = cross3(G, normal);
        const v3 D = unit(cross3(normal, P));
        const double mu = pc[0], mu2 = pc[1], T = pc[2], T2 = pc[3];
        const double in_cosI = dot3(in_dir, normal);
        const double V = mu * in_cosI;
        const double W = mu2 - 1 + T2 - 2 * mu * T * dot3(D, in_dir);
        const double result = sqrt(V * V - W);  // np.sqrt: NaN, not an exception
        const double Q1 = result - V;
        const double Q2 = -result - V;
        // Python's max(a, b) = b if b > a else a; min(a, b) = b if b < a else a
        double Q = Q1;
        if (mode == ROX_TRANSMIT)
            Q = (Q2 > Q1) ? Q2 : Q1;
        else if (mode == ROX_REFLECT)
            Q = (Q2 < Q1) ? Q2 : Q1;
        v3 o{mu * in_dir.x - T * D.x + Q * normal.x, mu * in_dir.y - T * D.y + Q * normal.y,
             mu * in_dir.z - T * D.z + Q * normal.z};
        const double rz = 1 - o.x * o.x - o.y * o.y;
        if (rz < 0.0)
            return PHASE_EVANESCENT;            // math.sqrt ValueError
        o.z = copysign(sqrt(rz), o.z);
        const double si = 1 - in_cosI * in_cosI;
        if (si < 0.0)
            return PHASE_EVANESCENT;
        const double in_sinI = sqrt(si);
        const double out_cosI = dot3(o, normal);
        const double so = 1 - out_cosI * out_cosI;
        if (so < 0.0)
            return PHASE_EVANESCENT;
        const double out_sinI = sqrt(so);
        dW = (ph[O_SPACING] / wvl) * (n_in * in_sinI + refl * n_out * out_sinI);
        out = o;
        return PHASE_OK;
    }
    if (kind == ROX_PH_DOE_RADIAL) {            // doe.py:272-323 + radial_phase_fct :28-54
        const double order = ph[O_ORDER];
        const v3 normal = unit(srf_nrml);
        v3 inc = in_dir;
        if (n_in != 1.0) {
            if (!refract(in_dir, srf_nrml, n_in, 1.0, inc))
                return PHASE_TIR;
        }
        const double in_cosI = dot3(inc, normal);
        const double mu = wvl / ph[O_REFWL];
        const double r_sqr = pt.x * pt.x + pt.y * pt.y;
        double w = 0, dWdX = 0, dWdY = 0;
        const int nc = ints_of(ph)[1];
        for (int i = 0; i < nc; ++i) {
            const double c = ph[O_COEF + i];
            w += c * pow_int(r_sqr, i + 1);
            const double r_exp = pow_int(r_sqr, i);
            const double fc = (double)(2 * (i + 1)) * c;
            dWdX += fc * pt.x * r_exp;
            dWdY += fc * pt.y * r_exp;
        }
        const double om = order * mu;
        const double b = in_cosI + om * (normal.x * dWdX + normal.y * dWdY);
        const double c = mu * (mu * (dWdX * dWdX + dWdY * dWdY) / 2 +
                               order * (inc.x * dWdX + inc.y * dWdY));
        const double rad = b * b - 2 * c;
        if (rad < 0.0)
            return PHASE_EVANESCENT;
        const double Q = -b + z_dir * sqrt(rad);
        v3 o{inc.x + om * dWdX + Q * normal.x, inc.y + om * dWdY + Q * normal.y,
             inc.z + om * 0.0 + Q * normal.z};
        dW = w * mu;
        if (n_in != 1.0) {
            v3 o2;
            if (!refract(o, srf_nrml, 1.0, n_out, o2))
                return PHASE_TIR;
            o = o2;
        }
        out = o;
        return PHASE_OK;
    }
    // ROX_PH_HOLOGRAM, doe.py:375-397
    const int flags = ints_of(ph)[2];
    const v3 normal = unit(srf_nrml);
    v3 ref_dir = unit(v3{pt.x - ph[O_A], pt.y - ph[O_A + 1], pt.z - ph[O_A + 2]});
    if (flags & 1)
        ref_dir = v3{-ref_dir.x, -ref_dir.y, -ref_dir.z};
    const double ref_cosI = dot3(ref_dir, normal);
    v3 obj_dir = unit(v3{pt.x - ph[O_B], pt.y - ph[O_B + 1], pt.z - ph[O_B + 2]});
    if (flags & 2)
        obj_dir = v3{-obj_dir.x, -obj_dir.y, -obj_dir.z};
    const double obj_cosI = dot3(obj_dir, normal);
    const double in_cosI = dot3(in_dir, normal);
    const double mu = wvl / ph[O_REFWL];
    const double b = in_cosI + mu * (obj_cosI - ref_cosI);
    const double refp_cosI = dot3(ref_dir, in_dir);
    const double objp_cosI = dot3(obj_dir, in_dir);
    const double ro_cosI = dot3(ref_dir, obj_dir);
    const double c = mu * (mu * (1.0 - ro_cosI) + (objp_cosI - refp_cosI));
    const double rad = b * b - 2 * c;
    if (rad < 0.0)
        return PHASE_EVANESCENT;
    const double Q = -b + z_dir * sqrt(rad);
    out = v3{in_dir.x + mu * (obj_dir.x - ref_dir.x) + Q * normal.x,
             in_dir.y + mu * (obj_dir.y - ref_dir.y) + Q * normal.y,
             in_dir.z + mu * (obj_dir.z - ref_dir.z) + Q * normal.z};
    dW = 0.;
    return PHASE_OK;
}

}  // namespace rox
