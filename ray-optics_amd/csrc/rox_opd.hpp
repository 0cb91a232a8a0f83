// rox_opd.hpp -- the wave-aberration formulas of the OPD and FAN outputs
#pragma once
#include "rox_math.hpp"
#include "rox_math_fast.hpp"

namespace rox {

// ------------------------------------------------------------------ OPD
// FAST (the tolerance-mode instances): the quotients and the square root of the wave-aberration
// formulas through rcp_f / sqrt_f (~1 ulp) instead of the correctly rounded expansions; the
// operation order is otherwise the reference's.  An OPD is a difference of optical paths of
// O(100) system units: 1e-16 relative on its terms is 1e-14 absolute.
template <bool FAST>
__device__ __forceinline__ double wf_div(double a, double b) { return FAST ? a * rcp_f(b) : a / b; }
template <bool FAST>
__device__ __forceinline__ double wf_sqrt(double x) { return FAST ? sqrt_f(x) : sqrt(x); }

// waveabr.py:117-132 eic_distance
template <bool FAST = false, class P3>
__device__ __forceinline__ double eic_distance(const v3 &p, const v3 &d, P3 p0, P3 d0)
{
    const v3 sd{d.x + d0[0], d.y + d0[1], d.z + d0[2]};
    const v3 dp{p.x - p0[0], p.y - p0[1], p.z - p0[2]};
    return wf_div<FAST>(dot3(sd, dp), 1. + dot3(d, v3{d0[0], d0[1], d0[2]}));
}

// waveabr.py:256-307 wave_abr_full_calc_finite_pup (+ transform.py:234-258)
template <bool FAST = false, class WF>      // rox_wavefront, in whatever address space the launch arguments live
__device__ __forceinline__ double wave_abr_finite_pup(WF &w, const v3 &ray1_p,
                                                      const v3 &ray0_d, const v3 &rayk_p,
                                                      const v3 &rayk_d, double ray_op)
{
    const double e1 = eic_distance<FAST>(ray1_p, ray0_d, w.cr1_p, w.cr0_d);
    const double ekp = eic_distance<FAST>(rayk_p, rayk_d, w.crk_p, w.crk_d);
    v3 b4p = rayk_p, b4d = rayk_d;
    if (w.after_kind != 0) {
        const v3 t{rayk_p.x - w.after_t[0], rayk_p.y - w.after_t[1], rayk_p.z - w.after_t[2]};
        if (w.after_kind == 1) {
            b4p = t;
        } else {
            b4p = rotate(w.after_rt, w.after_order, t);
            b4d = rotate(w.after_rt, w.after_order, rayk_d);
        }
    }
    const double dst = ekp - w.cr_exp_dist;
    const v3 pc{(b4p.x - dst * b4d.x) - w.cr_exp_pt[0], (b4p.y - dst * b4d.y) - w.cr_exp_pt[1],
                (b4p.z - dst * b4d.z) - w.cr_exp_pt[2]};
    const v3 rd{w.ref_dir[0], w.ref_dir[1], w.ref_dir[2]};
    const double R = w.ref_radius;
    // (R is a launch constant: the tolerance mode multiplies by its reciprocal, formed once)
    const double rR = FAST ? rcp_f(R) : 0.0;
    const double F = dot3(rd, b4d) - (FAST ? dot3(b4d, pc) * rR : dot3(b4d, pc) / R);
    const double J = (FAST ? dot3(pc, pc) * rR : dot3(pc, pc) / R) - 2.0 * dot3(rd, pc);
    const double denom = F + w.sign_soln * wf_sqrt<FAST>(F * F + (FAST ? J * rR : J / R));
    const double ep = (denom == 0) ? 0 : wf_div<FAST>(J, denom);
    return -w.n_obj * e1 - ray_op + w.n_img * ekp + w.cr_op - w.n_img * ep;
}

// waveabr.py:356-424 wave_abr_full_calc_inf_ref (ROX_WF_INF_FULL) and its pre-calc /
// calc split :427-488 (ROX_WF_INF_SPLIT); dist_to_shortest_join :178-196,
// ray_dist_to_perp_from_origin :166-175.  Chief-ray-only terms come from the host.
template <bool FAST = false, class WF>
__device__ __forceinline__ double wave_abr_inf_ref(WF &w, const v3 &ray1_p,
                                                   const v3 &ray0_d, const v3 &rayk_p,
                                                   const v3 &rayk_d, const v3 &rayl_p,
                                                   const v3 &rayl_d, double ray_op)
{
    const double e1 = eic_distance<FAST>(ray1_p, ray0_d, w.cr1_p, w.cr0_d);
    v3 p_b4 = rayk_p, d_b4 = rayk_d;
    if (w.last_kind) {
        p_b4 = rotate(w.last_rt, w.last_order, v3{rayk_p.x - w.last_t[0], rayk_p.y - w.last_t[1],
                                                  rayk_p.z - w.last_t[2]});
        d_b4 = rotate(w.last_rt, w.last_order, rayk_d);
    }
    const double op_b4 = dot3(d_b4, v3{-p_b4.x, -p_b4.y, -p_b4.z});
    const v3 p1{w.cr_last_p[0], w.cr_last_p[1], w.cr_last_p[2]};
    const v3 d1{w.cr_last_d[0], w.cr_last_d[1], w.cr_last_d[2]};
    const v3 del_p{rayl_p.x - p1.x, rayl_p.y - p1.y, rayl_p.z - p1.z};
    const v3 n = cross3(d1, rayl_d);
    const double nn = dot3(n, n);
    v3 P1, P2;
    if (nn == 0) {
        const double t2 = dot3(v3{p1.x - rayl_p.x, p1.y - rayl_p.y, p1.z - rayl_p.z}, d1) *
                          dot3(d1, rayl_d);
        P1 = p1;
        P2 = v3{rayl_p.x + t2 * rayl_d.x, rayl_p.y + t2 * rayl_d.y, rayl_p.z + t2 * rayl_d.z};
    } else {
        const double t1 = wf_div<FAST>(dot3(cross3(rayl_d, n), del_p), nn);
        const double t2 = wf_div<FAST>(dot3(cross3(d1, n), del_p), nn);
        P1 = v3{p1.x + t1 * d1.x, p1.y + t1 * d1.y, p1.z + t1 * d1.z};
        P2 = v3{rayl_p.x + t2 * rayl_d.x, rayl_p.y + t2 * rayl_d.y, rayl_p.z + t2 * rayl_d.z};
    }
    const v3 rF0{(P1.x + P2.x) / 2, (P1.y + P2.y) / 2, (P1.z + P2.z) / 2};
    const v3 dcr{w.d_cr_b4[0], w.d_cr_b4[1], w.d_cr_b4[2]};
    const double V_B = ray_op + op_b4;
    const double W0 = V_B - w.v_be +
                      w.n_img * dot3(v3{d_b4.x - dcr.x, d_b4.y - dcr.y, d_b4.z - dcr.z}, rF0);
    const v3 ta{rayl_p.x - w.image_pt[0], rayl_p.y - w.image_pt[1], rayl_p.z - w.image_pt[2]};
    const double dbc = dot3(d_b4, dcr);
    const double numer = dot3(v3{dcr.x - d_b4.x * dbc, dcr.y - d_b4.y * dbc, dcr.z - d_b4.z * dbc}, ta);
    const double denom = 1 + dot3(d_b4, dcr);
    if (w.kind == ROX_WF_INF_SPLIT) {
        const double pre_opd = -w.n_obj * e1 - W0;
        const double W_inf = wf_div<FAST>(w.n_img * numer, denom);
        return pre_opd - W_inf;
    }
    const double W_inf = W0 + wf_div<FAST>(w.n_img * numer, denom);
    return -w.n_obj * e1 - W_inf;
}

}  // namespace rox
