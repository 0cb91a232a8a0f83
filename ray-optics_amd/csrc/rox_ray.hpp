// rox_ray.hpp -- one ray through the surface table: the packet stores, the workgroup context and
// the three per-ray loops (exact FULL / probe, exact reduced outputs, tolerance mode); the ray
// start from a pupil point.
#pragma once
#include <cstddef>
#include <cstdint>

#include "rox_args.hpp"
#include "rox_math.hpp"
#include "rox_math_fast.hpp"
#include "rox_phase.hpp"
#include "rox_profiles.hpp"

namespace rox {

// ------------------------------------------------------------------ stores
// One packet component of ray r lives at seg[(slot*10 + c)*ld + r].  The
// (slot, c) part is wave-uniform, so it goes into an SGPR base; the ray part
// is one 32-bit byte offset per lane computed once per ray: the store is
// `global_store_dwordx2 v_off, v_data, s[base:base+1]` with no per-store
// 64-bit VALU address arithmetic.  (The host splits batches longer than 2^28
// rays into several launches so that the lane offset always fits 32 bits.)
struct SegOut {
    char *base;         // uniform: seg (already offset to this launch's first ray)
    int64_t row_bytes;  // uniform: ld * 8
    uint32_t voff;      // per lane: (r - first ray of the launch) * 8 < 2^32
    __device__ __forceinline__ void put(int slot, int c, double v) const
    {
        char *b = base + ((int64_t)slot * ROX_SEG_DOUBLES + c) * row_bytes;
        double *p = reinterpret_cast<double *>(b + (size_t)voff);
        __builtin_nontemporal_store(v, p);      // (against a plain store: FULL 236 us vs 257 us)
    }
    __device__ __forceinline__ void pdn(int slot, const v3 &p, const v3 &d, const v3 &n) const
    {
        put(slot, 0, p.x); put(slot, 1, p.y); put(slot, 2, p.z);
        put(slot, 3, d.x); put(slot, 4, d.y); put(slot, 5, d.z);
        put(slot, 7, n.x); put(slot, 8, n.y); put(slot, 9, n.z);
    }
    __device__ __forceinline__ void dst(int slot, double v) const { put(slot, 6, v); }
};

// the workgroup's view of the surface table (LDS) + the launch options
template <class TP>
struct CtxT {
    TP tbl;                 // [N][kRowDoubles]: LDS (tblp), or global through scalar loads (ctblp, F_GTAB)
    tblp ntab;              // [N] (one wavelength) or [W][N] (per-ray wavelengths)
    TP phc;                 // [N][kPhaseConsts] or [W][N][kPhaseConsts]; FEAT & F_PHASE only
    tblp aplthr;            // F_GTAB: [N][ROX_MAX_AP] circular clear-aperture thresholds; else nullptr
    tblp wvls;              // [W]
    tbli slot, nslots_before;
    tblp apthr;             // [N] sqrt_le_threshold(max_aperture + fuzz)
    tblp mu;                // F_FAST only: per wavelength row [N] mu, [N] mu^2, [N] sg (interact_f)
    int N;
    bool check_ap, intersect_obj, filter_ph;
    int first_surf, last_surf;
    double eps, fuzz;
    int probe_surf;         // MODE_PROBE
};
typedef CtxT<tblp> Ctx;

// what a traced ray leaves in registers for the epilogues
struct RayEnd {
    int status, fail_surf;
    double opl, phs;        // op_delta = phs + opl on success (raytrace.py:208, 261)
    v3 inc, ad, nrm;        // ray[-1]
    v3 ray1_p, rayk_p, rayk_d;   // OPD mode: ray[1].p, ray[-2].{p, d}
    v3 probe_p;             // MODE_PROBE: ray[probe_surf].p
};

// ------------------------------------------------------------------ one ray
// raytrace.py:83-264 trace_raw for one lane, for the two consumers that need the loop in the
// reference's own shape: FULL packets (segment stores, the late append of :185-191, phantom
// filtering) and the searches' MODE_PROBE.  The reduced-output modes have trace_ray_reduced()
// below, the tolerance-mode instances trace_ray_fast().  wi = wavelength index of the ray
// (wave-uniform unless PER_RAY_WVL).
// `live` = false for the lanes past the end of the batch: they trace nothing.
// kSync (FULL packets only): the waves of a workgroup meet at a barrier before
// every surface, so that the workgroup writes whole [segment] rows together;
// every wave must then reach every barrier: failed lanes idle instead of leaving.
#define ROX_LEAVE if (kSync) continue; else break
template <int OUT_MODE, bool PER_RAY_WVL, int FEAT, class CTX>
__device__ __forceinline__ void trace_ray(const CTX &c, const SegOut &so, const v3 &pt0,
                                          const v3 &dir0, int wi, bool live, RayEnd &e)
{
    static_assert(OUT_MODE == ROX_OUT_FULL || OUT_MODE == MODE_PROBE, "FULL packets and the search probe only");
    constexpr int O_CV = offsetof(rox_surface, cv) / 8, O_CC = offsetof(rox_surface, cc) / 8,
                  O_EC = offsetof(rox_surface, ec) / 8, O_CR = offsetof(rox_surface, cR) / 8,
                  O_COEF = offsetof(rox_surface, coefs) / 8,
                  O_RT = offsetof(rox_surface, rt) / 8, O_T = offsetof(rox_surface, t) / 8,
                  O_ZDIR = offsetof(rox_surface, z_dir) / 8,
                  O_PH = offsetof(rox_surface, ph) / 8;
    constexpr bool kPoly = (FEAT & F_POLY) != 0;
    constexpr bool kSync = OUT_MODE == ROX_OUT_FULL && (kPoly ? ROX_WG_SYNC_POLY : ROX_WG_SYNC);
    constexpr bool kIdentRt = ROX_IDENT_RT && (OUT_MODE != ROX_OUT_FULL || (kPoly && ROX_IDENT_RT_FULL_POLY));
    const int N = c.N;
    const auto tbl = c.tbl;
    tblp nwl = PER_RAY_WVL ? c.ntab + (size_t)wi * N : c.ntab;
#define SLOT(s) ((FEAT & F_PHFILT) ? c.slot[s] : (s))
#define NSLOTS_BEFORE(s) ((FEAT & F_PHFILT) ? c.nslots_before[s] : (s))
    // without phantom filtering segment k of a packet is interface k

    // ---- object surface, raytrace.py:145-158 -----------------------------
    int status = live ? ROX_OK : 255, fail_surf = -1;
    v3 bp, bn, bd = dir0;               // before_pt, before_normal, before_dir
    int b4_mode = ROX_DUMMY;
    if (live) {
        const auto row = tbl;
        if (c.intersect_obj) {
            const int2 mp{ints_of(row)[0], ints_of(row)[1]};      // mode, profile
            b4_mode = mp.x;
            double s_;
            v3 df;
            bool ok;
            if ((FEAT & F_PHASE) && mp.y == ROX_THINLENS) {     // thinlens.py:131-134
                s_ = -pt0.z / dir0.z;
                bp = v3{pt0.x + s_ * dir0.x, pt0.y + s_ * dir0.y, pt0.z + s_ * dir0.z};
                ok = true;
            } else if (!kPoly || mp.y <= ROX_CONIC) {
                ok = quadric_hit(mp.y == ROX_CONIC, row[O_CV], row[O_CC], row[O_EC], pt0, dir0,
                                 row[O_ZDIR], s_, bp);
                const double k = (mp.y == ROX_CONIC) ? (row[O_CC] + 1.0) * row[O_CV] : row[O_CV];
                const double ncv = row[O_CR];       // -cv as df forms it (roxtrace.hip, device row)
                df = v3{ncv * bp.x, ncv * bp.y, 1.0 - k * bp.z};
            } else {
                ok = newton_hit<FEAT>(mp.y, row[O_CV], row[O_CC] + 1.0, row[O_EC], row[O_CR],
                                      ints_of(row)[2], row + O_COEF, pt0, dir0, c.eps, s_, bp, df);
            }
            if (!ok) {              // raised outside the try block: no packet
                status = ROX_MISSED_SURFACE;
                fail_surf = 0;
            } else if ((FEAT & F_PHASE) && mp.y == ROX_THINLENS) {
                bn = v3{0., 0., 1.};
            } else {
                bn = unit(df);
            }
        } else {
            bp = pt0;
            bn = v3{0., 0., 1.};
        }
    }
    double z_dir_before = tbl[O_ZDIR];
    double opl = 0.0, phs = 0.0;
    double acc_dst = 0.0;           // dst of the most recently appended segment
    int acc_slot = 0;
    v3 inc{0, 0, 0}, nrm{0, 0, 0}, ad = dir0;
    e.ray1_p = e.rayk_p = e.rayk_d = e.probe_p = v3{0, 0, 0};
    if (OUT_MODE == MODE_PROBE && c.probe_surf == 0)
        e.probe_p = bp;
    if (OUT_MODE == ROX_OUT_FULL && status == ROX_OK)
        so.pdn(0, bp, bd, bn);

    // ---- remaining surfaces, raytrace.py:164-229 -------------------------
    for (int surf = 1; surf < N && (kSync || status == ROX_OK); ++surf) {
        if (kSync) {
            __builtin_amdgcn_s_barrier();
            if (status != ROX_OK)
                continue;
        }
        const auto prow = tbl + (size_t)(surf - 1) * kRowDoubles;     // `before`
        const auto row = tbl + (size_t)surf * kRowDoubles;             // `after`
        const int mode = ints_of(row)[0], prof = ints_of(row)[1];
        const double cv = row[O_CV];
        const bool thin = (FEAT & F_PHASE) && prof == ROX_THINLENS;

        // :170-174 transform to the new vertex frame, closest approach
        const int rt_order = ints_of(prow)[4];
        const v3 dp{bp.x - prow[O_T], bp.y - prow[O_T + 1], bp.z - prow[O_T + 2]};
        v3 b4p, b4d;
        // rt exactly the identity (flagged on the device row when the system is created): each
        // dgemv chain fma(0, z, fma(0, y, fma(1, x, 0.0))) is x + 0.0 for finite operands in
        // either column order (-0 becomes +0 as in the chain).  A non-finite component would
        // turn the other rows into NaN through 0 * inf, so the short cut is taken only when
        // every active lane's six components are finite (their sum is: a conservative test).
        // (kIdentRt: the probe, and FULL packets of the Newton instances; in the other FULL
        // kernels, which are bound by their packet stores, the extra branch measured 2 % slower)
        if (kIdentRt && (ints_of(prow)[5] & 2) != 0 &&
            wave_all(__builtin_isfinite(((dp.x + dp.y) + dp.z) + ((bd.x + bd.y) + bd.z)))) {
            b4p = v3{dp.x + 0.0, dp.y + 0.0, dp.z + 0.0};
            b4d = v3{bd.x + 0.0, bd.y + 0.0, bd.z + 0.0};
        } else {
            b4p = rotate(prow + O_RT, rt_order, dp);
            b4d = rotate(prow + O_RT, rt_order, bd);
        }
        const double pp_dst = -dot3(b4p, b4d);
        const v3 pp{b4p.x + pp_dst * b4d.x, b4p.y + pp_dst * b4d.y, b4p.z + pp_dst * b4d.z};

        // :181-183 intersect
        double s;
        v3 df;
        bool ok;
        if (thin) {
            s = -pp.z / b4d.z;
            inc = v3{pp.x + s * b4d.x, pp.y + s * b4d.y, pp.z + s * b4d.z};
            ok = true;
        } else if (!kPoly || prof <= ROX_CONIC) {
            ok = quadric_hit(prof == ROX_CONIC, cv, row[O_CC], row[O_EC], pp, b4d,
                             z_dir_before, s, inc);
        } else {
            ok = newton_hit<FEAT>(prof, cv, row[O_CC] + 1.0, row[O_EC], row[O_CR],
                                  ints_of(row)[2], row + O_COEF, pp, b4d, c.eps, s, inc, df);
        }
        const bool b4_filtered = c.filter_ph && (b4_mode == ROX_PHANTOM);
        if (!ok) {                                  // :231-237
            status = ROX_MISSED_SURFACE;
            fail_surf = surf;
            if (OUT_MODE == ROX_OUT_FULL) {
                const int sl = b4_filtered ? NSLOTS_BEFORE(surf - 1) : SLOT(surf - 1);
                if (b4_filtered)
                    so.pdn(sl, bp, bd, bn);
                so.dst(sl, pp_dst);
            }
            ROX_LEAVE;
        }
        const double dst_b4 = pp_dst + s;
        // :185-191 the *previous* segment is completed only now
        if (b4_filtered) {
            acc_dst += dst_b4;
        } else {
            acc_dst = dst_b4;
            acc_slot = SLOT(surf - 1);
        }
        if (OUT_MODE == ROX_OUT_FULL)
            so.dst(acc_slot, acc_dst);
        // (without phantom filtering the record of this interface -- complete or partial -- holds
        // inc_pt and the normal in slot `surf` whatever happens next: stored as they become known)
        constexpr bool kEarly = OUT_MODE == ROX_OUT_FULL && ROX_FULL_EARLY_STORES && !(FEAT & F_PHFILT);
        if (kEarly) {
            so.put(surf, 0, inc.x); so.put(surf, 1, inc.y); so.put(surf, 2, inc.z);
        }

        // :193-194 (in_gap_range, :123-132)
        {
            const int g = surf - 1;
            const bool in_gap = !(c.last_surf >= 0 && c.first_surf == c.last_surf) &&
                                g >= c.first_surf && (c.last_surf < 0 || g < c.last_surf);
            if (in_gap)
                opl += nwl[surf - 1] * dst_b4;
        }

        // :196 normal = normalize(df(inc_pt))
        if (thin) {
            nrm = v3{0., 0., 1.};
        } else {
            if (!kPoly || prof <= ROX_CONIC) {
                const double k = (prof == ROX_CONIC) ? (row[O_CC] + 1.0) * cv : cv;
                const double ncv = row[O_CR];       // -cv as df forms it (roxtrace.hip, device row)
                df = v3{ncv * inc.x, ncv * inc.y, 1.0 - k * inc.z};
            }
            nrm = unit(df);
        }
        if (kEarly) {
            so.put(surf, 7, nrm.x); so.put(surf, 8, nrm.y); so.put(surf, 9, nrm.z);
        }

        // :198-202 aperture test (in_surface_range, :134-142)
        if (c.check_ap && surf >= c.first_surf && (c.last_surf < 0 || surf <= c.last_surf) &&
            mode != ROX_PHANTOM) {
            const int n_ap = (FEAT & F_APLIST) ? ints_of(row)[3] : 0;
            const bool in = n_ap > 0
                ? inside_aperture_list(row, n_ap, inc.x, inc.y, c.fuzz,
                                       c.aplthr ? c.aplthr + (size_t)surf * ROX_MAX_AP : nullptr)
                : (inc.x * inc.x + inc.y * inc.y) <= c.apthr[surf];   // sqrt-free, see above
            if (!in)
                status = ROX_BLOCKED;               // :247-251
        }

        // :205-221 phase element, or refract / reflect / pass through
        if (status == ROX_OK) {
            if ((FEAT & F_PHASE) && ints_of(row + O_PH)[0] != ROX_PH_NONE) {
                double dW = 0.0;
                const auto pc = c.phc + ((PER_RAY_WVL ? (size_t)wi * N : 0) + surf) * kPhaseConsts;
                const int rc = apply_phase(row + O_PH, pc, inc, b4d, nrm, z_dir_before,
                                           c.wvls[wi], nwl[surf - 1], nwl[surf], mode, ad, dW);
                if (rc == PHASE_OK)
                    phs += dW;
                else
                    status = (rc == PHASE_TIR) ? ROX_TIR : ROX_EVANESCENT;    // :253-257
            } else if (mode == ROX_REFLECT) {
                ad = mirror(b4d, nrm);
            } else if (mode == ROX_TRANSMIT) {
                if (!refract(b4d, nrm, nwl[surf - 1], nwl[surf], ad))
                    status = ROX_TIR;               // :239-245
            } else {
                ad = b4d;
            }
        }
        if (status != ROX_OK) {
            // partial packet: [inc_pt, before_dir, 0.0, normal] in the next slot
            fail_surf = surf;
            if (OUT_MODE == ROX_OUT_FULL) {
                const int sl = NSLOTS_BEFORE(surf);
                if (kEarly) {
                    so.put(sl, 3, bd.x); so.put(sl, 4, bd.y); so.put(sl, 5, bd.z);
                } else {
                    so.pdn(sl, inc, bd, nrm);
                }
                so.dst(sl, 0.0);
            }
            ROX_LEAVE;
        }

        if (OUT_MODE == MODE_PROBE && surf == c.probe_surf)
            e.probe_p = inc;
        // :223-229 roll
        bp = inc; bd = ad;
        if (FEAT & F_PHFILT)
            bn = nrm;           // only a filtered phantom's late append needs it
        z_dir_before = row[O_ZDIR];
        b4_mode = mode;
        if (OUT_MODE == ROX_OUT_FULL) {
            const bool cur_filtered = c.filter_ph && (mode == ROX_PHANTOM) && surf < N - 1;
            if (kEarly) {
                so.put(surf, 3, ad.x); so.put(surf, 4, ad.y); so.put(surf, 5, ad.z);
            } else if (!cur_filtered) {
                so.pdn(SLOT(surf), inc, ad, nrm);
            }
        }
    }
    if (OUT_MODE == ROX_OUT_FULL && status == ROX_OK)   // :259-262
        so.dst(SLOT(N - 1), 0.0);
#undef SLOT
#undef NSLOTS_BEFORE
#undef ROX_LEAVE
    e.status = status;
    e.fail_surf = fail_surf;
    e.opl = opl;
    e.phs = phs;
    e.inc = inc; e.ad = ad; e.nrm = nrm;
}

// ------------------------------------------------------------------ one ray, reduced outputs, exact
// The loop of the reduced-output modes (LAST, HITS, packed hits, OPD, FAN and the through-focus
// kernel) of the exact instances, in the shape the tolerance-mode kernels showed to pay
// (trace_ray_fast below).  These modes ran trace_ray() until round 6 (HITS 110.6 -> 104.8 us double
// Gauss, 386 -> 362 lithography lens, 307 -> 289 Nikkor; EXPERIMENTS.md); the arithmetic is trace_ray()'s,
// operation for operation -- so every bit of every output is the same -- but a missed surface, a
// blocked ray or a total internal reflection is a FLAG the iteration ends on, not a way out of
// the middle of it.  The operations behind a raised flag run on (on NaN where a radicand was
// negative) in lanes nobody reads any more: no saved exec masks inside the iteration, no
// register copies where paths meet, and the incidence point / direction are the loop-carried
// before_pt / before_dir themselves.  FULL packets (segment stores, the late append of
// raytrace.py:185-191, phantom filtering) and MODE_PROBE stay with trace_ray().  (Its straight-line
// intersection is rox_profiles.hpp quadric_hit_sl().)

// raytrace.py:19-30 as refract() computes it, without the early exit (false = TIR, out is NaN)
__device__ __forceinline__ bool refract_sl(const v3 &d, const v3 &nrm, double n_in, double n_out, v3 &out)
{
    const double nlen = slim_sqrt(dot3(nrm, nrm));
    const double cosI = dot3(d, nrm) / nlen;
    const double sin2 = 1.0 - cosI * cosI;
    const double rad = n_out * n_out - n_in * n_in * sin2;
    const double n_cosIp = copysign(slim_sqrt(rad), cosI);
    const double alpha = n_cosIp - n_in * cosI;
    const v3 num{n_in * d.x + alpha * nrm.x, n_in * d.y + alpha * nrm.y, n_in * d.z + alpha * nrm.z};
    out = slim_div3(num, n_out);
    return !(rad < 0.0);
}

template <int OUT_MODE, bool PER_RAY_WVL, int FEAT, class CTX>
__device__ __forceinline__ void trace_ray_reduced(const CTX &c, const v3 &pt0, const v3 &dir0, int wi,
                                                  bool live, RayEnd &e)
{
    static_assert(OUT_MODE != ROX_OUT_FULL && OUT_MODE != MODE_PROBE, "reduced-output modes only");
    constexpr int O_CV = offsetof(rox_surface, cv) / 8, O_CC = offsetof(rox_surface, cc) / 8,
                  O_EC = offsetof(rox_surface, ec) / 8, O_CR = offsetof(rox_surface, cR) / 8,
                  O_COEF = offsetof(rox_surface, coefs) / 8,
                  O_RT = offsetof(rox_surface, rt) / 8, O_T = offsetof(rox_surface, t) / 8,
                  O_ZDIR = offsetof(rox_surface, z_dir) / 8,
                  O_PH = offsetof(rox_surface, ph) / 8;
    constexpr bool kPoly = (FEAT & F_POLY) != 0;
    const int N = c.N;
    const auto tbl = c.tbl;
    tblp nwl = PER_RAY_WVL ? c.ntab + (size_t)wi * N : c.ntab;

    // ---- object surface, raytrace.py:145-158 (before_normal is only ever stored: not needed)
    int status = live ? ROX_OK : 255, fail_surf = -1;
    v3 inc = pt0, ad = dir0, nrm{0, 0, 0};
    if (live && c.intersect_obj) {
        const auto row = tbl;
        const int prof = ints_of(row)[1];
        double s_;
        v3 df, bp;
        bool ok;
        if ((FEAT & F_PHASE) && prof == ROX_THINLENS) {     // thinlens.py:131-134
            s_ = -pt0.z / dir0.z;
            bp = v3{pt0.x + s_ * dir0.x, pt0.y + s_ * dir0.y, pt0.z + s_ * dir0.z};
            ok = true;
        } else if (!kPoly || prof <= ROX_CONIC) {
            ok = quadric_hit(prof == ROX_CONIC, row[O_CV], row[O_CC], row[O_EC], pt0, dir0,
                             row[O_ZDIR], s_, bp);
        } else {
            ok = newton_hit<FEAT>(prof, row[O_CV], row[O_CC] + 1.0, row[O_EC], row[O_CR],
                                  ints_of(row)[2], row + O_COEF, pt0, dir0, c.eps, s_, bp, df);
        }
        if (!ok) {                          // raised outside the try block: no packet
            status = ROX_MISSED_SURFACE;
            fail_surf = 0;
        } else {
            inc = bp;
        }
    }
    double z_dir_before = tbl[O_ZDIR];
    double opl = 0.0, phs = 0.0;
    e.ray1_p = e.rayk_p = e.rayk_d = e.probe_p = v3{0, 0, 0};

    // ---- remaining surfaces, raytrace.py:164-229
    for (int surf = 1; surf < N && status == ROX_OK; ++surf) {
        const auto prow = tbl + (size_t)(surf - 1) * kRowDoubles;     // `before`
        const auto row = tbl + (size_t)surf * kRowDoubles;             // `after`
        const int mode = ints_of(row)[0], prof = ints_of(row)[1];
        const double cv = row[O_CV];
        const bool thin = (FEAT & F_PHASE) && prof == ROX_THINLENS;

        // :170-174 transform to the new vertex frame, closest approach (trace_ray(): the identity
        // short cut under the same finiteness test, the dgemv chains otherwise)
        const int rt_order = ints_of(prow)[4];
        const v3 dp{inc.x - prow[O_T], inc.y - prow[O_T + 1], inc.z - prow[O_T + 2]};
        v3 b4p, b4d;
        if (ROX_IDENT_RT && (ints_of(prow)[5] & 2) != 0 &&
            wave_all(__builtin_isfinite(((dp.x + dp.y) + dp.z) + ((ad.x + ad.y) + ad.z)))) {
            b4p = v3{dp.x + 0.0, dp.y + 0.0, dp.z + 0.0};
            b4d = v3{ad.x + 0.0, ad.y + 0.0, ad.z + 0.0};
        } else {
            b4p = rotate(prow + O_RT, rt_order, dp);
            b4d = rotate(prow + O_RT, rt_order, ad);
        }
        const double pp_dst = -dot3(b4p, b4d);
        const v3 pp{b4p.x + pp_dst * b4d.x, b4p.y + pp_dst * b4d.y, b4p.z + pp_dst * b4d.z};

        // :181-183 intersect
        double s;
        v3 df;
        bool hit;
        if (thin) {
            s = -pp.z / b4d.z;
            inc = v3{pp.x + s * b4d.x, pp.y + s * b4d.y, pp.z + s * b4d.z};
            hit = true;
        } else if (!kPoly || prof <= ROX_CONIC) {
            hit = quadric_hit_sl(prof == ROX_CONIC, cv, row[O_CC], row[O_EC], pp, b4d, z_dir_before, s, inc);
        } else {
            hit = newton_hit<FEAT>(prof, cv, row[O_CC] + 1.0, row[O_EC], row[O_CR],
                                   ints_of(row)[2], row + O_COEF, pp, b4d, c.eps, s, inc, df);
        }
        // :193-194 (in_gap_range, :123-132); a ray that missed keeps the path it had (:231-237)
        {
            const int g = surf - 1;
            const bool in_gap = !(c.last_surf >= 0 && c.first_surf == c.last_surf) &&
                                g >= c.first_surf && (c.last_surf < 0 || g < c.last_surf);
            if (in_gap) {
                const double dst_b4 = pp_dst + s;
                const double opl_new = opl + nwl[surf - 1] * dst_b4;
                opl = hit ? opl_new : opl;
            }
        }

        // :196 normal = normalize(df(inc_pt))
        if (thin) {
            nrm = v3{0., 0., 1.};
        } else {
            if (!kPoly || prof <= ROX_CONIC) {
                const double k = (prof == ROX_CONIC) ? (row[O_CC] + 1.0) * cv : cv;
                const double ncv = row[O_CR];       // -cv as df forms it (roxtrace.hip, device row)
                df = v3{ncv * inc.x, ncv * inc.y, 1.0 - k * inc.z};
            }
            nrm = unit(df);
        }

        // :198-202 aperture test (in_surface_range, :134-142)
        bool blocked = false;
        if (c.check_ap && surf >= c.first_surf && (c.last_surf < 0 || surf <= c.last_surf) &&
            mode != ROX_PHANTOM) {
            const int n_ap = (FEAT & F_APLIST) ? ints_of(row)[3] : 0;
            blocked = n_ap > 0
                ? !inside_aperture_list(row, n_ap, inc.x, inc.y, c.fuzz,
                                        c.aplthr ? c.aplthr + (size_t)surf * ROX_MAX_AP : nullptr)
                : !((inc.x * inc.x + inc.y * inc.y) <= c.apthr[surf]);
        }

        // :205-221 phase element, or refract / reflect / pass through (wave-uniform branches)
        bool tir = false;
        int ph_fail = ROX_OK;
        if ((FEAT & F_PHASE) && ints_of(row + O_PH)[0] != ROX_PH_NONE) {
            if (hit && !blocked) {
                double dW = 0.0;
                const auto pc = c.phc + ((PER_RAY_WVL ? (size_t)wi * N : 0) + surf) * kPhaseConsts;
                v3 out = ad;
                const int rc = apply_phase(row + O_PH, pc, inc, b4d, nrm, z_dir_before,
                                           c.wvls[wi], nwl[surf - 1], nwl[surf], mode, out, dW);
                ad = out;
                if (rc == PHASE_OK)
                    phs += dW;
                else
                    ph_fail = (rc == PHASE_TIR) ? ROX_TIR : ROX_EVANESCENT;       // :253-257
            }
        } else if (mode == ROX_REFLECT) {
            ad = mirror(b4d, nrm);
        } else if (mode == ROX_TRANSMIT) {
            tir = !refract_sl(b4d, nrm, nwl[surf - 1], nwl[surf], ad);              // :239-245
        } else {
            ad = b4d;
        }
        // :231-257 the first failure in the reference's order: miss, blocked, TIR / evanescent
        const int st = !hit ? (int)ROX_MISSED_SURFACE
                     : blocked ? (int)ROX_BLOCKED
                     : tir ? (int)ROX_TIR : ph_fail;
        if (st != ROX_OK) {
            status = st;
            fail_surf = surf;
            break;
        }
        if (OUT_MODE == ROX_OUT_OPD || OUT_MODE == ROX_OUT_FAN) {
            if (surf == 1)
                e.ray1_p = inc;
            if (surf == N - 2) {
                e.rayk_p = inc;
                e.rayk_d = ad;
            }
        }
        z_dir_before = row[O_ZDIR];
    }
    e.status = status;
    e.fail_surf = fail_surf;
    e.opl = opl;
    e.phs = phs;
    e.inc = inc; e.ad = ad; e.nrm = nrm;
}

// ------------------------------------------------------------------ one ray, tolerance mode
// trace_ray() for the F_FAST instances: the same loop (raytrace.py:83-264) over the same table,
// reduced-output modes only -- no packet stores, hence no segment bookkeeping -- with the
// arithmetic of the section "tolerance mode" above.  c.mu / c.mu2 = n_in / n_out and its square
// per interface, staged by the workgroup.
template <int OUT_MODE, bool PER_RAY_WVL, int FEAT, class CTX>
__device__ __forceinline__ void trace_ray_fast(const CTX &c, const SegOut &so, const v3 &pt0,
                                               const v3 &dir0, int wi, bool live, RayEnd &e)
{
    static_assert(OUT_MODE != MODE_PROBE, "the searches keep the exact arithmetic");
    // FULL packets (round 6): the segment stores of trace_ray() -- [p, d, dst, normal] per
    // interface, the distance of a segment known only at the next intersection, the partial
    // record [inc_pt, before_dir, 0.0, normal] where a ray is blocked or totally reflected -- in
    // this loop.  Without phantom filtering (the host sends ROX_FILTER_PHANTOMS launches to the
    // exact kernels): segment k is interface k.  The workgroup's waves meet at a barrier before
    // every interface as in trace_ray(), so every wave runs every iteration.
    constexpr bool kFull = OUT_MODE == ROX_OUT_FULL;
    constexpr int O_CV = offsetof(rox_surface, cv) / 8, O_CC = offsetof(rox_surface, cc) / 8,
                  O_EC = offsetof(rox_surface, ec) / 8, O_CR = offsetof(rox_surface, cR) / 8,
                  O_COEF = offsetof(rox_surface, coefs) / 8,
                  O_RT = offsetof(rox_surface, rt) / 8, O_T = offsetof(rox_surface, t) / 8,
                  O_ZDIR = offsetof(rox_surface, z_dir) / 8,
                  O_PH = offsetof(rox_surface, ph) / 8;
    constexpr bool kPoly = (FEAT & F_POLY) != 0;
    constexpr bool kSync = kFull && (kPoly ? ROX_WG_SYNC_POLY : ROX_WG_SYNC);
    const int N = c.N;
    const auto tbl = c.tbl;
    tblp nwl = PER_RAY_WVL ? c.ntab + (size_t)wi * N : c.ntab;
    tblp muw = PER_RAY_WVL ? c.mu + (size_t)wi * 3 * N : c.mu;      // [N] mu, [N] mu^2, [N] sg

    // The object surface and the transfer to interface 1 keep the REFERENCE's arithmetic
    // (trace_ray()'s operations in its order, correctly rounded): an object at infinity sits
    // 1e10 system units away (rayoptics' convention), so `before_pt - t`, `-dot(b4_pt, b4_dir)`
    // and `b4_pt + pp_dst * b4_dir` cancel numbers of that size down to the lens' own, and what
    // is left carries ~1e-6 of rounding that depends on the operation order.  That noise is part
    // of the reference's answer; any other order lands 1e-7 away from it.  Once per ray.
    int status = live ? ROX_OK : 255, fail_surf = -1;
    v3 bp = pt0, bd = dir0;
    v3 pp1{0, 0, 0}, b4d1 = dir0;
    double pp_dst1 = 0.0;
    if (live) {
        const auto row = tbl;
        v3 bn{0., 0., 1.};
        if (c.intersect_obj) {                  // raytrace.py:145-158 (the normal: FULL packets only)
            const int prof = ints_of(row)[1];
            double s_;
            v3 df{0., 0., 1.};
            bool ok;
            if ((FEAT & F_PHASE) && prof == ROX_THINLENS) {
                s_ = -pt0.z / dir0.z;
                bp = v3{pt0.x + s_ * dir0.x, pt0.y + s_ * dir0.y, pt0.z + s_ * dir0.z};
                ok = true;
            } else if (!kPoly || prof <= ROX_CONIC) {
                ok = quadric_hit(prof == ROX_CONIC, row[O_CV], row[O_CC], row[O_EC], pt0, dir0,
                                 row[O_ZDIR], s_, bp);
                if (kFull) {
                    const double k = (prof == ROX_CONIC) ? (row[O_CC] + 1.0) * row[O_CV] : row[O_CV];
                    df = v3{row[O_CR] * bp.x, row[O_CR] * bp.y, 1.0 - k * bp.z};
                }
            } else {
                // (an aspheric OBJECT surface -- never at infinity -- takes the tolerance-mode
                // iteration: the exact one would set the register budget of the whole kernel)
                ok = newton_hit_f<FEAT>(prof, row[O_CV], row[O_CC] + 1.0, row[O_EC], row[O_CR],
                                        ints_of(row)[2], row + O_COEF, pt0, dir0, c.eps, s_, bp, df);
            }
            if (!ok) {
                status = ROX_MISSED_SURFACE;
                fail_surf = 0;
            } else if (kFull && !((FEAT & F_PHASE) && prof == ROX_THINLENS)) {
                bn = unit_f(df);
            }
        }
        if (kFull && status == ROX_OK)
            so.pdn(0, bp, bd, bn);
        const v3 dp{bp.x - row[O_T], bp.y - row[O_T + 1], bp.z - row[O_T + 2]};
        const v3 b4p = rotate(row + O_RT, ints_of(row)[4], dp);
        b4d1 = rotate(row + O_RT, ints_of(row)[4], bd);
        pp_dst1 = -dot3(b4p, b4d1);
        pp1 = v3{b4p.x + pp_dst1 * b4d1.x, b4p.y + pp_dst1 * b4d1.y, b4p.z + pp_dst1 * b4d1.z};
    }
    double z_dir_before = tbl[O_ZDIR];
    double opl = 0.0, phs = 0.0;
    // The loop body is straight-line per lane: a missed surface, a blocked ray or a total
    // internal reflection is a FLAG -- the arithmetic behind it runs on (NaN for a negative
    // radicand), and the iteration ends with one status select and one exit test.  `inc` and
    // `ad` are the loop-carried point and direction themselves (the reference's before_pt /
    // before_dir): a lane that fails leaves with values nobody reads (every consumer asks its
    // status first), so nothing has to be copied aside for it.
    v3 inc = bp, nrm{0, 0, 0}, ad = dir0;
    e.ray1_p = e.rayk_p = e.rayk_d = e.probe_p = v3{0, 0, 0};

    // one interface, from the closest approach `pp` (at distance pp_dst along b4d from the previous
    // intersection) on; false = the ray ends here.  Inlined twice: for interface 1, whose transfer
    // was made above in the reference's arithmetic, and in the loop -- so that the three vectors of
    // that first transfer are not carried, 14 registers wide, through every later interface.
    auto interface = [&](const int surf, const v3 &pp, const v3 &b4d, const double pp_dst)
        __attribute__((always_inline)) -> bool {
        const auto row = tbl + (size_t)surf * kRowDoubles;
        const int mode = ints_of(row)[0], prof = ints_of(row)[1];
        const double cv = row[O_CV];
        const bool thin = (FEAT & F_PHASE) && prof == ROX_THINLENS;
        const v3 bd0 = ad;          // before_dir in the previous frame (FULL: a partial record stores it)

        // :181-183 intersect
        double s;
        v3 df;
        bool hit;
        if (thin) {
            s = -pp.z * rcp_f(b4d.z);
            inc = v3{fma(s, b4d.x, pp.x), fma(s, b4d.y, pp.y), fma(s, b4d.z, pp.z)};
            hit = true;
        } else if (!kPoly || prof <= ROX_CONIC) {
            hit = quadric_hit_f(prof == ROX_CONIC, cv, row[O_CC], row[O_EC], pp, b4d, z_dir_before, s, inc);
        } else {
            hit = newton_hit_f<FEAT>(prof, cv, row[O_CC] + 1.0, row[O_EC], row[O_CR],
                                     ints_of(row)[2], row + O_COEF, pp, b4d, c.eps, s, inc, df);
        }
        // :193-194 (in_gap_range, :123-132); a ray that missed keeps the path it had (:231-237)
        {
            const int g = surf - 1;
            const bool in_gap = !(c.last_surf >= 0 && c.first_surf == c.last_surf) &&
                                g >= c.first_surf && (c.last_surf < 0 || g < c.last_surf);
            if (in_gap) {
                const double opl_new = fma(nwl[surf - 1], pp_dst + s, opl);
                opl = hit ? opl_new : opl;
            }
        }
        // :185-191 the previous segment is completed only now (:231-237: up to the closest
        // approach where the surface was missed)
        constexpr bool kEarly = kFull && ROX_FULL_EARLY_STORES;
        if (kFull)
            so.dst(surf - 1, hit ? pp_dst + s : pp_dst);
        if (kEarly && hit) {
            so.put(surf, 0, inc.x); so.put(surf, 1, inc.y); so.put(surf, 2, inc.z);
        }

        // :196 normal = normalize(df(inc_pt)); a sphere's gradient has unit length on the sphere
        if (thin) {
            nrm = v3{0., 0., 1.};
        } else if (!kPoly || prof <= ROX_CONIC) {
            const double k = (prof == ROX_CONIC) ? (row[O_CC] + 1.0) * cv : cv;     // (wave-uniform)
            nrm = v3{-cv * inc.x, -cv * inc.y, fma(-k, inc.z, 1.0)};
            if (prof == ROX_CONIC)
                nrm = unit_f(nrm);
        } else {
            nrm = unit_f(df);
        }

        if (kEarly && hit) {
            so.put(surf, 7, nrm.x); so.put(surf, 8, nrm.y); so.put(surf, 9, nrm.z);
        }

        // :198-202 aperture test (in_surface_range, :134-142)
        bool blocked = false;
        if (c.check_ap && surf >= c.first_surf && (c.last_surf < 0 || surf <= c.last_surf) &&
            mode != ROX_PHANTOM) {
            const int n_ap = (FEAT & F_APLIST) ? ints_of(row)[3] : 0;
            blocked = n_ap > 0
                ? !inside_aperture_list(row, n_ap, inc.x, inc.y, c.fuzz,
                                        c.aplthr ? c.aplthr + (size_t)surf * ROX_MAX_AP : nullptr)
                : !(fma(inc.y, inc.y, inc.x * inc.x) <= c.apthr[surf]);
        }

        // :205-221 phase element (the exact code: rare), or refract / reflect / pass through
        bool tir = false;
        int ph_fail = ROX_OK;
        if ((FEAT & F_PHASE) && ints_of(row + O_PH)[0] != ROX_PH_NONE) {
            if (hit && !blocked) {
                double dW = 0.0;
                const auto pc = c.phc + ((PER_RAY_WVL ? (size_t)wi * N : 0) + surf) * kPhaseConsts;
                v3 out = ad;
                const int rc = apply_phase(row + O_PH, pc, inc, b4d, nrm, z_dir_before,
                                           c.wvls[wi], nwl[surf - 1], nwl[surf], mode, out, dW);
                ad = out;
                if (rc == PHASE_OK)
                    phs += dW;
                else
                    ph_fail = (rc == PHASE_TIR) ? ROX_TIR : ROX_EVANESCENT;       // :253-257
            }
        } else if (mode == ROX_TRANSMIT || mode == ROX_REFLECT) {                   // (wave-uniform)
            tir = !interact_f(b4d, nrm, muw[surf], muw[N + surf], muw[2 * N + surf], ad);   // :239-245
        } else {
            ad = b4d;       // dummy / phantom: the direction as it is, whatever the normal (:215-221)
        }
        // :231-257 the first failure in the reference's order: miss, blocked, TIR / evanescent
        const int st = !hit ? (int)ROX_MISSED_SURFACE
                     : blocked ? (int)ROX_BLOCKED
                     : tir ? (int)ROX_TIR : ph_fail;
        if (st != ROX_OK) {
            status = st;
            fail_surf = surf;
            if (kFull && hit) {         // :239-257 partial record: [inc_pt, before_dir, 0.0, normal]
                if (kEarly) {
                    so.put(surf, 3, bd0.x); so.put(surf, 4, bd0.y); so.put(surf, 5, bd0.z);
                } else {
                    so.pdn(surf, inc, bd0, nrm);
                }
                so.dst(surf, 0.0);
            }
            return false;
        }
        if (kEarly) {
            so.put(surf, 3, ad.x); so.put(surf, 4, ad.y); so.put(surf, 5, ad.z);
        } else if (kFull) {
            so.pdn(surf, inc, ad, nrm);
        }
        if (OUT_MODE == ROX_OUT_OPD || OUT_MODE == ROX_OUT_FAN) {
            if (surf == 1)
                e.ray1_p = inc;
            if (surf == N - 2) {
                e.rayk_p = inc;
                e.rayk_d = ad;
            }
        }
        z_dir_before = row[O_ZDIR];
        return true;
    };

    if constexpr (kSync) {
        // every wave of the workgroup reaches every barrier; lanes whose ray has ended idle
        bool alive = false;
        if (N > 1) {
            __builtin_amdgcn_s_barrier();
            if (status == ROX_OK)
                alive = interface(1, pp1, b4d1, pp_dst1);
        }
        for (int surf = 2; surf < N; ++surf) {
            __builtin_amdgcn_s_barrier();
            if (!alive)
                continue;
            const auto prow = tbl + (size_t)(surf - 1) * kRowDoubles;
            v3 b4p{inc.x - prow[O_T], inc.y - prow[O_T + 1], inc.z - prow[O_T + 2]};
            v3 b4d = ad;
            if ((ints_of(prow)[5] & 2) == 0) {
                b4p = rotate_f(prow + O_RT, b4p);
                b4d = rotate_f(prow + O_RT, ad);
            }
            const double pp_dst = -dot3_f(b4p, b4d);
            const v3 pp{fma(pp_dst, b4d.x, b4p.x), fma(pp_dst, b4d.y, b4p.y), fma(pp_dst, b4d.z, b4p.z)};
            alive = interface(surf, pp, b4d, pp_dst);
        }
    } else if (status == ROX_OK && N > 1 && interface(1, pp1, b4d1, pp_dst1)) {
        for (int surf = 2; surf < N; ++surf) {
            // :170-174 transform to the new vertex frame, closest approach to its origin
            const auto prow = tbl + (size_t)(surf - 1) * kRowDoubles;
            v3 b4p{inc.x - prow[O_T], inc.y - prow[O_T + 1], inc.z - prow[O_T + 2]};
            v3 b4d = ad;
            if ((ints_of(prow)[5] & 2) == 0) {  // (identity rotations are flagged on the device row)
                b4p = rotate_f(prow + O_RT, b4p);
                b4d = rotate_f(prow + O_RT, ad);
            }
            const double pp_dst = -dot3_f(b4p, b4d);
            const v3 pp{fma(pp_dst, b4d.x, b4p.x), fma(pp_dst, b4d.y, b4p.y), fma(pp_dst, b4d.z, b4p.z)};
            if (!interface(surf, pp, b4d, pp_dst))
                break;
        }
    }
    if (kFull && status == ROX_OK)      // :259-262
        so.dst(N - 1, 0.0);
    e.status = status;
    e.fail_surf = fail_surf;
    e.opl = opl;
    e.phs = phs;
    e.inc = inc; e.ad = ad; e.nrm = nrm;
}

// ------------------------------------------------------------------ ray start
// opticalspec.py:1339-1353 apply_vignetting + :289-400 ray_start_from_osp +
// trace.py:302-308.  pupil (px, py) is updated in place (the reference's quirk).
template <class FLD>     // rox_field (kernel argument, batch item in constant memory, aim problem)
__device__ __forceinline__ void ray_start(FLD &f, uint32_t flags, double &px,
                                          double &py, v3 &pt0, v3 &dir0)
{
    if (flags & ROX_APPLY_VIGNETTING) {         // opticalspec.py:1339-1353
        if (px < 0.0) { if (f.vlx != 0.0) px *= (1.0 - f.vlx); }
        else          { if (f.vux != 0.0) px *= (1.0 - f.vux); }
        if (py < 0.0) { if (f.vly != 0.0) py *= (1.0 - f.vly); }
        else          { if (f.vuy != 0.0) py *= (1.0 - f.vuy); }
    }
    pt0 = v3{f.pt0[0], f.pt0[1], f.pt0[2]};
    const int kind = f.kind;                    // wave-uniform
    if (kind <= ROX_FLD_AIM_PT) {
        v3 pt1;
        if (kind == ROX_FLD_EPD) {              // :358-366
            pt1 = v3{f.eprad * px + f.aim[0], f.eprad * py + f.aim[1], f.z_enp};
        } else if (kind == ROX_FLD_AIM_PT) {    // :334-337
            pt1 = v3{px, py, f.z_enp};
        } else {                                // :340-356 wide angle
            pt1 = rotate(f.rot, f.rot_order, v3{f.eprad * px, f.eprad * py, f.eprad * 0.});
            pt1.z -= f.z_enp;
        }
        dir0 = unit(v3{pt1.x - pt0.x, pt1.y - pt0.y, pt1.z - pt0.z});
    } else {                                    // :368-398 angular measures
        double dx, dy;
        if (kind == ROX_FLD_NA) {
            dx = f.eprad * px;
            dy = f.eprad * py;
        } else if (kind == ROX_FLD_FNO) {
            const double slope = f.eprad;
            const double ax = px * slope, ay = py * slope;
            const double hypt = sqrt(1 + ax * ax + ay * ay);
            dx = slope * px / hypt;
            dy = slope * py / hypt;
        } else {
            dx = px;
            dy = py;
        }
        if (kind != ROX_FLD_AIM_DIR) {
            dx += f.cr_dir[0];
            dy += f.cr_dir[1];
        }
        const double dd = fma(dy, dy, fma(dx, dx, 0.0));    // np.dot of 2-vectors
        dir0 = v3{dx, dy, sqrt(1 - dd)};
    }
    if (kind != ROX_FLD_EPD_WIDE && dir0.z * f.z_dir0 < 0)   // trace.py:304-308
        dir0 = v3{-dir0.x, -dir0.y, -dir0.z};
}

}  // namespace rox
