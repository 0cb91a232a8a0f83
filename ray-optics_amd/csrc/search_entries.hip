// search_entries.hip -- the host side of the iterated single-ray searches (include/roxtrace.h):
// chief-ray aiming, the wide-angle pupil search, pupil iterations and vignetting.  The kernels
// are rox_search.hpp's, compiled per feature instance in search_*.hip.
#include <cstring>

#include "rox_system.hpp"

using namespace rox;

namespace {

// The LDS need of a search launch (rox_search.hpp search_ctx()): surface table + index table +
// phase constants + wavelengths + slot map + the vignetting search's aperture thresholds.
// gtab = that does not fit the LDS of a workgroup: the general instance over the table in global
// memory (search_general_gtab.hip), where the table and the phase constants stay and the
// circular clear-aperture thresholds of the checked trace get an array.
int search_lds(const rox_system *sys, size_t &lds, bool &gtab)
{
    const size_t N = sys->n_ifcs, W = sys->n_wvls;
    auto bytes = [N, W](bool g) {
        return up16((g ? N * ROX_MAX_AP * sizeof(double)
                       : N * sizeof(dev_surface) + W * N * sizeof(double) * kPhaseConsts) +
                    W * N * sizeof(double) + W * sizeof(double) + 2 * N * sizeof(int32_t) + N * sizeof(double));
    };
    lds = bytes(false);
    gtab = lds > kLdsLimit || force_gtab();
    if (gtab && (lds = bytes(true)) > kLdsLimit)
        return fail(ROX_E_UNSUPPORTED, "%zu interfaces x %zu wavelengths need %zu B of LDS for their "
                                       "indices and thresholds alone (max %zu)", N, W, lds, kLdsLimit);
    return 0;
}

// the entry points of the search instance a launch takes: the leanest of kSearchInstances that
// covers the system's features (their trial rays never filter phantoms), or -- gtab: search_lds
// found the table too large for the LDS -- the general instance over global memory
const SearchInstanceFns &search_fns(const rox_system *sys, bool gtab)
{
#define ROX_SEARCH_FNS(name, FEAT) &search_##name,
    static const SearchInstanceFns *const fns[] = {ROX_SEARCH_INSTANCES(ROX_SEARCH_FNS)};
#undef ROX_SEARCH_FNS
    if (gtab)
        return search_general_gtab;
    const int last = (int)(sizeof kSearchInstances / sizeof kSearchInstances[0]) - 1;
    int i = 0;
    while (i < last && (sys->features & ~kSearchInstances[i]) != 0)
        ++i;
    return *fns[i];
}

// the iterated single-ray searches (aiming, vignetting, pupil iterations): up to this many
// problems per call get a wave each (latency: a model's fields, run side by side); larger
// batches keep a lane per problem (throughput: soaks, sweeps)
constexpr int32_t kWavePerProblemMax = 1024;

// What the search entries do once their own argument checks have passed.  `block` lays the
// pointers of `a` out in the system's search block, the n problems first; the instance's launch
// `fn` runs on them; copy_out() hands the results to the caller once the kernel is done.
// search_mu is held from before the block is written until the results are copied out.
template <class Args, class Prob, class CopyOut>
int run_search(const char *entry, rox_system *sys, Args &a, const Layout &block, const Prob *probs, int32_t n,
               void (*SearchInstanceFns::*fn)(const Args &, size_t, hipStream_t), void *stream,
               CopyOut copy_out)
{
    hipStream_t st = (hipStream_t)stream;
    size_t lds;
    bool gtab;
    ROX_TRY(search_lds(sys, lds, gtab));
    std::lock_guard<std::mutex> lock(sys->search_mu);
    if (sys->h_search_cap < block.size()) {
        size_t cap = size_t(16) << 10;
        while (cap < block.size())
            cap *= 2;
        HIP_TRY(regrow(sys->h_search, sys->h_search_cap, cap, cap, hipHostMallocMapped));
    }
    block.carve(sys->h_search);
    memcpy(sys->h_search, probs, sizeof(Prob) * n);
    a.rows = sys->d_rows;               // (the fields AimArgs, EnpArgs and VigArgs have in common)
    a.n_table = sys->d_ntab;
    a.ph_consts = sys->d_phc;
    a.wvls = sys->d_wvls;
    a.slots = sys->d_slots[0];
    a.n_ifcs = sys->n_ifcs;
    a.n_wvls = sys->n_wvls;
    a.n = n;
    (search_fns(sys, gtab).*fn)(a, lds, st);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = hipStreamSynchronize(st);
    if (e != hipSuccess)
        return fail(ROX_E_HIP, "%s: %s", entry, hipGetErrorString(e));
    copy_out();
    return 0;
}

}  // namespace

extern "C" {

int rox_iterate_ray_raw(rox_system *sys, int32_t n, const rox_aim *probs, double eps,
                        double *aim_xy, int32_t *result, double *last_xy, int32_t *last_status,
                        void *stream)
{
    if (!sys || n < 0 || (n > 0 && (!probs || !aim_xy || !result)) || (!last_xy != !last_status))
        return fail(ROX_E_ARG, "rox_iterate_ray_raw: bad argument");
    if (n == 0)
        return 0;
    for (int i = 0; i < n; ++i) {
        if (probs[i].wvl_idx < 0 || probs[i].wvl_idx >= sys->n_wvls)
            return fail(ROX_E_ARG, "probs[%d].wvl_idx %d out of range", i, probs[i].wvl_idx);
        if (probs[i].surf < 0 || probs[i].surf >= sys->n_ifcs)
            return fail(ROX_E_ARG, "probs[%d].surf %d out of range", i, probs[i].surf);
        if (probs[i].two_d && !(probs[i].epsfcn >= 0.0))
            return fail(ROX_E_ARG, "probs[%d].epsfcn %g", i, probs[i].epsfcn);
    }
    const size_t yb = up16(sizeof(double) * 2 * n), rb = up16(sizeof(int32_t) * n);
    AimArgs a{};
    Layout block;
    block.add(a.probs, up16(sizeof(rox_aim) * n)).add(a.aim_xy, yb).add(a.result, rb);
    if (last_xy)
        block.add(a.last_xy, yb).add(a.last_status, rb);
    a.eps = eps;
    a.wave_per_problem = n <= kWavePerProblemMax;
    return run_search("rox_iterate_ray_raw", sys, a, block, probs, n, &SearchInstanceFns::aim, stream, [&] {
        memcpy(aim_xy, a.aim_xy, sizeof(double) * 2 * n);
        memcpy(result, a.result, sizeof(int32_t) * n);
        if (last_xy) {
            memcpy(last_xy, a.last_xy, sizeof(double) * 2 * n);
            memcpy(last_status, a.last_status, sizeof(int32_t) * n);
        }
    });
}

int rox_aim_chief_rays(rox_system *sys, int32_t n, const rox_aim *probs, double eps,
                       double *aim_xy, int32_t *result, void *stream)
{
    return rox_iterate_ray_raw(sys, n, probs, eps, aim_xy, result, nullptr, nullptr, stream);
}

int rox_find_real_enp(rox_system *sys, int32_t n, const rox_enp *probs, double eps,
                      double *z_out, int32_t *result, void *stream)
{
    if (!sys || n < 0 || (n > 0 && (!probs || !z_out || !result)))
        return fail(ROX_E_ARG, "rox_find_real_enp: bad argument");
    if (n == 0)
        return 0;
    for (int i = 0; i < n; ++i) {
        if (probs[i].wvl_idx < 0 || probs[i].wvl_idx >= sys->n_wvls)
            return fail(ROX_E_ARG, "probs[%d].wvl_idx %d out of range", i, probs[i].wvl_idx);
        if (probs[i].surf < 0 || probs[i].surf >= sys->n_ifcs)
            return fail(ROX_E_ARG, "probs[%d].surf %d out of range", i, probs[i].surf);
    }
    EnpArgs a{};
    Layout block;
    block.add(a.probs, up16(sizeof(rox_enp) * n)).add(a.z_out, up16(sizeof(double) * 2 * n))
        .add(a.result, up16(sizeof(int32_t) * n));
    a.eps = eps;
    return run_search("rox_find_real_enp", sys, a, block, probs, n, &SearchInstanceFns::enp, stream, [&] {
        memcpy(z_out, a.z_out, sizeof(double) * 2 * n);
        memcpy(result, a.result, sizeof(int32_t) * n);
    });
}

int rox_iterate_pupil_rays(rox_system *sys, int32_t n, const rox_pupil_iter *probs, double eps,
                           double *start_r, void *stream)
{
    if (!sys || n < 0 || (n > 0 && (!probs || !start_r)))
        return fail(ROX_E_ARG, "rox_iterate_pupil_rays: bad argument");
    if (n == 0)
        return 0;
    for (int i = 0; i < n; ++i) {
        const rox_pupil_iter &p = probs[i];
        if (p.wvl_idx < 0 || p.wvl_idx >= sys->n_wvls)
            return fail(ROX_E_ARG, "probs[%d].wvl_idx %d out of range", i, p.wvl_idx);
        if (p.indx < 0 || p.indx >= sys->n_ifcs || (p.xy != 0 && p.xy != 1))
            return fail(ROX_E_ARG, "probs[%d] is malformed", i);
        ROX_TRY(check_field(&p.fld));
    }
    VigArgs a{};
    Layout block;
    block.add(a.iters, up16(sizeof(rox_pupil_iter) * n)).add(a.vig, up16(sizeof(double) * n));
    a.eps = eps;
    a.wave_per_problem = n <= kWavePerProblemMax;
    return run_search("rox_iterate_pupil_rays", sys, a, block, probs, n, &SearchInstanceFns::vig, stream,
                      [&] { memcpy(start_r, a.vig, sizeof(double) * n); });
}

int rox_calc_vignetting(rox_system *sys, int32_t n, const rox_vig *probs, double eps,
                        double *vig, int32_t *clip_surf, void *stream)
{
    if (!sys || n < 0 || (n > 0 && (!probs || !vig || !clip_surf)))
        return fail(ROX_E_ARG, "rox_calc_vignetting: bad argument");
    if (n == 0)
        return 0;
    for (int i = 0; i < n; ++i) {
        const rox_vig &p = probs[i];
        if (p.wvl_idx < 0 || p.wvl_idx >= sys->n_wvls)
            return fail(ROX_E_ARG, "probs[%d].wvl_idx %d out of range", i, p.wvl_idx);
        if (p.stop_surf >= sys->n_ifcs || (p.xy != 0 && p.xy != 1) || p.max_iter < 0)
            return fail(ROX_E_ARG, "probs[%d] is malformed", i);
        ROX_TRY(check_field(&p.fld));
    }
    VigArgs a{};
    Layout block;
    block.add(a.probs, up16(sizeof(rox_vig) * n)).add(a.vig, up16(sizeof(double) * n))
        .add(a.clip, up16(sizeof(int32_t) * n));
    a.eps = eps;
    a.wave_per_problem = n <= kWavePerProblemMax;
    return run_search("rox_calc_vignetting", sys, a, block, probs, n, &SearchInstanceFns::vig, stream, [&] {
        memcpy(vig, a.vig, sizeof(double) * n);
        memcpy(clip_surf, a.clip, sizeof(int32_t) * n);
    });
}

}  // extern "C"
