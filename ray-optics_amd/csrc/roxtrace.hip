// roxtrace.hip -- the core of the host side of libroxtrace.so (include/roxtrace.h): the error
// path of every entry point, the device / pinning / copy entries, and rox_system.  The rest of
// the C ABI over the gfx950 kernels of rox_device.hpp, one concern per unit:
//   rox_system.hpp      rox_system, the per-stream state StreamCtx, what the units below share
//   launch.hip          launch policy and launch: check_opts, use_fast(), want_small(), pick_instance,
//                       want_two_pass, launch_setup, launch -> trace_kernel<...> (csrc/inst_*.hip)
//   trace_entries.hip   rox_trace_rays / _pupil_grid / _pupil_list / _pupil_grids, the pupil axes,
//                       ROX_HOST_POINTERS staging, rox_time_pupil_grid
//   focus.hip           rox_trace_through_focus[_grids] (trace_focus_items, the finishing pass)
//   search_entries.hip  rox_aim_chief_rays, rox_iterate_ray_raw, rox_find_real_enp,
//                       rox_iterate_pupil_rays, rox_calc_vignetting -> csrc/rox_search.hpp kernels
//   selftest.hip        rox_selftest_fp64
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <new>

#include "rox_system.hpp"

#pragma clang fp contract(off)

using namespace rox;

namespace {

thread_local char g_err[512] = "";

StreamCtx *ctx_for(rox_system *sys, hipStream_t st)
{
    std::lock_guard<std::mutex> lock(sys->mu);
    for (StreamCtx *c : sys->ctxs)
        if (c->stream == st)
            return c;
    StreamCtx *c = new (std::nothrow) StreamCtx;
    if (c) {
        c->stream = st;
        sys->ctxs.push_back(c);
    }
    return c;
}

// DiffractionGrating constants per (wavelength, interface), doe.py:138-143,
// with libm pow() for `mu**2` and `T**2` as CPython / NumPy scalars evaluate them.
// (Called through a volatile pointer: the compiler folds a direct pow(x, 2.0) into x * x,
// which is not what libm returns for about one argument in a thousand.)
double (*volatile libm_pow)(double, double) = pow;

void phase_consts(const rox_surface *rows, int N, const double *n_table, const double *wvls,
                  int W, std::vector<double> &pc)
{
    pc.assign((size_t)W * N * kPhaseConsts, 0.0);
    for (int w = 0; w < W; ++w)
        for (int i = 1; i < N; ++i) {
            const rox_phase &ph = rows[i].ph;
            if (ph.kind != ROX_PH_GRATING)
                continue;
            const double n_in = n_table[(size_t)w * N + i - 1], n_out = n_table[(size_t)w * N + i];
            const double refl = rows[i].mode == ROX_REFLECT ? -1.0 : 1.0;
            const double mu = n_in / n_out;
            const double T = refl * (wvls[w] * ph.order) / (ph.spacing_nm * n_out);
            double *o = &pc[((size_t)w * N + i) * kPhaseConsts];
            o[0] = mu;
            o[1] = libm_pow(mu, 2.0);
            o[2] = T;
            o[3] = libm_pow(T, 2.0);
        }
}

}  // namespace

int rox::host_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

void rox::system_slot_map(const rox_system *s, bool filter, std::vector<int32_t> &m, int32_t &n_seg)
{
    const int N = s->n_ifcs;
    m.assign(2 * N, 0);
    int next = 0;
    for (int i = 0; i < N; ++i) {
        // a phantom's segment is dropped when the *following* surface sees
        // b4_interact_mode == 'phantom' (raytrace.py:185-188); the last
        // interface has no follower, and the object is 'dummy' unless
        // intersect_obj reads its own mode
        const bool filtered = filter && s->rows[i].mode == ROX_PHANTOM && i > 0 && i < N - 1;
        m[N + i] = next;                // nslots_before[i]
        m[i] = filtered ? -1 : next++;
    }
    n_seg = next;
}

int rox::stream_ctx(rox_system *sys, hipStream_t st, StreamCtx *&cx)
{
    cx = ctx_for(sys, st);
    return cx ? 0 : fail(ROX_E_NOMEM, "out of host memory");
}

std::unique_lock<std::mutex> rox::enqueue_lock(rox_system *sys, hipStream_t st)
{
    StreamCtx *cx = ctx_for(sys, st);
    return cx ? std::unique_lock<std::mutex>(cx->enqueue_mu) : std::unique_lock<std::mutex>();
}

// ---------------------------------------------------------------------- C ABI
const rox_surface *rox::system_rows(const rox_system *sys, int32_t *n_ifcs)
{
    *n_ifcs = sys->n_ifcs;
    return sys->rows.data();
}

extern "C" {

int rox_abi_version(void) { return ROX_ABI_VERSION; }

const char *rox_last_error(void) { return g_err; }

int rox_device_count(int *count)
{
    if (!count)
        return fail(ROX_E_ARG, "null argument");
    *count = 0;
    hipError_t e = hipGetDeviceCount(count);
    if (e != hipSuccess) {
        *count = 0;
        return fail(ROX_E_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    return 0;
}

int rox_set_device(int device)
{
    HIP_TRY(hipSetDevice(device));
    return 0;
}

int rox_pin_host_memory(void *p, size_t bytes, void **device_ptr)
{
    if (!p || !bytes || !device_ptr)
        return fail(ROX_E_ARG, "rox_pin_host_memory: bad argument");
    HIP_TRY(hipHostRegister(p, bytes, hipHostRegisterMapped | hipHostRegisterPortable));
    hipError_t e = hipHostGetDevicePointer(device_ptr, p, 0);
    if (e != hipSuccess) {
        (void)hipHostUnregister(p);
        return fail(ROX_E_HIP, "hipHostGetDevicePointer: %s", hipGetErrorString(e));
    }
    return 0;
}

int rox_unpin_host_memory(void *p)
{
    if (!p)
        return fail(ROX_E_ARG, "rox_unpin_host_memory: null pointer");
    HIP_TRY(hipHostUnregister(p));
    return 0;
}

int rox_copy_async(void *dst, const void *src, size_t bytes, void *stream)
{
    if (bytes == 0)
        return 0;
    if (!dst || !src)
        return fail(ROX_E_ARG, "rox_copy_async: null pointer");
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, (hipStream_t)stream));
    return 0;
}

int rox_synchronize(void *stream)
{
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

int rox_system_create(const rox_surface *rows, int32_t n_ifcs, const double *n_table,
                      const double *wvls, int32_t n_wvls, rox_system **out_sys)
{
    if (!rows || !n_table || !out_sys || n_ifcs < 2 || n_wvls < 1)
        return fail(ROX_E_ARG, "rox_system_create: bad argument");
    int features = 0, n_newton = 0;
    for (int i = 0; i < n_ifcs; ++i) {
        const rox_surface &s = rows[i];
        if (s.profile >= ROX_EVENPOLY && s.profile <= ROX_XTOROID)
            ++n_newton;
        if (s.mode < ROX_TRANSMIT || s.mode > ROX_PHANTOM || s.profile < ROX_SPHERICAL ||
            s.profile > ROX_THINLENS || s.ncoef < 0 || s.ncoef > ROX_MAX_COEF || s.n_ap < 0 ||
            s.n_ap > ROX_MAX_AP || s.ph.kind < ROX_PH_NONE || s.ph.kind > ROX_PH_HOLOGRAM ||
            s.ph.ncoef < 0 || s.ph.ncoef > ROX_MAX_COEF)
            return fail(ROX_E_ARG, "rox_system_create: row %d is malformed", i);
        // rox_surface.flags: ROX_SURF_CV_INT_ZERO says "the curvature is the INTEGER 0" (its
        // only effect: the zero signs of Spherical / Conic df).  It means nothing on any other
        // row, and a caller that left the field uninitialised must not get flat normals on a
        // curved surface: refused, as are bits this version does not define.
        if ((s.flags & ~ROX_SURF_CV_INT_ZERO) != 0)
            return fail(ROX_E_ARG, "rox_system_create: row %d: unknown bits in rox_surface.flags (%#x)", i,
                        (unsigned)s.flags);
        if ((s.flags & ROX_SURF_CV_INT_ZERO) && !(s.profile <= ROX_CONIC && s.cv == 0.0))
            return fail(ROX_E_ARG, "rox_system_create: row %d: ROX_SURF_CV_INT_ZERO on a surface that is not "
                                   "a Spherical / Conic of zero curvature", i);
        if (s.profile == ROX_EVENPOLY)
            features |= F_EVEN;
        else if (s.profile == ROX_RADIALPOLY)
            features |= F_RADIAL;
        else if (s.profile == ROX_YTOROID || s.profile == ROX_XTOROID)
            features |= F_TOROID;
        else if (s.profile == ROX_THINLENS)
            features |= F_PHASE;
        if (s.n_ap > 0)
            features |= F_APLIST;
        if (s.ph.kind != ROX_PH_NONE)
            features |= F_PHASE;
    }
    if ((features & F_PHASE) && !wvls)
        return fail(ROX_E_ARG, "rox_system_create: phase elements need the wavelengths (wvls)");
    rox_system *sys = new (std::nothrow) rox_system;
    if (!sys)
        return fail(ROX_E_NOMEM, "out of host memory");
    sys->n_ifcs = n_ifcs;
    sys->n_wvls = n_wvls;
    sys->features = features;
    sys->n_newton = n_newton;
    sys->rows.assign(rows, rows + n_ifcs);
    hipError_t e = hipGetDevice(&sys->device);
    if (e != hipSuccess) {
        delete sys;
        return fail(ROX_E_NO_DEVICE, "hipGetDevice: %s", hipGetErrorString(e));
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, sys->device) == hipSuccess && prop.multiProcessorCount > 0)
        sys->num_cus = prop.multiProcessorCount;
    int rc = 0;
    do {
        std::vector<dev_surface> drows(n_ifcs);
        for (int i = 0; i < n_ifcs; ++i) {
            drows[i].pub = rows[i];
            // device copy only: rt is exactly the identity (every centred interface) -- the
            // kernels then transform with `v + 0.0` instead of the dgemv chain (rox_ray.hpp)
            {
                static const double eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
                bool ident = true;
                for (int k = 0; k < 9; ++k)
                    ident = ident && rows[i].rt[k] == eye[k] && !std::signbit(rows[i].rt[k]);
                // device copy of flags: bit 1 = identity rotation (bit 0 = ROX_SURF_CV_INT_ZERO)
                drows[i].pub.flags = (rows[i].flags & ROX_SURF_CV_INT_ZERO) | (ident ? 2 : 0);
            }
            // device copy only: `-self.cv` as Spherical/Conic.df forms it (rox_ray.hpp reads
            // it from the cR slot, which only toroids use): +0.0 for an integer-zero curvature
            if (rows[i].profile <= ROX_CONIC)
                drows[i].pub.cR = (rows[i].flags & ROX_SURF_CV_INT_ZERO) ? 0.0 : -rows[i].cv;
            const double c0 = rows[i].profile == ROX_RADIALPOLY ? 1.0 : 2.0;
            double c_coef = c0;                 // profiles.py:877-882, 1104-1109, 1364-1369
            for (int k = 0; k < ROX_MAX_COEF; ++k) {
                drows[i].cd[2 * k] = rows[i].coefs[k];
                drows[i].cd[2 * k + 1] = c_coef * rows[i].coefs[k];
                c_coef += c0;
            }
        }
        std::vector<double> wv(n_wvls, 0.0), pc;
        if (wvls)
            wv.assign(wvls, wvls + n_wvls);
        phase_consts(rows, n_ifcs, n_table, wv.data(), n_wvls, pc);
        const size_t rb = sizeof(dev_surface) * n_ifcs, nb = sizeof(double) * n_wvls * n_ifcs;
        if (hipMalloc(&sys->d_rows, rb) != hipSuccess || hipMalloc(&sys->d_ntab, nb) != hipSuccess ||
            hipMalloc(&sys->d_phc, nb * kPhaseConsts) != hipSuccess ||
            hipMalloc(&sys->d_wvls, sizeof(double) * n_wvls) != hipSuccess) {
            rc = fail(ROX_E_HIP, "hipMalloc failed for the surface table");
            break;
        }
        if (hipMemcpy(sys->d_rows, drows.data(), rb, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(sys->d_ntab, n_table, nb, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(sys->d_phc, pc.data(), nb * kPhaseConsts, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(sys->d_wvls, wv.data(), sizeof(double) * n_wvls, hipMemcpyHostToDevice) !=
                hipSuccess) {
            rc = fail(ROX_E_HIP, "hipMemcpy failed for the surface table");
            break;
        }
        for (int f = 0; f < 2 && !rc; ++f) {
            std::vector<int32_t> m;
            system_slot_map(sys, f == 1, m, sys->n_seg[f]);
            if (hipMalloc(&sys->d_slots[f], sizeof(int32_t) * m.size()) != hipSuccess ||
                hipMemcpy(sys->d_slots[f], m.data(), sizeof(int32_t) * m.size(),
                          hipMemcpyHostToDevice) != hipSuccess)
                rc = fail(ROX_E_HIP, "slot map upload failed");
        }
    } while (0);
    if (rc) {
        rox_system_destroy(sys);
        return rc;
    }
    *out_sys = sys;
    return 0;
}

int rox_system_destroy(rox_system *sys)
{
    if (!sys)
        return 0;
    (void)hipFree(sys->d_rows);
    (void)hipFree(sys->d_ntab);
    (void)hipFree(sys->d_phc);
    (void)hipFree(sys->d_wvls);
    (void)hipFree(sys->d_slots[0]);
    (void)hipFree(sys->d_slots[1]);
    for (StreamCtx *c : sys->ctxs) {
        (void)hipFree(c->axes.d);
        (void)hipFree(c->compact.d_tiles);
        (void)hipFree(c->compact.d_ticket);
        (void)hipFree(c->compact.d_hits_base);
        (void)hipFree(c->pack.d_xy);
        (void)hipFree(c->pack.d_status);
        (void)hipFree(c->stage.d);
        (void)hipHostFree(c->stage.h);
        (void)hipFree(c->batch.d_items);
        (void)hipHostFree(c->batch.h_items);
        (void)hipFree(c->batch.d_tickets);
        (void)hipFree(c->batch.d_tiles);
        (void)hipFree(c->focus.d);
        (void)hipHostFree(c->focus.h.h);
        if (c->focus.h.ev)
            (void)hipEventDestroy(c->focus.h.ev);
        for (hipEvent_t ev : c->batch.ev)
            if (ev)
                (void)hipEventDestroy(ev);
        delete c;
    }
    (void)hipHostFree(sys->h_search);
    delete sys;
    return 0;
}

int rox_system_num_segments(const rox_system *sys, uint32_t flags, int32_t *n_seg)
{
    if (!sys || !n_seg)
        return fail(ROX_E_ARG, "null argument");
    *n_seg = sys->n_seg[(flags & ROX_FILTER_PHANTOMS) ? 1 : 0];
    return 0;
}

}  // extern "C"
