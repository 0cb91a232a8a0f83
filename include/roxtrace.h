/* roxtrace.h -- C ABI of libroxtrace.so, the MI355X (gfx950) sequential
 * real-ray trace engine that sits behind ray-optics' `raytr` hot path.
 *
 * The reference (mjhoptics/ray-optics) is pure Python and has no FFI; the
 * seams this ABI replaces are module-level functions:
 *
 *   rox_trace_rays         <- rayoptics/raytr/raytrace.py:51-80   trace()
 *                             rayoptics/raytr/raytrace.py:83-264  trace_raw()
 *                             rayoptics/raytr/analyses.py:458-510 trace_list_of_rays()
 *   rox_trace_pupil_grid   <- rayoptics/raytr/trace.py:563-605    trace_grid()
 *                             rayoptics/raytr/trace.py:537-560    trace_fan()
 *                             rayoptics/raytr/analyses.py:666-696 trace_ray_grid()
 *                             rayoptics/raytr/analyses.py:212-230 trace_ray_fan()
 *   rox_trace_pupil_grids  <- rayoptics/seq/sequential.py:1058-1114 SequentialModel.trace_grid /
 *                             trace_wavefront (the loop over wavelengths), one launch
 *   rox_trace_pupil_list   <- rayoptics/raytr/analyses.py:437-455 trace_ray_list()
 *                             (each of the above through trace.py:160-221
 *                             trace_safe -> trace.py:253-310 trace_base ->
 *                             opticalspec.py:289-400 ray_start_from_osp,
 *                             opticalspec.py:1339-1353 apply_vignetting)
 *   rox_aim_chief_rays     <- rayoptics/raytr/trace.py:313-415    iterate_ray() (both branches)
 *                             rayoptics/raytr/trace.py:627-640    aim_chief_ray()
 *   rox_iterate_ray_raw    <- rayoptics/raytr/trace.py:866-961    iterate_ray_raw() -- the reverse
 *                             chief ray of wideangle.py:620-665 eval_real_image_ht()
 *   rox_find_real_enp      <- rayoptics/raytr/wideangle.py:86-427 find_real_enp() /
 *                             find_edge() / find_z_enp_on_interval(), :46-83
 *                             enp_z_coordinate()
 *   rox_calc_vignetting    <- rayoptics/raytr/vigcalc.py:233-340, 396-461
 *                             calc_vignetting_for_field() / calc_vignetted_ray() /
 *                             iterate_pupil_ray()
 *   rox_iterate_pupil_rays <- rayoptics/raytr/vigcalc.py:396-461 iterate_pupil_ray() as
 *                             vigcalc.set_pupil (:123-230) calls it
 *   rox_system_create      <- rayoptics/seq/sequential.py:149-202 path()/path_sequence()
 *                             (the per-wavelength (Intfc, Gap, Tfrm, Indx, Zdir)
 *                             list flattened into one POD table)
 *
 * All arithmetic is IEEE binary64.  Plain pointers and sizes only; no torch or
 * numpy types appear in any signature.  The Python binding a ray-optics
 * maintainer would add is a ctypes stub: see INTEGRATION.md.  Timing and
 * self-test helpers used by bench.py and tests/ are declared separately in
 * roxtrace_diag.h: they are not part of the drop-in boundary.
 *
 * Ownership: the caller owns every input/output buffer; the library owns only
 * the rox_system handle.  Every entry point returns 0 on success and a
 * negative rox_err on failure, with a message retrievable through
 * rox_last_error().  Per-ray trace failures are *not* errors: they are
 * reported in rox_out.status / rox_out.fail_surf.
 */
#ifndef ROXTRACE_H
#define ROXTRACE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* libroxtrace.so is built with -fvisibility=hidden: the entry points declared between this
 * push and the pop at the end of the header are the library's whole dynamic symbol table
 * (tests/test_abi.py compares `nm -D` with the declarations). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

/* ABI history: 4 = packed hits appended over launches (ROX_HITS_APPEND), rox_pin_host_memory,
 * rox_aim carries both branches of iterate_ray;  5 = rox_trace_pupil_grids (several grids, one
 * launch), rox_find_real_enp / rox_enp (the wide-angle pupil search);  6 = rox_out.ld is the
 * capacity of seg in pairs for ROX_OUT_HITS_COMPACT (overflow: n_hits < 0), rox_copy_async,
 * rox_iterate_ray_raw, rox_iterate_pupil_rays;  7 = rox_synchronize (a binding without the
 * HIP runtime can wait for the asynchronous entries);  8 = ROX_FAST_FP64 (tolerance-mode
 * kernels for the reduced-output modes), rox_surface.flags validated by rox_system_create,
 * the dynamic symbol table is exactly this header's (+ roxtrace_diag.h's) functions and
 * DT_SONAME is libroxtrace.so.8, rox_spot_stats.
 * rox_abi_version() of the library must equal the header a binding was written against. */
#define ROX_ABI_VERSION 8
#define ROX_MAX_COEF 10   /* EvenPolynomial r^2..r^20 / RadialPolynomial r^1..r^10 */
#define ROX_MAX_AP 4      /* clear apertures per surface carried in the table */
#define ROX_SEG_DOUBLES 10 /* p[3], d[3], dst, nrml[3]  (model_constants.py:31) */

/* interface interact_mode (raytrace.py:211-221) */
enum { ROX_TRANSMIT = 0, ROX_REFLECT = 1, ROX_DUMMY = 2, ROX_PHANTOM = 3 };
/* surface profile kinds (rayoptics/elem/profiles.py).  ROX_THINLENS is not a
 * profile in the reference but the ThinLens interface's own intersect/normal
 * (rayoptics/oprops/thinlens.py:128-136): s = -p.z/d.z, normal (0,0,1). */
enum { ROX_SPHERICAL = 0, ROX_CONIC = 1, ROX_EVENPOLY = 2, ROX_RADIALPOLY = 3,
       ROX_YTOROID = 4, ROX_XTOROID = 5, ROX_THINLENS = 6 };
/* phase elements (raytrace.py:41-48, 205-210; rayoptics/oprops/doe.py) */
enum { ROX_PH_NONE = 0,
       ROX_PH_GRATING = 1,   /* DiffractionGrating.phase_ludwig, doe.py:124-175 */
       ROX_PH_DOE_RADIAL = 2,/* DiffractiveElement.phase with radial_phase_fct,
                                doe.py:28-54, 272-323                           */
       ROX_PH_HOLOGRAM = 3 };/* HolographicElement.phase, doe.py:375-397 (the
                                phase element of every ThinLens)               */
/* clear-aperture kinds (rayoptics/elem/surface.py:398-494).  Elliptical has
 * no point_inside() in the reference, so it returns None and the ray is
 * always blocked; ROX_AP_ALWAYS_BLOCK reproduces that. */
enum { ROX_AP_CIRCULAR = 0, ROX_AP_RECTANGULAR = 1, ROX_AP_ALWAYS_BLOCK = 2 };
/* per-ray status (rayoptics/raytr/traceerror.py:12-52) */
enum { ROX_OK = 0, ROX_MISSED_SURFACE = 1, ROX_TIR = 2, ROX_BLOCKED = 3,
       ROX_EVANESCENT = 4 };
/* what rox_out.seg receives */
enum { ROX_OUT_FULL = 0,  /* seg[n_seg][10][ld]: the whole RayPkg.ray          */
       ROX_OUT_LAST = 1,  /* seg[10][ld]: ray[-1] only (trace_safe 'last')      */
       ROX_OUT_HITS = 2,  /* seg[2][ld]: SpotDiagramFigure's `spot` filter,
                             (ray[-1].p + (foc/ray[-1].d[2])*ray[-1].d - image_pt).xy
                             (rayoptics/mpl/axisarrayfigure.py:229-238)         */
       ROX_OUT_OPD = 3,   /* seg[1][ld]: wave_abr_full_calc_finite_pup, the OPD of
                             the ray w.r.t. the chief ray on a finite reference
                             sphere, system units (rayoptics/raytr/waveabr.py:256-307);
                             constants in rox_opts.wf; on an infinite reference
                             sphere wave_abr_full_calc_inf_ref (:356-424)       */
       ROX_OUT_HITS_COMPACT = 4,
                          /* seg[n_hits][2]: the HITS pair (x, y) of the rays that
                             reach the image only, interleaved, packed in ray order
                             -- the (R_ok, 2) array SequentialModel.trace_grid(...,
                             form='list', append_if_none=False) hands to
                             SpotDiagramFigure (rayoptics/seq/sequential.py:1058-1085,
                             rayoptics/mpl/axisarrayfigure.py:229-263).  The count goes
                             to rox_out.n_hits.  seg / n_hits may be device memory or
                             device-mapped pinned host memory (hipHostMalloc): the
                             kernel then writes the spot straight into host memory.
                             op / fail_surf / pupil are not written in this mode;
                             status is optional.                                */
       ROX_OUT_FAN = 5 }; /* seg[3][ld]: what analyses.eval_fan / focus_fan compute per
                             ray of a RayFan (rayoptics/raytr/analyses.py:233-274,
                             317-345): rows 0, 1 = the HITS pair (transverse
                             aberration at rox_opts.foc w.r.t. rox_opts.image_pt),
                             row 2 = the OPD as ROX_OUT_OPD gives it (rox_opts.wf) */
/* rox_opts.flags */
enum { ROX_CHECK_APERTURES = 1u,     /* raytrace.py:198-202                    */
       ROX_INTERSECT_OBJ = 2u,       /* raytrace.py:147-154                    */
       ROX_FILTER_PHANTOMS = 4u,     /* raytrace.py:185-188                    */
       ROX_APPLY_VIGNETTING = 8u,    /* trace.py:298-300 (pupil entries only)  */
       ROX_HOST_POINTERS = 16u };    /* every buffer is ordinary host memory: the
                                        library stages it itself (small batches
                                        through a device-mapped pinned block the
                                        kernel reads and writes directly, large
                                        ones through HBM) and the call returns
                                        when the results are in place.  seg
                                        slots the trace does not produce come
                                        back as NaN in this mode                */
/* ROX_HITS_APPEND (HITS_COMPACT only): the pairs of this call go *behind* the
 * *rox_out.n_hits pairs already in rox_out.seg, and n_hits becomes the new total --
 * a running count kept on the device side, so that several grids (the pupil-row
 * blocks of one rank of a sharded spot diagram, every (field, wavelength) of a
 * figure) pack into one buffer with no host round trip between the launches.
 * rox_out.ld is the capacity of seg in pairs: nothing is stored at or beyond it, and a
 * call that needed more room leaves the NEGATED pair count it needed in n_hits (later
 * appending calls keep it negative).                                          */
#define ROX_HITS_APPEND 32u
/* ROX_FAST_FP64: tolerance mode.  The default kernels reproduce the reference's NumPy path bit
 * for bit; with this flag the caller accepts ray intercepts, directions, optical paths and OPDs
 * within 1e-10 * max(1, |reference value|) of it -- the tolerance ray-optics users compare ray
 * traces at -- and the reduced-output modes (LAST, HITS, HITS_COMPACT, OPD, FAN), which are bound
 * by instruction issue, run on kernels that are still IEEE binary64 but use reciprocal /
 * reciprocal-square-root seeds with Newton-Raphson refinement, fused multiply-adds and Horner
 * series instead of NumPy's operation order (csrc/rox_math_fast.hpp, "tolerance mode"; observed
 * deviation <= 1e-12).  A ray whose miss / total-internal-reflection radicand or aperture margin
 * lies within rounding of zero may be classified the other way.  The flag is a permission: the
 * library takes it where it buys time and answers bit-exactly (which is within any tolerance)
 * elsewhere -- ROX_OUT_FULL packets come from the tolerance-mode kernels only for systems
 * made mostly of aspheres, whose FULL launches are bound by arithmetic too (every segment
 * within the same bar, partial records of failed rays included); FULL launches of other
 * systems (bound by their stores), FULL with ROX_FILTER_PHANTOMS and the search entries
 * (rox_aim_chief_rays, rox_find_real_enp, rox_calc_vignetting, rox_iterate_*) stay
 * bit-exact.  In a rox_trace_pupil_grids call every item must carry the same setting.   */
#define ROX_FAST_FP64 64u
/* rox_surface.rt_order: NumPy hands `rt.dot(v)` to OpenBLAS dgemv, whose FMA
 * chain runs over the columns in a different order for an F-ordered rt (the
 * transpose view compute_local_transforms makes, rayoptics/elem/transform.py:86)
 * and a C-ordered one (np.identity, or the transpose of a transpose that
 * 'dec and return' decenters produce).  Probed on OpenBLAS 0.3.29/Haswell:
 *   F: y_i = fma(a_i2,x2, fma(a_i1,x1, fma(a_i0,x0, 0)))
 *   C: y_i = fma(a_i2,x2, fma(a_i0,x0, fma(a_i1,x1, 0)))                       */
enum { ROX_RT_F_ORDER = 0, ROX_RT_C_ORDER = 1 };
/* rox_wavefront.kind */
enum { ROX_WF_FINITE = 0, ROX_WF_INF_FULL = 1, ROX_WF_INF_SPLIT = 2 };
/* rox_grid.kind */
enum { ROX_GRID_PRODUCT = 0, /* trace_grid: ray r=(i*num+j), x_i outer, y_j inner */
       ROX_GRID_FAN = 1 };   /* trace_fan: ray r at (x_r, y_r), num rays          */

typedef enum { ROX_E_OK = 0, ROX_E_ARG = -1, ROX_E_HIP = -2, ROX_E_NOMEM = -3,
               ROX_E_UNSUPPORTED = -4, ROX_E_NO_DEVICE = -5 } rox_err;

typedef struct rox_aperture {
    int32_t kind;            /* ROX_AP_* */
    int32_t is_obscuration;  /* surface.py:419,457: result inverted            */
    double x_offset, y_offset;   /* surface.py:391-394 (rotation never applied) */
    double a;                /* radius | x_half_width                          */
    double b;                /* unused | y_half_width                          */
} rox_aperture;              /* 40 bytes */

/* One row per interface, object and image included.  Row i carries the
 * transform and gap data *from* interface i *to* interface i+1, exactly as
 * the reference's path tuple does (sequential.py:167-202). */
/* Phase element attached to an interface (ifc.phase_element).  Which fields
 * are read depends on kind:
 *   GRATING    a = grating_normal, order, spacing_nm = _grating_spacing_nm
 *   DOE_RADIAL coefs[ncoef] = coefficients (r^2, r^4, ...), order, ref_wl
 *   HOLOGRAM   a = ref_pt, b = obj_pt, flags bit0 ref_virtual, bit1 obj_virtual,
 *              ref_wl                                                          */
typedef struct rox_phase {
    int32_t kind;            /* ROX_PH_*                                       */
    int32_t ncoef;
    int32_t flags;
    int32_t reserved;
    double order;
    double ref_wl;           /* nm                                             */
    double spacing_nm;
    double a[3];
    double b[3];
    double coefs[ROX_MAX_COEF];
} rox_phase;                 /* 168 bytes */

/* rox_surface.flags.  ROX_SURF_CV_INT_ZERO: the reference model holds this Spherical / Conic
 * curvature as the Python *integer* 0 (its own double Gauss data does,
 * rayoptics/raytr/tests/ag_dblgauss_s.py).  `-self.cv*p[0]` in Spherical/Conic.df
 * (profiles.py:360-362, 605-609) is then `0 * x` -- +0 for x > 0 -- where the float 0.0 gives
 * `-0.0 * x` = -0; intersect() and sag() see +0.0 either way.  cv itself is 0.0.            */
#define ROX_SURF_CV_INT_ZERO 1

typedef struct rox_surface {
    int32_t mode;            /* ROX_TRANSMIT...                                */
    int32_t profile;         /* ROX_SPHERICAL...                               */
    int32_t ncoef;           /* max_nonzero_coef (profiles.py:827-832)         */
    int32_t n_ap;            /* len(clear_apertures); 0 -> max_aperture test   */
    int32_t rt_order;        /* summation order of rt.dot(v), see ROX_RT_*      */
    int32_t flags;           /* ROX_SURF_* (0 from callers that predate it)     */
    double cv;               /* vertex curvature                               */
    double cc;               /* conic constant                                 */
    double ec;               /* cc + 1.0 as the reference evaluates it         */
    double cR;               /* Y/XToroid sweep curvature (profiles.py:1317-1437) */
    double coefs[ROX_MAX_COEF];
    double rt[9];            /* lcl_tfrms[i][0], row-major (already R^T)       */
    double t[3];             /* lcl_tfrms[i][1]                                */
    double z_dir;            /* z_dir[i] of the gap after this interface       */
    double max_aperture;     /* interface.py:113-122                           */
    rox_aperture ap[ROX_MAX_AP];
    rox_phase ph;            /* kind == ROX_PH_NONE: refract / reflect as usual */
} rox_surface;               /* 576 bytes */

/* Per (field, wavelength, focus) constants of the OPD calculation: the chief
 * ray package and reference sphere that trace.setup_pupil_coords() leaves in
 * fld.chief_ray / fld.ref_sphere (rayoptics/raytr/trace.py:608-624,
 * rayoptics/raytr/waveabr.py:23-76). */
typedef struct rox_wavefront {
    double cr1_p[3];         /* cr_ray[1][mc.p]                                 */
    double cr0_d[3];         /* cr_ray[0][mc.d]                                 */
    double crk_p[3];         /* cr_ray[-2][mc.p]                                */
    double crk_d[3];         /* cr_ray[-2][mc.d]                                */
    double cr_op;            /* chief-ray optical path                          */
    double cr_exp_pt[3];     /* cr_exp_seg[0]                                   */
    double cr_exp_dist;      /* cr_exp_seg[2]                                   */
    double ref_dir[3];       /* ref_sphere[1]                                   */
    double ref_radius;       /* ref_sphere[2]                                   */
    double n_obj, n_img;     /* abs(fod.n_obj), abs(fod.n_img)                  */
    double sign_soln;        /* -1 if ref_dir[2]*cr.ray[-1].d[2] < 0 else +1    */
    /* transform_after_surface(ifcs[-2], .) (rayoptics/elem/transform.py:234-258):
     * 0 = identity, 1 = p - t, 2 = rt.dot(p - t), rt.dot(d) */
    int32_t after_kind;
    int32_t after_order;     /* ROX_RT_* of after_rt                            */
    double after_rt[9];
    double after_t[3];
    /* Infinite reference sphere (is_kinda_big(ref_radius), waveabr.py:213-221):
     * wave_abr_full_calc_inf_ref (waveabr.py:356-424, kind ROX_WF_INF_FULL) or its
     * pre-calc / calc split (waveabr.py:427-488, ROX_WF_INF_SPLIT: the same
     * quantities, the final sum associated differently).  Chief-ray-only terms
     * are formed on the host as the reference forms them.                      */
    int32_t kind;            /* ROX_WF_*                                        */
    int32_t last_kind;       /* lcl_tfrm_last: 0 = None, 1 = (rt, t)            */
    int32_t last_order;      /* ROX_RT_* of last_rt                             */
    int32_t reserved;
    double last_rt[9];       /* seq_model.lcl_tfrms[-2][0]                      */
    double last_t[3];
    double cr_last_p[3];     /* cr_ray[-1][mc.p]                                */
    double cr_last_d[3];     /* cr_ray[-1][mc.d]                                */
    double d_cr_b4[3];       /* rt.dot(cr_ray[-2][mc.d])                        */
    double v_be;             /* cr_op + ray_dist_to_perp_from_origin(cr b4)     */
    double image_pt[3];      /* ref_sphere[0]                                   */
} rox_wavefront;

typedef struct rox_opts {
    uint32_t flags;          /* ROX_CHECK_APERTURES | ...                      */
    int32_t out_mode;        /* ROX_OUT_*                                      */
    int32_t first_surf;      /* raytrace.py:118 (trace() passes 1)             */
    int32_t last_surf;       /* raytrace.py:119; <0 means None (trace(): N-2)  */
    double eps;              /* Newton tolerance, raytrace.py:83 (1e-12)       */
    double fuzz;             /* pt_inside_fuzz, surface.py:198 (1e-5)          */
    double foc;              /* HITS only: defocus                             */
    double image_pt[2];      /* HITS only: fld.ref_sphere[0][:2]               */
    rox_wavefront wf;        /* OPD only                                       */
} rox_opts;

/* Per-field constants of ray_start_from_osp (opticalspec.py:289-400), one
 * kind per branch of that function, and of apply_vignetting
 * (opticalspec.py:1339-1353).  With pupil = (px, py) after vignetting:
 *   EPD       :358-366  pt1 = (eprad*px + aim[0], eprad*py + aim[1], z_enp);
 *                       dir0 = normalize(pt1 - pt0)
 *   EPD_WIDE  :340-356  pt1 = rot.(eprad*px, eprad*py, 0), pt1.z -= z_enp
 *                       (z_enp carries obj2enp_dist); dir0 = normalize(pt1 - pt0);
 *                       callers clear ROX_INTERSECT_OBJ (trace.py:302-303) and
 *                       the sign flip of trace.py:304-308 is skipped
 *   AIM_PT    :334-337  pupil_type 'aim pt': pt1 = (px, py, z_enp)
 *   NA        :372-376  pupil_dir = eprad*(px, py)  (eprad carries na/n)
 *   FNO       :377-384  slope = eprad (= -1/(2 fno)); hypt = sqrt(1 + (px*slope)^2
 *                       + (py*slope)^2); pupil_dir = slope*(px, py)/hypt
 *   AIM_DIR   :369-371  pupil_type 'aim dir': dir_tot = (px, py)
 *   the angular kinds (NA, FNO, AIM_DIR) finish with dir_tot = pupil_dir + cr_dir,
 *   dir0 = (dir_tot, sqrt(1 - dir_tot.dir_tot))  (:386-398)                      */
enum { ROX_FLD_EPD = 0, ROX_FLD_EPD_WIDE = 1, ROX_FLD_AIM_PT = 2, ROX_FLD_NA = 3,
       ROX_FLD_FNO = 4, ROX_FLD_AIM_DIR = 5 };

typedef struct rox_field {
    double pt0[3];           /* EPD: obj2enp_dist*[d0x/d0z, d0y/d0z, 0]; else p0 */
    double aim[2];           /* fld.aim_info or (0,0)                          */
    double eprad;            /* pupil_value/2 (see the kinds above)            */
    double z_enp;            /* fod.obj_dist + fod.enp_dist (pt1[2])           */
    double vlx, vux, vly, vuy;   /* opticalspec.py:1339-1353                   */
    double z_dir0;           /* seq_model.z_dir[0] (trace.py:307); 0 = wide-angle
                                model: dir0 is never flipped (trace.py:302-303;
                                callers also clear ROX_INTERSECT_OBJ)            */
    int32_t kind;            /* ROX_FLD_*                                      */
    int32_t rot_order;       /* ROX_RT_* of rot (np.matmul -> dgemv)           */
    double rot[9];           /* EPD_WIDE: rot_v1_into_v2(d0, z), row-major     */
    double cr_dir[2];        /* angular kinds: chief-ray direction (:386-392)  */
} rox_field;                 /* 192 bytes */

typedef struct rox_grid {
    double start[2];         /* grid_rng[0]                                    */
    double stop[2];          /* grid_rng[1]                                    */
    int32_t num;             /* grid_rng[2]                                    */
    int32_t kind;            /* ROX_GRID_PRODUCT | ROX_GRID_FAN                */
    int32_t row_begin;       /* PRODUCT only: trace pupil rows (x index i)     */
    int32_t row_count;       /*   [row_begin, row_begin+row_count); 0 = all    */
} rox_grid;                  /* (row blocks are the multi-GPU sharding unit)   */

typedef struct rox_out {
    double *seg;             /* see ROX_OUT_*; may be NULL only if unused      */
    double *op;              /* [ld] op_delta (on failure: opl, raytrace.py:236) or NULL */
    uint8_t *status;         /* [ld] ROX_OK...                                 */
    int16_t *fail_surf;      /* [ld] surface index at which the ray failed, -1 if ok; or NULL */
    double *pupil;           /* [2][ld] pupil coords after vignetting (pupil entries) or NULL */
    int64_t ld;              /* ray-axis leading dimension, >= number of rays;
                                ROX_OUT_HITS_COMPACT: capacity of seg in (x, y) pairs
                                (>= number of rays unless ROX_HITS_APPEND)         */
    int64_t *n_hits;         /* HITS_COMPACT only: receives the number of (x, y)
                                pairs written to seg                          */
} rox_out;

/* The rox_out.ld to allocate a packet buffer of n_rays rays with (in doubles; >= n_rays, at
 * most max(256, n_rays / 16) more, whole 64-byte lines).  Any ld >= n_rays gives the same
 * values; this one keeps the rows of a ROX_OUT_FULL packet from lying a power of two bytes
 * apart (ld = n_rays on a 1024 x 1024 grid: 1 % slower, 16 % with ROX_FULL_TILE_GROUP=0).
 * No device needed. */
int64_t rox_packet_ld(int64_t n_rays);

typedef struct rox_system rox_system;

/* library / device ------------------------------------------------------- */
int rox_abi_version(void);
int rox_device_count(int *count);
int rox_set_device(int device);
const char *rox_last_error(void);

/* Host memory the kernels write directly (ROX_OUT_HITS_COMPACT's seg / n_hits may be
 * such memory).  rox_pin_host_memory page-locks [p, p + bytes) -- ordinary or
 * MAP_SHARED memory, e.g. a segment several ranks of a node map (the multi-GPU
 * spot diagram: every rank's kernel writes its packed hits over its own PCIe link
 * into the consumer's address space) -- and returns the pointer device code uses
 * for it.  The registration lasts until rox_unpin_host_memory(p).               */
int rox_pin_host_memory(void *p, size_t bytes, void **device_ptr);
int rox_unpin_host_memory(void *p);
/* An asynchronous copy of `bytes` bytes in the order of `stream` between any two of device
 * memory, page-locked host memory and memory registered with rox_pin_host_memory (copy
 * engine; no kernel).  The pipelined multi-GPU spot diagram moves a row block's packed pairs
 * to the consumer's host memory with it while the next block is being traced.          */
int rox_copy_async(void *dst, const void *src, size_t bytes, void *stream);
/* Wait until everything enqueued on `stream` (a hipStream_t, NULL = the default stream) has
 * finished: the trace entries with device / pinned pointers and rox_copy_async return as soon
 * as their work is enqueued.  For callers that do not link the HIP runtime themselves
 * (examples/spot_diagram.c); the Python engine waits through torch's stream instead.        */
int rox_synchronize(void *stream);

/* system table ----------------------------------------------------------- */
/* rows[n_ifcs]; n_table[n_wvls][n_ifcs], n_table[w][i] = refractive index of
 * the gap after interface i at wavelength w (unsigned, sequential.py:649-655;
 * the last column is unused); wvls[n_wvls] = the wavelengths in nm (read by
 * phase elements only; may be NULL when no row carries one).  The handle's
 * table is immutable: a model edit means a new handle (mirrors
 * path_sequence.cache_clear(), sequential.py:666-668).
 *
 * Threading: launches on different HIP streams and from different host threads
 * may share one handle -- per-launch scratch (cached pupil axes, compaction
 * state) is kept per stream behind a mutex.  Launches on one stream run in
 * stream order as usual.  The scratch of a stream (a few KB, plus the staging
 * arena of ROX_HOST_POINTERS calls made on it) lives until rox_system_destroy:
 * use a bounded set of streams per handle, and do not issue device-pointer
 * launches on one stream from two host threads at once (ROX_HOST_POINTERS
 * calls, which are synchronous, take turns per stream by themselves). */
int rox_system_create(const rox_surface *rows, int32_t n_ifcs,
                      const double *n_table, const double *wvls, int32_t n_wvls,
                      rox_system **out_sys);
int rox_system_destroy(rox_system *sys);
/* number of segments a FULL packet holds (n_ifcs minus filtered phantoms) */
int rox_system_num_segments(const rox_system *sys, uint32_t flags,
                            int32_t *n_seg);

/* vignetting search ------------------------------------------------------ */
/* One problem per (field, pupil direction): vigcalc.calc_vignetted_ray
 * (rayoptics/raytr/vigcalc.py:259-340) -- trace the pupil-edge ray with aperture
 * checks (pt_inside_fuzz 1e-4); where it is clipped, iterate the pupil coordinate
 * (iterate_pupil_ray, vigcalc.py:396-461: scipy's secant, tol 1e-6, on rays traced
 * without aperture checks) until the ray grazes that aperture's edge
 * (edge_pt_target, rayoptics/elem/surface.py:210-218, 422-427, 459-464,
 * rayoptics/seq/interface.py:94-111); repeat until no other aperture clips.  The
 * four directions of calc_vignetting_for_field (vigcalc.py:233-256) of every
 * field run as lanes of one launch.  probs / vig / clip are host memory;
 * synchronous. */
typedef struct rox_vig {
    rox_field fld;           /* ray-start constants of the field               */
    double start_dir[2];     /* pupil.pupil_rays[1 + i]                         */
    double unit_dir[2];      /* normalize(start_dir), as NumPy forms it         */
    int32_t xy;              /* i // 2: the pupil axis searched                 */
    int32_t wvl_idx;
    int32_t stop_surf;       /* seq_model.stop_surface, < 0: floating stop      */
    int32_t max_iter;        /* max_iter_count (50)                             */
} rox_vig;                   /* 240 bytes */
int rox_calc_vignetting(rox_system *sys, int32_t n, const rox_vig *probs,
                        double eps, double *vig, int32_t *clip_surf, void *stream);

/* vigcalc.iterate_pupil_ray (rayoptics/raytr/vigcalc.py:396-461) on its own -- what
 * vigcalc.set_pupil (:123-230, from the stop size to the pupil specification) iterates the
 * axial marginal ray through the edge of the stop with: scipy's secant iteration (tol 1e-6)
 * of the pupil coordinate `xy` from start_r0 until the ray, traced without aperture checks,
 * meets interface `indx` at the radius r_target (the reference's "raised before the surface
 * => 0.9 x that trial" rule included).  start_r[n] = the pupil coordinate found. */
typedef struct rox_pupil_iter {
    rox_field fld;           /* ray-start constants of the field               */
    double start_r0;
    double r_target;
    int32_t xy;              /* 0 / 1: the pupil axis iterated                  */
    int32_t wvl_idx;
    int32_t indx;            /* the interface whose edge is the target          */
    int32_t pad;
} rox_pupil_iter;            /* 224 bytes */
int rox_iterate_pupil_rays(rox_system *sys, int32_t n, const rox_pupil_iter *probs,
                           double eps, double *start_r, void *stream);

/* point spread function ---------------------------------------------------
 * analyses.calc_psf(wavefront, ndim, maxdim) (rayoptics/raytr/analyses.py:848-875;
 * callers: analyses.update_psf_data :878-883, mpl/analysisfigure.py:418).
 * opd: [ndim][ndim] OPD in waves as ROX_OUT_OPD / eval_wavefront produce it, NaN =
 * no data; psf: [maxdim][maxdim], the normalised |FFT|^2 of the zero-padded pupil
 * function with the reference's fftshift conventions.  ndim must be even and the
 * block must fit (maxdim/2 + ndim/2 + 1 <= maxdim) -- the shapes for which the
 * reference's slice assignment is valid; maxdim need not be a power of two.
 * Computed as a pruned DFT (two complex GEMMs on the fp64 matrix cores).
 * flags: 0 (device pointers, asynchronous on `stream`) or ROX_HOST_POINTERS. */
int rox_calc_psf(const double *opd, int32_t ndim, int32_t maxdim, double *psf,
                 uint32_t flags, void *stream);

/* trace entries ---------------------------------------------------------- */
/* explicit rays: pt0, dir0 are SoA [3][n_rays] with leading dimension
 * n_rays; wvl_idx is [n_rays] or NULL (then wvl_idx_all is used for all).
 * `stream` is a hipStream_t (NULL = the default stream); the call is
 * asynchronous with respect to the host unless ROX_HOST_POINTERS is set. */
int rox_trace_rays(rox_system *sys, int64_t n_rays,
                   const double *pt0, const double *dir0,
                   const int32_t *wvl_idx, int32_t wvl_idx_all,
                   const rox_opts *opts, const rox_out *out, void *stream);

/* rays generated on the device from a pupil grid or fan */
int rox_trace_pupil_grid(rox_system *sys, const rox_field *fld,
                         const rox_grid *grid, int32_t wvl_idx,
                         const rox_opts *opts, const rox_out *out,
                         void *stream);

/* the same grid for n_grids (field, wavelength) pairs in ONE launch: item i traces
 * flds[i] at wvl_idx[i] with opts[i] into outs[i] -- the per-wavelength loop of
 * SequentialModel.trace_grid / trace_wavefront (rayoptics/seq/sequential.py:1058-1114)
 * and the per-field loops of the figures that call them
 * (rayoptics/mpl/axisarrayfigure.py:213-262).  Every item behaves exactly as the
 * rox_trace_pupil_grid call with the same arguments.  out_mode and
 * ROX_FILTER_PHANTOMS must be the same for all items; device pointers only
 * (no ROX_HOST_POINTERS), no ROX_HITS_APPEND; with ROX_OUT_HITS_COMPACT every item
 * has its own outs[i].seg and outs[i].n_hits. */
int rox_trace_pupil_grids(rox_system *sys, int32_t n_grids, const rox_field *flds,
                          const int32_t *wvl_idx, const rox_grid *grid,
                          const rox_opts *opts, const rox_out *outs, void *stream);

/* rays generated on the device from explicit pupil coordinates px,py[n_rays] */
int rox_trace_pupil_list(rox_system *sys, const rox_field *fld,
                         int64_t n_rays, const double *px, const double *py,
                         int32_t wvl_idx, const rox_opts *opts,
                         const rox_out *out, void *stream);

/* What a spot diagram's consumers reduce the image-plane hits to, computed on the device from
 * the output of a ROX_OUT_HITS launch (layout ROX_SPOT_ROWS: seg = (x, y)[2][ld] + status, rays
 * that did not reach the image skipped) or of a ROX_OUT_HITS_COMPACT launch (ROX_SPOT_PAIRS: seg
 * = interleaved pairs, status NULL, the count read from n_hits on the device when given):
 *   summary  count, sum x, sum y, sum x^2, sum y^2 (centroid, RMS spot radius), min / max of x and
 *            y -- RayGeoPSF.ray_data_bounds (rayoptics/mpl/analysisfigure.py:237-248);
 *   hist     optional [n_x_edges - 1][n_y_edges - 1] counts = numpy.histogram2d(x, y,
 *            bins=[x_edges, y_edges]) as RayGeoPSF.plot's `ax.hist2d` calls it (:250-290):
 *            edges[i] <= v < edges[i + 1], the last bin closed on the right, values outside
 *            dropped.  x_edges / y_edges / summary / hist are HOST pointers; the call is
 *            synchronous (two launches on `stream` + one synchronise).                      */
enum { ROX_SPOT_ROWS = 0, ROX_SPOT_PAIRS = 1 };
typedef struct rox_spot_summary {
    int64_t n;               /* entries counted                                 */
    double sum[2];           /* sum x, sum y                                    */
    double sum_sq[2];        /* sum x^2, sum y^2                                */
    double min[2], max[2];   /* +inf / -inf when n == 0                         */
} rox_spot_summary;          /* 72 bytes */
int rox_spot_stats(const double *seg, int64_t ld, const uint8_t *status, const int64_t *n_hits,
                   int64_t n, int32_t layout, const double *x_edges, int32_t n_x_edges,
                   const double *y_edges, int32_t n_y_edges, rox_spot_summary *summary,
                   uint32_t *hist, void *stream);

/* Through-focus scan: trace a pupil grid ONCE and evaluate every ray at n_planes focus
 * positions in the same launch -- the refocus functions analyses.focus_wavefront /
 * focus_fan / focus_pupil_coords (rayoptics/raytr/analyses.py:313-342, 561-580, 769-791),
 * which re-evaluate traced rays at a new defocus `foc`, over a whole range of focus shifts.
 * A plane carries what a ROX_OUT_FAN launch reads from rox_opts: foc, image_pt and wf.
 *
 *   rows   optional DEVICE array [n_planes][3][ld]: plane k's (x abr, y abr, OPD) of ray r at
 *          rows[(k*3 + c)*ld + r].  Bit-identical to the seg[3][ld] that n_planes
 *          rox_trace_pupil_grid calls with out_mode ROX_OUT_FAN and that plane's foc /
 *          image_pt / wf write: every entry of a ray with status ROX_OK is the same IEEE
 *          double; the entries of a ray that fails are not written, as a FAN launch leaves
 *          them.  ld >= the number of rays of the grid.
 *   status optional DEVICE array [rays]: the per-ray status (as rox_out.status).
 *   stats  optional [n_planes] rox_focus_stats, host or device memory, over the rays with
 *          status ROX_OK.  Reduced in the kernel (per-wave partial records, summed in a fixed
 *          order by a finishing pass; no floating-point atomics): two identical calls give
 *          bit-identical statistics.  A host destination makes the call synchronous.
 *   rows and stats may not both be NULL.
 *
 * planes is HOST memory (copied before the call returns).
 * opts supplies flags, first_surf / last_surf, eps and fuzz; its out_mode must be ROX_OUT_FAN,
 * its foc / image_pt / wf are ignored in favour of planes[].  ROX_HOST_POINTERS is not
 * accepted.  ROX_FAST_FP64 runs the tolerance-mode kernels: the rows then equal those of
 * n_planes tolerance-mode FAN launches (within ~1e-13 relative of the exact values, the same
 * per-ray status).  Pupil grids of kind ROX_GRID_PRODUCT and ROX_GRID_FAN at one wavelength,
 * at most 2^28 rays.  Argument errors (n_planes outside [1, ROX_MAX_FOCUS_PLANES], NULL planes,
 * ld below the ray count, both outputs NULL, another out_mode, a plane whose wf could not be
 * traced by a FAN launch, a wvl_idx outside the system's wavelengths) return ROX_E_ARG before
 * anything is enqueued.  Asynchronous on `stream` unless stats is host memory.           */
#define ROX_MAX_FOCUS_PLANES 256
typedef struct rox_focus_plane {
    double foc;              /* defocus (rox_opts.foc of a FAN launch)                      */
    double image_pt[2];      /* fld.ref_sphere[0][:2] (rox_opts.image_pt)                   */
    double reserved;         /* 0                                                           */
    rox_wavefront wf;        /* this focus's reference sphere (rox_opts.wf); kind per plane  */
} rox_focus_plane;           /* 544 bytes */
typedef struct rox_focus_stats {
    int64_t n;               /* rays with status ROX_OK                                     */
    double cx, cy;           /* centroid: sum x / n, sum y / n                              */
    double rms_spot;         /* sqrt(sum((x - cx)^2 + (y - cy)^2) / n): about the centroid */
    double rms_spot_image_pt;/* sqrt(sum(x^2 + y^2) / n): about image_pt                   */
    double opd_mean;         /* sum OPD / n, system units (as rows)                        */
    double opd_rms;          /* sqrt(sum((OPD - opd_mean)^2) / n): about the mean          */
    double opd_min, opd_max; /* every field but n is NaN when n == 0.  Means and squared
                                deviations are merged pairwise (Chan, Golub & LeVeque), not
                                formed as sum(v^2)/n - mean^2: no cancellation on a large
                                OPD piston                                                  */
} rox_focus_stats;           /* 72 bytes */
int rox_trace_through_focus(rox_system *sys, const rox_field *fld, const rox_grid *grid,
                            int32_t wvl_idx, const rox_opts *opts,
                            int32_t n_planes, const rox_focus_plane *planes,
                            double *rows, int64_t ld, uint8_t *status,
                            rox_focus_stats *stats, void *stream);

/* n_items through-focus scans in ONE launch -- the (field x wavelength) loops of
 * SequentialModel.trace_grid / trace_wavefront (rayoptics/seq/sequential.py:1058-1114) over the
 * refocus functions above: field curvature, focal shift and a white-light best focus from one
 * call.  Item i is exactly
 *   rox_trace_through_focus(sys, &flds[i], &grids[i], wvl_idx[i], &opts[i],
 *                           n_planes, planes + i*n_planes, ...)
 * with its rows at rows + i*n_planes*3*ld, its status at status + i*ld and its statistics at
 * stats + i*n_planes: rows, status and statistics are bit-identical to that single call (the
 * same workgroup size, workgroup count and merge order per item).
 *   grids  per item: start / stop may differ (each field's vignetting box, trace_wavefront);
 *          kind, num and row_begin / row_count must be the same, so every item has R rays.
 *   opts   per item: out_mode ROX_OUT_FAN; ROX_FILTER_PHANTOMS, ROX_FAST_FP64, first_surf and
 *          last_surf the same for every item.  ROX_HOST_POINTERS / ROX_HITS_APPEND are refused.
 *   planes HOST [n_items][n_planes]; rows DEVICE [n_items][n_planes][3][ld] or NULL; status
 *          DEVICE [n_items][ld] or NULL; stats host or device [n_items][n_planes] or NULL (not
 *          both rows and stats NULL).
 * Argument errors (n_items outside [1, ROX_MAX_FOCUS_ITEMS], n_planes outside
 * [1, ROX_MAX_FOCUS_PLANES], NULL arrays, ld < R, a grid or options mismatch, a bad plane wf,
 * a wvl_idx outside the system) return ROX_E_ARG naming the item and plane before anything is
 * enqueued.  Asynchronous on `stream` unless stats is host memory.                            */
#define ROX_MAX_FOCUS_ITEMS 1024
int rox_trace_through_focus_grids(rox_system *sys, int32_t n_items, const rox_field *flds,
                                  const int32_t *wvl_idx, const rox_grid *grids,
                                  const rox_opts *opts, int32_t n_planes,
                                  const rox_focus_plane *planes,
                                  double *rows, int64_t ld, uint8_t *status,
                                  rox_focus_stats *stats, void *stream);

/* Diffraction through focus: the PSF and Strehl ratio of every plane of a through-focus scan,
 * read straight from the rows the two entries above write (the refocus of
 * analyses.focus_wavefront, rayoptics/raytr/analyses.py:769-791, followed by calc_psf,
 * :848-875, at every focus).
 *   rows   DEVICE [n_items][n_planes][3][ld], status DEVICE [n_items][ld] (the through-focus
 *          layouts).  Plane (i, k) reads component 2 (OPD, system units) of the first
 *          ndim*ndim rays, ray r = a*ndim + b being grid[a][b].
 *   wave_scale  HOST [n_items]: the OPD grid in waves of plane (i, k) is
 *          wave_scale[i] * rows[i][k][2][r] where status[i][r] == ROX_OK, NaN elsewhere (one
 *          IEEE product, as focus_wavefront forms convert_to_opd*opdelta).
 *   psf    DEVICE [n_items][n_planes][maxdim][maxdim] or NULL: each plane bit-identical to
 *          rox_calc_psf of that plane's OPD grid (same phase, twiddles, GEMM tiles and k order).
 *   stats  host or device [n_items][n_planes] or NULL (not both psf and stats NULL).
 *          strehl = |sum_ok exp(i 2 pi W)|^2 / n^2 over the OPD itself (a perfect wavefront
 *          gives exactly 1), reduced in a fixed order: identical calls give bit-identical
 *          statistics.  A host destination makes the call synchronous.
 * ndim even with its block inside maxdim (the rox_calc_psf rules), n_items in
 * [1, ROX_MAX_FOCUS_ITEMS], n_planes in [1, ROX_MAX_FOCUS_PLANES], ld >= ndim*ndim, finite
 * wave_scale; argument errors return ROX_E_ARG naming the parameter before anything is
 * enqueued.  Scratch is bounded per launch; larger batches run as consecutive launches with
 * the same results.  Asynchronous on `stream` unless stats is host memory.                   */
typedef struct rox_focus_psf_stats {
    int64_t n;               /* rays with status ROX_OK on this plane's grid                */
    double strehl;           /* |sum_ok exp(i 2 pi W)|^2 / n^2; NaN if n == 0               */
    double psf_peak;         /* AP_max: the max of |F P F^T|^2 the returned PSF was divided by */
    double reserved;
} rox_focus_psf_stats;       /* 32 bytes */
int rox_focus_psf(int32_t n_items, int32_t n_planes, const double *rows, int64_t ld,
                  const uint8_t *status, const double *wave_scale, int32_t ndim, int32_t maxdim,
                  double *psf, rox_focus_psf_stats *stats, void *stream);

/* MTF through focus: the line OTFs of every PSF rox_focus_psf writes, along image x and y.
 * A PSF is M x M (M = maxdim); axis 0 is the pupil / image x direction (grid[a][b], a stepping
 * pupil x), axis 1 is y, pixel (M/2, M/2) is the plane's image point, and pixel j of direction
 * d sits at image coordinate -p (j - M/2), p the plane's pitch (calc_psf_scaling's delta_xp,
 * rayoptics/raytr/analyses.py:818-845).  The sign puts the OTF phase in image coordinates: the
 * PSF's centroid there has the sign of the geometric spot centroid about the image point.
 *   LSF_x[j] = sum_l PSF[j][l],  LSF_y[l] = sum_j PSF[j][l]
 *   OTF_d(nu) = sum_j LSF_d[j] exp(+2 pi i nu p (j - M/2)) / sum_j LSF_d[j],  MTF = |OTF|
 * (the DTFT at nu cycles per system unit; at nu = m / (M p) the normalised circular
 * autocorrelation of calc_psf's padded pupil array).
 *   psf    DEVICE [n_items][n_planes][maxdim][maxdim] (the rox_focus_psf layout)
 *   pitch  HOST [n_items][n_planes], each finite and > 0
 *   freqs  HOST [n_freq], each finite and >= 0 (cycles per system unit: lp/mm for a mm system)
 *   otf    host or device [n_items][n_planes][2][n_freq][2]: (re, im), direction 0 = x, 1 = y.
 *          nu = 0 gives exactly (1, 0) (the normaliser is the zero-phase DTFT's sum, in its
 *          order).  NaN where nu p > 1/2 (above the PSF grid's Nyquist frequency) or where the
 *          PSF's sum is not positive and finite (a plane no ray reached).  Reduced in a fixed
 *          order without atomics: identical calls give bit-identical results.  A host
 *          destination makes the call synchronous.
 * n_items in [1, ROX_MAX_FOCUS_ITEMS], n_planes in [1, ROX_MAX_FOCUS_PLANES], maxdim in
 * [2, 32768], n_freq in [1, ROX_MAX_MTF_FREQS]; argument errors return ROX_E_ARG naming the
 * parameter before anything is enqueued.  Scratch is bounded per launch; larger stacks run as
 * consecutive launches with the same results.  Asynchronous on `stream` unless otf is host
 * memory.                                                                                       */
#define ROX_MAX_MTF_FREQS 1024
int rox_focus_mtf(int32_t n_items, int32_t n_planes, const double *psf, int32_t maxdim,
                  const double *pitch, int32_t n_freq, const double *freqs,
                  double *otf, void *stream);

/* Encircled energy through focus, geometric: ray counts within radii and the radii that hold
 * given fractions of the rays, for the spot of every plane of a through-focus scan.
 *   rows, status  DEVICE [n_items][n_planes][3][ld] and [n_items][ld] (the through-focus
 *          layouts): components 0 and 1 are x abr and y abr about the plane's image point.  Only
 *          the first n_rays rays count, and of those only the ones with status ROX_OK; the rows
 *          of a failed ray are never read.
 *   centers  HOST [n_items][n_planes][2], finite, in the rows' coordinates; NULL = (0, 0).
 *          d2 = dx*dx + dy*dy with dx = x - cx, dy = y - cy: each step one IEEE binary64
 *          operation in this order, no contraction into FMA.
 *   radii  HOST [n_items][n_planes][n_radii], each finite and >= 0, non-decreasing within a
 *          plane (read only with counts).
 *   counts optional, host or device [n_items][n_planes][n_radii]: the number of OK rays with
 *          d2 <= r*r (r*r one IEEE product).  Exact.
 *   fractions  HOST [n_frac], each in (0, 1] (read only with ee_radius).
 *   ee_radius  optional, host or device [n_items][n_planes][n_frac]: sqrt(D(m)), D(1) <= ... <=
 *          D(n) the plane's sorted d2 and m = clamp(ceil(fractions[q] * n), 1, n) (the product
 *          one IEEE product): an exact order statistic (fraction 1: the farthest ray).  NaN
 *          where n == 0.
 *   n_ok   optional, host or device [n_items][n_planes]: the OK ray count n.
 * counts and ee_radius may not both be NULL.  n_items in [1, ROX_MAX_FOCUS_ITEMS], n_planes in
 * [1, ROX_MAX_FOCUS_PLANES], n_rays in [1, ld], n_radii in [0, ROX_MAX_EE_RADII] (>= 1 with
 * counts), n_frac in [0, ROX_MAX_EE_FRACTIONS] (>= 1 with ee_radius).  Integer histograms and a
 * radix select on the bit patterns of d2; identical calls give bit-identical results, host and
 * device destinations alike.  Argument errors return ROX_E_ARG naming the parameter before
 * anything is enqueued.  Scratch is bounded per launch; larger jobs run as consecutive launches
 * with the same results.  Asynchronous on `stream` unless an output is host memory.          */
#define ROX_MAX_EE_RADII     1024
#define ROX_MAX_EE_FRACTIONS   64
int rox_focus_ee(int32_t n_items, int32_t n_planes, const double *rows, int64_t ld,
                 const uint8_t *status, int64_t n_rays, const double *centers,
                 int32_t n_radii, const double *radii, int64_t *counts,
                 int32_t n_frac, const double *fractions, double *ee_radius,
                 int64_t *n_ok, void *stream);

/* Geometric MTF and line spread through focus: the OTF of the ray spot along given directions,
 * and the histogram of the rays projected on them, for every plane of a through-focus scan.
 *   rows, status  DEVICE [n_items][n_planes][3][ld] and [n_items][ld] (the through-focus
 *          layouts): components 0 and 1 are x abr and y abr about the plane's image point.  Only
 *          the first n_rays rays count, and of those only the ones with status ROX_OK; the rows
 *          of a failed ray are never read.
 *   dirs   HOST [n_items][n_dir][2] = (ex, ey), finite and not both zero; unit vectors are
 *          expected but not checked.  u = ex*x + ey*y: two IEEE binary64 products and one sum,
 *          no contraction into FMA, so (1, 0) and (0, 1) give exactly x and y.
 *   freqs  HOST [n_freq], each finite and >= 0 (cycles per system unit), in any spacing; there
 *          is no Nyquist limit (read only with otf).
 *   otf    optional, host or device [n_items][n_planes][n_dir][n_freq][2] = (re, im):
 *          OTF_d(nu) = (1/n) sum_ok exp(-2 pi i nu u), the phase convention of rox_focus_mtf
 *          (the low-frequency phase is -2 pi nu times the spot centroid along the direction).
 *          Per term t = nu*u (one product), r = t - rint(t) (exact), then sincospi(2 r);
 *          re = sum cos and im = -sum sin, each reduced in a fixed order without atomics, then
 *          one IEEE division by n.  nu = 0 gives exactly (1, 0).  NaN where n == 0.
 *   edges  HOST [n_items][n_planes][n_dir][n_bins + 1], finite and strictly increasing per
 *          (item, plane, direction) (read only with lsf).
 *   lsf    optional, host or device [n_items][n_planes][n_dir][n_bins]: the number of OK rays
 *          whose u lies in each bin as numpy.histogram(u, edges) decides it: half-open bins,
 *          the last one closed, rays outside not counted.  Exact.
 *   n_ok   optional, host or device [n_items][n_planes]: the OK ray count n.
 * otf and lsf may not both be NULL.  n_items in [1, ROX_MAX_FOCUS_ITEMS], n_planes in
 * [1, ROX_MAX_FOCUS_PLANES], n_rays in [1, ld], n_dir in [1, ROX_MAX_GMTF_DIRS], n_freq in
 * [0, ROX_MAX_MTF_FREQS] (>= 1 with otf), n_bins in [0, ROX_MAX_LSF_BINS] (>= 1 with lsf).
 * Identical calls give bit-identical results, host and device destinations alike.  Argument
 * errors return ROX_E_ARG naming the parameter (and the index of a bad element) before anything
 * is enqueued.  Scratch is bounded per launch; larger jobs run as consecutive launches with the
 * same results.  Asynchronous on `stream` unless an output is host memory.                    */
#define ROX_MAX_GMTF_DIRS   8
#define ROX_MAX_LSF_BINS 4096
int rox_focus_gmtf(int32_t n_items, int32_t n_planes, const double *rows, int64_t ld,
                   const uint8_t *status, int64_t n_rays,
                   int32_t n_dir, const double *dirs,
                   int32_t n_freq, const double *freqs, double *otf,
                   int32_t n_bins, const double *edges, int64_t *lsf,
                   int64_t *n_ok, void *stream);

/* Encircled energy through focus, diffraction: the fraction of every PSF rox_focus_psf writes
 * that lies within given radii.  Orientation as rox_focus_mtf: pixel (j, l) sits at image
 * (X, Y) = (-p (j - M/2), -p (l - M/2)) about the plane's image point, M = maxdim.
 *   psf    DEVICE [n_items][n_planes][maxdim][maxdim] (the rox_focus_psf layout)
 *   pitch  HOST [n_items][n_planes], each finite and > 0
 *   centers  HOST [n_items][n_planes][2], finite, in those coordinates; NULL = each PSF's own
 *          centroid.
 *   radii  HOST [n_items][n_planes][n_radii], each finite and >= 0, non-decreasing per plane
 *   ee     host or device [n_items][n_planes][n_radii]: the sum of the PSF over the pixels whose
 *          centre has d2 <= r*r (d2 formed from X - cx and Y - cy as rox_focus_ee forms it),
 *          divided by the sum over all pixels.  Numerator and denominator are reduced in the
 *          same fixed order: a radius covering every pixel gives exactly 1.0.  NaN where the
 *          PSF's sum is not positive and finite.
 *   centroid  optional, host or device [n_items][n_planes][2]: sum(X PSF) / sum(PSF) and
 *          likewise for Y, written whether or not it served as the centre (NaN where the sum is
 *          not positive and finite).
 * No floating-point atomics: identical calls give bit-identical results.  n_items in
 * [1, ROX_MAX_FOCUS_ITEMS], n_planes in [1, ROX_MAX_FOCUS_PLANES], maxdim in [2, 32768], n_radii
 * in [1, ROX_MAX_EE_RADII]; argument errors return ROX_E_ARG naming the parameter before
 * anything is enqueued.  Scratch is bounded per launch; larger stacks run as consecutive
 * launches with the same results.  Asynchronous on `stream` unless an output is host memory. */
int rox_focus_psf_ee(int32_t n_items, int32_t n_planes, const double *psf, int32_t maxdim,
                     const double *pitch, const double *centers, int32_t n_radii,
                     const double *radii, double *ee, double *centroid, void *stream);

/* Zernike fits of the wavefront through focus: the least-squares coefficients of the OPD of
 * every plane of a through-focus scan in a given Zernike basis.
 *   rows, status  DEVICE [n_items][n_planes][3][ld] and [n_items][ld] (the through-focus
 *          layouts).  Only component 2 (OPD) is read: W = wave_scale[i] * rows[i][k][2][r] in
 *          waves (one IEEE product); the rows of a ray that is not fitted are never read.
 *   grids  HOST [n_items]: each ROX_GRID_PRODUCT and whole (row_begin 0, row_count 0 or num),
 *          num >= 2; start and stop may differ per item.  Ray r = a*num + b sits at pupil
 *          (px[a], py[b]), each axis built from start by repeated += of (stop - start)/(num - 1)
 *          in binary64, the doubles the trace started the ray from.
 *   circle HOST [n_items][3]: (cx, cy, radius) in pupil coordinates, finite, radius > 0; NULL =
 *          (0, 0, 1).  x = (px - cx) / radius, y = (py - cy) / radius; a ray is fitted when its
 *          status is ROX_OK and x*x + y*y <= 1 (two products, then the sum, no FMA).
 *   wave_scale  HOST [n_items], finite.
 *   terms  HOST [n_terms]: term j is scale * R_n^|m|(rho) * {1 | cos(m theta) | sin(|m| theta)}
 *          for m = 0, m > 0, m < 0, x = rho cos theta, y = rho sin theta.  Evaluated as
 *          P(rho^2) * Re/Im((x + i y)^|m|), P the radial polynomial over rho^|m| with scale
 *          folded into its integer coefficients, by Horner from the highest power.
 *          1 <= n_terms <= ROX_MAX_ZERNIKE_TERMS, 0 <= n <= ROX_MAX_ZERNIKE_ORDER, |m| <= n,
 *          n - |m| even, finite scale.
 *   coef   optional, host or device [n_items][n_planes][n_terms], waves.
 *   stats  optional, host or device [n_items][n_planes].
 * coef and stats may not both be NULL.  Normal equations G c = Z^T W (G = Z^T Z, the same for
 * every plane) accumulated with f64 MFMA in a fixed order, a Jacobi-equilibrated Cholesky
 * solve, and one step of iterative refinement from a second read of the rows (c += G^-1 Z^T r);
 * a third read forms the residual statistics from the residuals themselves.  fit = 1 where
 * n < n_terms (n = 0 included), fit = 2 where a Cholesky pivot of the equilibrated G is not
 * above 1e-12 (singular or ill-conditioned); either gives NaN coefficients, rms_residual and
 * pv_residual.  cond is max/min pivot of the equilibrated G (1/pivot at the failing pivot with
 * fit = 2, NaN with fit = 1).  No floating-point atomics: identical calls give bit-identical
 * results, host and device destinations alike.  Argument errors return ROX_E_ARG naming the
 * parameter and item before anything is enqueued.  Scratch is bounded per launch; larger jobs
 * run as consecutive launches with the same results.  Asynchronous on `stream` unless an output
 * is host memory.                                                                            */
#define ROX_MAX_ZERNIKE_TERMS 91      /* every term up to radial order 12 */
#define ROX_MAX_ZERNIKE_ORDER 20
typedef struct rox_zernike_term {
    int32_t n, m;
    double scale;
} rox_zernike_term;           /* 16 bytes */
typedef struct rox_zernike_stats {
    int64_t n;                /* rays fitted: status ROX_OK and inside the unit circle       */
    int64_t n_outside;        /* ROX_OK rays outside the circle (not fitted, counted)         */
    double rms;               /* sqrt(sum (W - mean W)^2 / n) over the fitted rays, waves     */
    double rms_residual;      /* sqrt(sum (W - sum_j c_j Z_j)^2 / n), waves                   */
    double pv_residual;       /* max - min of the residuals, waves                            */
    double cond;              /* max / min Cholesky pivot of the equilibrated G               */
    int32_t fit;              /* 0 fitted; 1 n < n_terms; 2 singular / ill-conditioned        */
    int32_t reserved;
} rox_zernike_stats;          /* 56 bytes */
int rox_focus_zernike(int32_t n_items, int32_t n_planes, const double *rows, int64_t ld,
                      const uint8_t *status, const rox_grid *grids, const double *circle,
                      const double *wave_scale, int32_t n_terms, const rox_zernike_term *terms,
                      double *coef, rox_zernike_stats *stats, void *stream);

/* Beam footprints: per-surface reductions of the ROX_OUT_FULL packets of finished launches --
 * how large the beam is on every interface, where it lands, how steeply it arrives and where
 * rays are lost -- computed where the packets are (HBM).
 *   trace_flags  the rox_opts.flags the packets were traced with; only ROX_FILTER_PHANTOMS is
 *          read: it decides n_seg = rox_system_num_segments(sys, trace_flags) and which
 *          interface a slot holds.
 *   outs   HOST [n_items] of DEVICE pointers: the rox_out of each FULL launch (an item of
 *          rox_trace_pupil_grids, a rox_trace_pupil_grid or rox_trace_rays call).  seg
 *          [n_seg][10][ld], status, fail_surf and ld are read, of the first n_rays rays.
 *   Records.  With nb[s] = the number of slots before interface s, ray r has nseg(r) records:
 *          n_seg when its status is ROX_OK; 0 when fail_surf <= 0 (or not an interface);
 *          nb[fail_surf - 1] + 1 when ROX_MISSED_SURFACE; nb[fail_surf] + 1 otherwise, the last
 *          of those being the partial record [inc_pt, before_dir, 0, normal].  Slot k of ray r
 *          is read only when k < nseg(r).  A full segment counts always, a partial record only
 *          with ROX_FP_PARTIAL (the reference's `len(ray) > i` test in
 *          vigcalc.max_aperture_at_surf, rayoptics/raytr/vigcalc.py:31-42); with
 *          ROX_FP_OK_ONLY only rays with status ROX_OK count.
 *   fp     optional, host or device [n_items][n_seg] rox_footprint.
 *   half_width  HOST [n_seg], finite and > 0 (read only with maps).
 *   maps   optional, host or device [n_items][n_seg][n_bins][n_bins] uint32:
 *          numpy.histogram2d(x, y, bins=n_bins, range=[[-h, h], [-h, h]]) of the counted
 *          records of the slot, h = half_width[k] (x is the first axis).  Edge j is
 *          -h + j * (2h / n_bins) (one quotient, one product, one sum), the last edge h; a value
 *          is placed by comparison with the edges: bins are half-open, the last one closed,
 *          values outside are dropped.  n_bins in [1, 512].  Integer atomics: exact.
 * fp and maps may not both be NULL.  n_items in [1, ROX_MAX_FOCUS_ITEMS], n_rays in
 * [1, 2^28], ld >= n_rays.  No floating-point atomics: per-wave partial records merged in a fixed
 * order (Chan / Golub / LeVeque for the centroid and the RMS); identical calls give bit-identical
 * results, host and device destinations alike.  Argument errors return ROX_E_ARG naming the
 * parameter and item before anything is enqueued and leave the outputs untouched.  Scratch is
 * bounded per launch; larger jobs run as consecutive launches with the same results.
 * Asynchronous on `stream` unless an output is host memory.                                 */
#define ROX_FP_PARTIAL 1u
#define ROX_FP_OK_ONLY 2u
typedef struct rox_footprint {
    int64_t n;               /* records counted                                              */
    int64_t n_fail[5];       /* rays that failed at this slot's interface, by status (slot
                                nb[fail_surf]; index 0 unused and 0); no flag changes it     */
    int64_t n_inc;           /* segments in cos_inc_min / cos_inc_sum                        */
    double min[2], max[2];   /* bounding box of (p.x, p.y); empty: +inf / -inf               */
    double r2_max;           /* max of x*x + y*y (two products, one sum; no FMA): an exact
                                selection, sqrt left to the caller; empty: -inf              */
    double cx, cy;           /* centroid                                                     */
    double rms_r;            /* sqrt(sum((x - cx)^2 + (y - cy)^2) / n)                       */
    double cos_inc_min;      /* over full segments, slot k >= 1: min and sum of |b4 . nrml|, */
    double cos_inc_sum;      /*   b4 = slot k-1's direction taken into slot k's frame by the
                                rt (in its rt_order) of every interface in between           */
    double cos_exit_min;     /* over full segments: min of |d . nrml|                        */
} rox_footprint;             /* 144 bytes; cx .. cos_exit_min are NaN where nothing counted   */
int rox_surface_footprints(rox_system *sys, uint32_t trace_flags, uint32_t fp_flags,
                           int32_t n_items, const rox_out *outs, int64_t n_rays,
                           rox_footprint *fp, const double *half_width, int32_t n_bins,
                           uint32_t *maps, void *stream);

/* Fresnel transmission and polarization ray tracing over the ROX_OUT_FULL packets of finished
 * launches: how much of the light of every ray arrives, what each surface costs and how strongly
 * the system polarizes, computed where the packets are (HBM).  Two orthogonal unit field vectors
 * transverse to the ray are carried from the object slot to the image slot; s and p are
 * redefined at every interface, so a skew ray mixes them (the product of (Ts + Tp) / 2 per
 * surface is not the transmission off axis).
 *   trace_flags, outs, n_rays   as rox_surface_footprints; of a slot's 10 rows d and nrml are
 *          read, of rays with status ROX_OK only.
 *   tx_flags   ROX_TX_FIELDS: rows has 10 rows per item, not 4.
 *   wvl_idx    HOST [n_items]: the wavelength each item was traced at (row of n_table).
 *   n_coat, coat_kind, coat_value   optional HOST coating tables: coat_kind[n_coat] int32 ROX_COAT_*
 *          and coat_value[n_coat][2]; n_coat = the system's number of interfaces.  Both NULL
 *          (n_coat ignored): every interface bare.  coat_value is read where the kind is
 *          ROX_COAT_FIXED and must then lie in [0, 1].
 *   rows   optional, host or device [n_items][n_rows][ld_rows], ld_rows >= n_rays; n_rows = 4 or 10.
 *   surf   optional, host or device [n_items][n_seg] rox_tx_surface.
 *   item   optional, host or device [n_items] rox_tx_item.
 * Arithmetic, in operation order (IEEE double, no FMA anywhere in this entry: every step is
 * one NumPy float64 operation).  Dot products are x*x' + y*y' + z*z' summed left to right;
 * a cross product u x v is (u.y*v.z - u.z*v.y, u.z*v.x - u.x*v.z, u.x*v.y - u.y*v.x).
 *   Frames.  A vector v of interface i's frame is taken into the next frame as rt_i . v, rt the
 *          rox_surface.rt of row i: component a = (rt[a][c0]*v[c0] + rt[a][c1]*v[c1]) +
 *          rt[a][2]*v[2] with (c0, c1) = (0, 1) for ROX_RT_F_ORDER and (1, 0) for ROX_RT_C_ORDER
 *          (the interfaces and order of rox_footprint.cos_inc_*, unfused).  From slot k-1 to
 *          slot k every interface slot_ifc[k-1] .. slot_ifc[k] - 1 is applied in turn, to the
 *          previous slot's direction (giving b4) and to the carried E1, E2.
 *   Slot k, interface s = slot_ifc[k]: d = the slot's direction, N = its normal; at slot 0
 *          b4 = d.  ci = |b4 . N|, ct = |d . N|.
 *   Slot 0 (the object) sets the state: a = (d.z, 0, -d.x), a = (1, 0, 0) if a.a == 0;
 *          E1 = a / sqrt(a.a) (the x-like state), E2 = d x E1 (the y-like state), q = 1.
 *   The last slot (the image) changes nothing.
 *   Every slot in between has amplitude coefficients ts, tp, a flux factor qs and power
 *   coefficients Ts, Tp, with n1 = n_table[w][s-1], n2 = n_table[w][s]:
 *          bare     ROX_TRANSMIT, profile not ROX_THINLENS, ph.kind == ROX_PH_NONE, n1 != n2:
 *                   A = n1*ci, B = n2*ct, ts = (A + A) / (A + B), tp = (A + A) / (n2*ci + n1*ct),
 *                   qs = B / A, Ts = qs*(ts*ts), Tp = qs*(tp*tp); ci == 0: ts = tp = qs = 0.
 *          mirror   ROX_REFLECT: ts = -1, tp = 1, qs = 1, Ts = Tp = 1 (an ideal mirror).
 *          ideal    ROX_DUMMY and ROX_PHANTOM interfaces, n1 == n2, thin lenses and phase
 *                   elements (gratings, DOEs, holograms) are COUNTED AS IDEAL: the field is
 *                   carried through the bend with ts = tp = qs = 1, Ts = Tp = 1.
 *          Coatings override the model of a ROX_TRANSMIT or ROX_REFLECT interface:
 *          ROX_COAT_BARE as above; ROX_COAT_IDEAL ts = tp = qs = 1 and Ts = Tp = 1;
 *          ROX_COAT_FIXED (Ts, Tp) = coat_value[s], ts = sqrt(Ts), tp = sqrt(Tp), qs = 1 (on a
 *          mirror these are the reflectances).  On a mirror ts is negated, coated or not.
 *          c = b4 x N; if c.c == 0: c = b4 x (1,0,0) when |b4.x| <= |b4.y|, else b4 x (0,1,0).
 *          s^ = c / sqrt(c.c), p_in = b4 x s^, p_out = d x s^; for E in (E1, E2):
 *          E <- (ts*(s^ . E))*s^ + (tp*(p_in . E))*p_out; q <- q*qs.
 *   Rows of a ray with status ROX_OK, from g11 = E1.E1, g12 = E1.E2, g22 = E2.E2,
 *          m = (g11 + g22)/2, h = (g11 - g22)/2, r = sqrt(h*h + g12*g12):
 *          row 0  T = q*m, the transmission of unpolarized light
 *          row 1  T1 = q*g11    row 2  T2 = q*g22 (the x-like and the y-like input state)
 *          row 3  D = r/m, the diattenuation (0 when m == 0)
 *          rows 4-6 E1, rows 7-9 E2 in the image frame (ROX_TX_FIELDS)
 *          Every row of any other ray is NaN.  Columns n_rays .. ld_rows - 1 are not written.
 * Records are over the rays with status ROX_OK; minima and maxima are exact selections, sums are
 * per-wave partial sums merged in a fixed order by a finishing kernel (no floating-point
 * atomics).  Where nothing counted the sums are 0 and the minima and maxima NaN.
 * rows, surf and item may not all be NULL.  n_items in [1, ROX_MAX_FOCUS_ITEMS], n_rays in
 * [1, 2^28], ld >= n_rays.  Identical calls give bit-identical results, host and device
 * destinations alike.  Argument errors return ROX_E_ARG naming the parameter and item before
 * anything is enqueued and leave the outputs untouched.  Scratch per launch is 32 MiB or, where
 * that is more, what one item needs: 64 bytes of partial records per wave of 128 rays and slot
 * (n_rays * (n_seg + 1) / 2 bytes: 7 MB at 2^20 rays and 13 slots, 1.9 GB at the largest n_rays,
 * 2^28) plus, for rows bound for host memory, 8 MiB of rows.  Larger jobs run as consecutive
 * launches over fewer items (and, for rows bound for host memory, fewer rays) with the same
 * results.  Asynchronous on `stream` unless an output is host memory.
 * Not modelled here: absorption, multilayer coatings, complex (metal) indices (these are
 * rox_surface_thinfilm's, below), diffraction efficiency.                                     */
#define ROX_TX_FIELDS 1u
enum { ROX_COAT_BARE = 0, ROX_COAT_IDEAL = 1, ROX_COAT_FIXED = 2 };
enum { ROX_COAT_STACK = 3 };       /* rox_surface_thinfilm only */
#define ROX_MAX_COAT_LAYERS 64          /* layers of one interface's stack */
#define ROX_MAX_COAT_LAYERS_TOTAL 4096  /* layers of one call */
typedef struct rox_tx_surface {
    int64_t n;               /* rays counted (status ROX_OK)                                 */
    double ts_sum, tp_sum;   /* sums of Ts and of Tp at this slot (object and image: 1)      */
    double t_sum;            /* sum of (Ts + Tp)/2                                            */
    double ts_min, tp_min;
    double ci_sum, ci_min;   /* sum and minimum of ci                                        */
} rox_tx_surface;            /* 64 bytes */
typedef struct rox_tx_item {
    int64_t n_ok;            /* rays with status ROX_OK                                      */
    int64_t n_rays;          /* rays launched (the call's n_rays)                            */
    double t_sum, t_min, t_max;
    double t1_sum, t2_sum;
    double d_sum, d_max;
} rox_tx_item;               /* 72 bytes */
int rox_surface_transmission(rox_system *sys, uint32_t trace_flags, uint32_t tx_flags,
                             int32_t n_items, const rox_out *outs, int64_t n_rays,
                             const int32_t *wvl_idx, int32_t n_coat, const int32_t *coat_kind,
                             const double *coat_value, double *rows, int64_t ld_rows,
                             rox_tx_surface *surf, rox_tx_item *item, void *stream);

/* rox_surface_transmission with thin-film stacks and metal mirrors: the same walk over the same
 * packets with COMPLEX field vectors (a stack's ts and tp differ in phase), and at an interface
 * whose coat_kind is ROX_COAT_STACK the characteristic matrix of its layers evaluated per ray.
 * Everything rox_surface_transmission says about trace_flags, outs, n_rays, wvl_idx, n_coat,
 * coat_kind, coat_value, rows, surf, item, the records, the scratch, the chunking, the
 * destinations and the errors holds here, with these differences:
 *   coat_kind  may also be ROX_COAT_STACK, on an interface between object and image that is
 *          ROX_TRANSMIT (no thin lens, no phase element) or ROX_REFLECT; anywhere else
 *          ROX_E_ARG names the interface.  Both media of a transmitting interface are real
 *          (n_table).
 *   wvl    HOST [n_items]: each item's vacuum wavelength in the unit of layer_thickness, finite
 *          and > 0.
 *   stack_first  HOST int32 [n_coat + 1]: CSR offsets into the layer arrays (stack_first[0] = 0);
 *          only an interface of kind ROX_COAT_STACK has layers, at most ROX_MAX_COAT_LAYERS, and
 *          a call at most ROX_MAX_COAT_LAYERS_TOTAL.  Layers are listed in the order the light
 *          crosses them, from medium s-1 to medium s.  A stack may have 0 layers.
 *   layer_thickness  HOST [n_layers], finite and >= 0.
 *   layer_index  HOST [n_wvls][n_layers][2]: (re, im) of each layer's index per row of n_table,
 *          re > 0, im >= 0: N = n + ik with exp(-iwt), k > 0 absorbs.
 *   sub_index  HOST [n_wvls][n_coat][2]: the complex index of the metal or substrate behind a
 *          ROX_REFLECT interface with a stack (re, im >= 0, not both 0); read only there, and
 *          required if there is one.
 *          wvl, layer_thickness and layer_index may be NULL when there is no layer, stack_first
 *          when no interface has a stack.
 *   tx_flags   ROX_TX_FIELDS: rows has 16 rows per item: rows 4-9 re(E1), re(E2), rows 10-15
 *          im(E1), im(E2).
 * Arithmetic (IEEE double, no FMA; sqrt, division, sincos and exp of the device's library, so a
 * restatement agrees within a bound, not bit for bit).  Complex products are
 * (a.r*b.r - a.i*b.i, a.r*b.i + a.i*b.r); 1/a = (a.r/m, -a.i/m), m = a.r*a.r + a.i*a.i.
 *   Frames, slot 0 and the last slot as above; E1 and E2 start real.  Frames act on the real
 *          and on the imaginary part.
 *   Interfaces of the kinds ROX_COAT_BARE, _IDEAL and _FIXED: exactly the formulas above with the
 *          real ts, tp applied to the real and to the imaginary part of E separately.  A call
 *          without a stack gives rows 0-9 bit-identical to rox_surface_transmission's and rows
 *          10-15 zero.
 *   ROX_COAT_STACK at interface s: A = n1*ci, a2 = (n1*n1)*(1 - ci*ci), B' = n2*ct.  For a medium
 *          of squared index N2 = N*N: g = sqrt(N2 - a2) on the branch Im g >= 0 (Re g >= 0 when
 *          Im g = 0), from z = N2 - a2, m = sqrt(z.r*z.r + z.i*z.i): z.r >= 0: g.r =
 *          sqrt((m + z.r)/2), g.i = z.i/(g.r + g.r) (0 when g.r = 0); else g.i = sqrt((m - z.r)/2),
 *          g.r = z.i/(g.i + g.i).  Admittances: y = g (s), y = N2*(1/g) (p).  z == 0 exactly (the
 *          ray runs along the layer: g = 0, 1/g is not finite) is not defined: that ray's rows
 *          and its share of the sums are NaN although it counts as OK.
 *          Exit side: transmitting ys = B', yp = (n2*n2)/B'; mirror: g from sub_index.
 *          (B, C) = (1, y_exit) for s and for p; att = 0.  Layers from the last to the first, with
 *          kd = (6.283185307179586*d)/wvl, x = kd*g.r, y = kd*g.i, e2 = exp(-(y + y)),
 *          ch = (1 + e2)/2, sh = (1 - e2)/2, cs = (cos(x)*ch, -(sin(x)*sh)), sn = (sin(x)*ch,
 *          cos(x)*sh) -- cos and sin of delta = x + iy over e^y, so nothing overflows -- and
 *          att = att + y:   u = sn*(C*(1/y_j)), v = (y_j*sn)*B,
 *          (B, C) <- (cs*B + (u.i, -u.r), cs*C + (v.i, -v.r)), 1/y_j = 1/g (s), g*(1/N2) (p).
 *          y0 = A (s), (n1*n1)/A (p); den = y0*B + C.
 *          Transmitting: f = exp(-att); ts = (f*(y0s + y0s))*(1/den_s),
 *          tp = ((f*(y0p + y0p))*(ci/ct))*(1/den_p), qs = B'/A; ci == 0: ts = tp = qs = 0.
 *          Without layers this is the bare formula.
 *          Mirror: ts = (y0s*B - C)*(1/den_s), tp = -((y0p*B - C)*(1/den_p)), qs = 1 (ci == 0:
 *          ts = tp = -1): a perfect conductor gives the ideal mirror's (-1, +1).
 *          Ts = qs*|ts|^2, Tp = qs*|tp|^2 (reflectances on a mirror), |t|^2 = t.r*t.r + t.i*t.i.
 *          For E in (E1, E2): a = ts*(s^ . E), b = tp*(p_in . E) (dot products of the real and of
 *          the imaginary part), E <- a*s^ + b*p_out per part; q <- q*qs.
 *   Rows:  g11 = E1r.E1r + E1i.E1i, g22 likewise, g12 = (E1r.E2r + E1i.E2i, E1r.E2i - E1i.E2r)
 *          (Hermitian products), m, h as above, r = sqrt(h*h + (g12.r*g12.r + g12.i*g12.i)).
 * The records' sums are merged over the same waves of 128 rays in the same order as
 * rox_surface_transmission's: without a stack they are its records bit for bit.              */
int rox_surface_thinfilm(rox_system *sys, uint32_t trace_flags, uint32_t tx_flags,
                         int32_t n_items, const rox_out *outs, int64_t n_rays,
                         const int32_t *wvl_idx, const double *wvl, int32_t n_coat,
                         const int32_t *coat_kind, const double *coat_value,
                         const int32_t *stack_first, const double *layer_thickness,
                         const double *layer_index, const double *sub_index, double *rows,
                         int64_t ld_rows, rox_tx_surface *surf, rox_tx_item *item, void *stream);

/* The projected solid angle of the image-space bundle: the signed area the num x num pupil grid
 * of a finished launch covers in the plane of the direction cosines (L, M) it arrives with --
 * for a Lambertian object of uniform radiance the irradiance at the image point is proportional
 * to the integral of T dL dM over that area (conservation of basic radiance; Rimmer, "Relative
 * illumination calculations", Proc. SPIE 655, 1986), which contains cos^4, pupil aberration,
 * distortion and vignetting.  One pass over rows that are already in HBM; no system is needed.
 *   outs   HOST [n_items] of DEVICE pointers: the rox_out of each ROX_GRID_PRODUCT launch of
 *          num x num rays, all rows traced: ray r = i*num + j, x_i outer, y_j inner.  seg, status
 *          and ld are read.  L of ray r is seg[(dir_row + 0)*ld + r], M is seg[(dir_row + 1)*ld + r]:
 *          dir_row = 3 for ROX_OUT_LAST, (n_seg - 1)*10 + 3 for ROX_OUT_FULL (the image slot's d.x
 *          and d.y, in the image interface's frame).  A ray counts iff its status is ROX_OK; the
 *          rows of any other ray are never read.
 *   weight optional DEVICE: ray r of item i has weight weight[i*weight_stride + r], read for
 *          counted rays only (rox_surface_transmission's rows with weight_stride =
 *          n_rows*ld_rows: row 0, T).  NULL: every weight is 1.
 *   item   optional, host or device [n_items] rox_sa_item.
 *   cells  optional, host or device [n_items][num-1][num-1]: the signed, unweighted area of
 *          every cell.
 * Arithmetic, in operation order (IEEE double, no FMA: every step is one NumPy float64
 * operation).  Cell (i, j) has the corners a = (i, j), b = (i+1, j), c = (i+1, j+1), d = (i, j+1)
 * and k counted corners.
 *   k = 4  area = ((Lc - La)*(Md - Mb) - (Ld - Lb)*(Mc - Ma)) * 0.5
 *          weight = ((wa + wb) + (wc + wd)) * 0.25
 *   k = 3  (p, q, r) = the counted corners in the cyclic order a, b, c, d, the missing one skipped:
 *          area = ((Lq - Lp)*(Mr - Mp) - (Lr - Lp)*(Mq - Mp)) * 0.5
 *          weight = ((wp + wq) + wr) / 3.0
 *   k < 3  area = 0.
 * Every ray and every cell is counted exactly once.  Minima and maxima are exact selections; the
 * sums are per-wave partial sums merged in a fixed order by a finishing kernel (no
 * floating-point atomics): identical calls, host and device destinations, and one call over n
 * items against n calls over one item each give the same bits.
 * item and cells may not both be NULL.  n_items in [1, ROX_MAX_FOCUS_ITEMS], num in
 * [2, ROX_MAX_SA_NUM], ld >= num*num, dir_row >= 0, weight_stride >= num*num with weight.
 * Argument errors return ROX_E_ARG naming the parameter and item before anything is enqueued and
 * leave the outputs untouched.  Scratch per launch is 32 MiB or, where that is more, what one
 * item needs (120 bytes of partial records per wave -- 4 MB at num = 16384 -- plus, for cells
 * bound for host memory, the item's cells); larger jobs run as consecutive launches over fewer
 * items with the same results.  Asynchronous on `stream` unless an output is host memory.   */
#define ROX_MAX_SA_NUM 16384
typedef struct rox_sa_item {
    int64_t n_ok;            /* rays counted (status ROX_OK)                                  */
    int64_t n_cells[5];      /* the (num-1)^2 cells by their number k of counted corners      */
    double a_full, a_tri;    /* the signed sums of the k = 4 and of the k = 3 areas           */
    double a_abs;            /* sum of |area| over both: > |a_full + a_tri| where the map folds */
    double aw_full, aw_tri;  /* sums of area*weight; without weight a_full and a_tri bit for bit */
    double l_sum, m_sum;     /* sums of L and of M over the counted rays                      */
    double l_min, l_max, m_min, m_max;
    double r2_max;           /* max of L*L + M*M (two products, one sum): an exact selection  */
} rox_sa_item;               /* 144 bytes; l_min .. r2_max are NaN where nothing counted, the
                                sums are then 0                                               */
int rox_projected_solid_angle(int32_t n_items, int32_t num, const rox_out *outs, int32_t dir_row,
                              const double *weight, int64_t weight_stride, rox_sa_item *item,
                              double *cells, void *stream);

/* Segment foci: where between two interfaces a weighted bundle is smallest, from the
 * ROX_OUT_FULL packets of finished launches.  A ray leaves the interface of slot k on a straight
 * line; per (item, slot) the weighted first and second moments of those lines are reduced where
 * the packets are (HBM), and the host solves a quadratic (below).  rox_surface_footprints gives
 * beam sizes on the interfaces only and takes no weights; this entry serves the ghost analysis
 * (a ghost path is an unfolded table, its rays weighted by rox_surface_thinfilm's row 0).
 *   trace_flags, n_items, outs, n_rays   as rox_surface_footprints; of a slot's 10 rows p, d and
 *          dst are read (fail_surf is not).
 *   weight optional DEVICE: ray r of item i has weight weight[i*weight_stride + r]
 *          (rox_surface_thinfilm's rows with weight_stride = n_rows*ld_rows: row 0, T).  NULL:
 *          every weight is 1.  weight_stride >= n_rays.
 *   window optional HOST pair (hx, hy), both > 0: w_in and n_in are over the rays with
 *          |ax| <= hx and |ay| <= hy (at the image slot: a detector of 2hx x 2hy centred on the
 *          axis).  NULL: every counted ray.
 *   rec    host or device [n_items][n_seg] rox_seg_focus.
 * Which rays count.  A ray is looked at only if its status is ROX_OK: no row and no weight of any
 * other ray is read.  Of those, a ray whose weight is not finite or is negative (NaN included;
 * rox_surface_thinfilm documents a NaN case) adds to n_bad of every slot and to nothing else.
 * Arithmetic per remaining ray and slot, in operation order (IEEE double, no FMA: every step is
 * one NumPy float64 operation), from the slot's p = (x, y, z), d = (L, M, N) and dst:
 *          N == 0: the ray adds to n_flat and to nothing else.  Otherwise it is counted (n):
 *          mx = L/N, my = M/N; ax = x - z*mx, ay = y - z*my (where the line meets the plane z = 0
 *          of the slot's frame); z_out = z + dst*N; inside = no window or (|ax| <= hx and
 *          |ay| <= hy).  a = (ax, ay), b = (mx, my), w = the weight (0 is allowed and counted).
 * Reduction.  The partition: the rays of an item in tiles of 1024; thread t (0 .. 255) of tile T
 * holds rays 1024*T + 256*j + t, j = 0 .. 3; wave v of the tile is its threads 64*v .. 64*v + 63.
 *   A counted ray is a record of its own: W = w, the means its a and b, the moments 0, w_in = w
 *          if inside else 0.  A thread merges its counted rays in the order of j into an empty
 *          record (W = 0, w_in = 0, counts 0, ranges +inf / -inf).
 *   The merge of P with Q, P's rays first (Chan, Golub and LeVeque's pairwise update, weighted):
 *          Q.W == 0: P keeps its means and moments; P.W == 0: it takes Q's; otherwise
 *          W = P.W + Q.W, f = Q.W/W, g = P.W*f, da = Q.a - P.a, db = Q.b - P.b,
 *          mean <- P.mean + d*f, m_aa <- (P.m_aa + Q.m_aa) + (da.x*da.x + da.y*da.y)*g,
 *          m_ab <- (P.m_ab + Q.m_ab) + (da.x*db.x + da.y*db.y)*g, m_bb likewise.
 *          w_in <- P.w_in + Q.w_in; counts add; minima and maxima are exact selections.
 *   A wave: for o = 32, 16, 8, 4, 2, 1 every lane l merges its value (P) with that of lane l ^ o
 *          (Q); lane 0's value is the wave's partial record.
 *   An (item, slot): the partial records of waves 0 .. n_waves - 1 (n_waves = 4*ceil(n_rays/1024))
 *          are merged by a finishing kernel of 256 threads: thread t merges waves t, t + 256, ...
 *          in that order into an empty record, then for h = 128, 64, .., 1 thread t < h merges
 *          its value (P) with thread t + h's (Q); thread 0's value is the record.
 * No floating-point atomics: identical calls, host and device destinations, and one call over n
 * items against n calls over one item each give the same bits.
 * What the host derives.  The bundle's weighted mean-square radius about its centroid at the
 * plane z = zeta of the slot's frame is (m_aa + 2*zeta*m_ab + zeta^2*m_bb)/w_sum: smallest at
 * zeta* = -m_ab/m_bb, where it is (m_aa - m_ab^2/m_bb)/w_sum.  The focus lies in the segment when
 * zeta* lies between the z_in and the z_out range.  At the image slot zeta* is the distance of the
 * focus from the image plane and the value at zeta = 0 the mean-square size of the patch.
 * n_items in [1, ROX_MAX_FOCUS_ITEMS], n_rays in [1, 2^28], ld >= n_rays.  Argument errors return
 * ROX_E_ARG naming the parameter and item before anything is enqueued and leave the outputs
 * untouched.  Scratch per launch is 32 MiB or, where that is more, what one item needs (120 bytes
 * of partial records per wave of 256 rays and slot: 17 MB at 2^20 rays and 35 slots); larger jobs
 * run as consecutive launches over fewer items with the same results.  Asynchronous on `stream`
 * unless rec is host memory.                                                                  */
typedef struct rox_seg_focus {
    int64_t n;               /* rays counted                                                  */
    int64_t n_flat;          /* rays left out because N == 0                                  */
    int64_t n_bad;           /* rays left out for their weight (the same at every slot)       */
    int64_t n_in;            /* counted rays inside the window                                */
    double w_sum;            /* sum of w over the counted rays                                */
    double w_in;             /* ... over those inside the window                              */
    double a_mean[2];        /* weighted means of a and of b                                  */
    double b_mean[2];
    double m_aa;             /* sum w |a - a_mean|^2                                          */
    double m_ab;             /* sum w (a - a_mean).(b - b_mean)                               */
    double m_bb;             /* sum w |b - b_mean|^2                                          */
    double z_in_min, z_in_max;   /* range of z over the counted rays; empty: +inf / -inf      */
    double z_out_min, z_out_max; /* range of z_out                                            */
} rox_seg_focus;             /* 136 bytes; a_mean .. m_bb are NaN where n == 0 or w_sum == 0  */
int rox_segment_foci(rox_system *sys, uint32_t trace_flags, int32_t n_items, const rox_out *outs,
                     int64_t n_rays, const double *weight, int64_t weight_stride,
                     const double *window, rox_seg_focus *rec, void *stream);

/* Weighted maps: numpy.histogram2d(weights=) of where the rays of ROX_OUT_FULL packets reach one
 * slot, summed exactly.  The count maps of rox_surface_footprints take no weight; here every ray
 * carries one (rox_surface_thinfilm's row 0 times a spectral factor: an irradiance picture of a
 * ghost, several wavelengths into one map), and the sums are 64-bit fixed point at a power-of-two
 * scale per map, so that they do not depend on any order -- of rays, waves, workgroups or launches.
 *   trace_flags, n_items, outs, n_rays   as rox_segment_foci.
 *   slot   in [0, n_seg), or -1 for the last slot (the image).  Of that slot rows 0 and 1 (p.x,
 *          p.y) are read, of rays with status ROX_OK only: no row and no weight of any other ray.
 *   weight, weight_stride   as rox_segment_foci: optional DEVICE, NULL = every weight is 1.
 *   item_factor  optional HOST [n_items], finite and >= 0 (the item's spectral weight); NULL = 1.
 *   item_map     optional HOST [n_items], in [0, n_maps): the map item i adds into.  NULL: item i
 *          adds into map i and n_maps == n_items.  Several items may share a map.
 *   n_maps in [1, ROX_MAX_FOCUS_ITEMS]; nbx, nby in [1, 1024].
 *   window HOST [n_maps][4] = (cx, cy, hx, hy), finite, hx and hy > 0, cx - hx < cx + hx (and y).
 *          Map m is numpy.histogram2d(x, y, bins=(nbx, nby), range=[[cx - hx, cx + hx],
 *          [cy - hy, cy + hy]], weights=...), x the first axis: with lo = cx - hx, hi = cx + hx
 *          edge j is lo + j*((hi - lo)/nbx) (one quotient, one product, one sum) and the last
 *          edge hi -- numpy.linspace's bits; y likewise.  A value is placed by comparison with
 *          the edges: bins are half-open, the last one closed, values outside and NaN dropped.
 *          With cx = cy = 0 and hx = hy these are the edges of rox_surface_footprints' maps.
 *   wmaps  host or device [n_maps][nbx][nby] int64; counts host or device, the same shape in
 *          uint32 (optional); scale_exp host or device [n_maps] (required with wmaps); item host
 *          or device [n_items] (optional).  wmaps, counts and item may not all be NULL.
 * Arithmetic, in operation order (IEEE double, no FMA).  Per OK ray r of item i:
 *          v = weight[i*weight_stride + r] * item_factor[i] (one product; absent operands are 1).
 *          A ray whose weight is not finite or is negative (NaN included), or whose v is not
 *          finite, adds to n_bad and to nothing else.  Every other OK ray is usable.
 *   Pass 1: per map m, vmax = the largest v over the usable rays of its items (an exact
 *          selection) and N = n_rays * the number of its items.  frexp(vmax) = (f, E), vmax =
 *          f*2^E with f in [0.5, 1): scale_exp[m] = 61 - ceil(log2(N)) - E, clamped to
 *          [-1000, 1000]; 0 where the map has no usable ray or vmax == 0.  Every q below is then
 *          <= 2^(61 - ceil(log2 N)) and no sum over a map's rays reaches 2^62: nothing overflows.
 *   Pass 2: q = llrint(ldexp(v, scale_exp[m])) (the ldexp is exact where q != 0; round to
 *          nearest even).  A usable ray inside the window adds q to wmaps[m][bx][by], 1 to
 *          counts[m][bx][by], and to its item's n_in and q_in; outside (NaN position included) to
 *          n_out and q_out.
 * The map in the caller's units is ldexp((double)wmaps, -scale_exp[m]), left to the caller.  Per
 * ray the quantisation error is at most 2^-(scale_exp + 1): about vmax * N * 2^-61.
 * Integer addition is exact and associative: identical calls, host and device destinations, any
 * permutation of an item's rays and one call over n items into n maps against n calls over one
 * item each give the same bits, and sum(wmaps[m]) == the sum of q_in over map m's items.
 * Argument errors return ROX_E_ARG naming the parameter and item before anything is enqueued and
 * leave the outputs untouched.  Scratch per launch is 32 MiB or, where that is more, what one item
 * (pass 1: 8 bytes per wave of 256 rays) or one map bound for host memory needs; larger jobs run as
 * consecutive launches with the same results.  Asynchronous on `stream` unless an output is host
 * memory.  ROX_WMAPS_PATH=lds / global forces one of the kernel's two scatter paths (same bits). */
typedef struct rox_wmap_item {
    int64_t n_in;            /* usable rays inside the map's window (binned)                  */
    int64_t n_out;           /* usable rays outside it (NaN position included)                */
    int64_t n_bad;           /* OK rays left out for their weight                             */
    int64_t q_in;            /* sum of q over the binned rays                                 */
    int64_t q_out;           /* sum of q over the usable rays outside                         */
} rox_wmap_item;             /* 40 bytes */
int rox_weighted_maps(rox_system *sys, uint32_t trace_flags, int32_t n_items, const rox_out *outs,
                      int64_t n_rays, int32_t slot,
                      const double *weight, int64_t weight_stride,
                      const double *item_factor, const int32_t *item_map, int32_t n_maps,
                      const double *window, int32_t nbx, int32_t nby,
                      int64_t *wmaps, uint32_t *counts, int32_t *scale_exp,
                      rox_wmap_item *item, void *stream);

/* Wavefront differentials: tolerancing from one trace.  By Fermat's principle the first-order
 * change of a ray's optical path under a small displacement delta of the surface point it meets
 * is (n1*b4 - n2*d).delta, b4 and d the ray's unit directions before and after the interface and
 * n1, n2 the unsigned indices (Hopkins & Tiziani 1966; Rimmer 1970); under a change dn of a gap's
 * index it is dn*dst.  Per OK ray and selected slot of the ROX_OUT_FULL packets of finished
 * launches this entry forms eleven such columns -- shifts, rotations about the vertex, curvature,
 * power, two astigmatic irregularities, the gap's index -- and reduces them, with caller-supplied
 * per-ray aux rows (the nominal OPD, the pupil coordinates), to the sums a covariance needs:
 * sensitivity tables, compensators, RSS budgets and Monte Carlo runs are then host linear algebra
 * on n_cols numbers.  The columns are INCREASES of optical path.
 *   trace_flags, n_items, outs, n_rays   as rox_segment_foci; of a slot's 10 rows d is read and,
 *          where the slot is selected, p and dst.
 *   wvl_idx  HOST [n_items], as rox_surface_transmission: item i's row of the index table.
 *   sel_slot HOST [n_sel], strictly increasing slots in [0, n_seg), n_sel in [0, n_seg].  NULL:
 *          every slot, and n_sel == n_seg.
 *   aux    optional DEVICE: ray r of item i has aux row a at aux[i*aux_stride + a*ld_aux + r];
 *          n_aux in [0, ROX_MAX_WD_AUX], ld_aux >= n_rays.
 *   n_cols = n_aux + 11*n_sel, in [1, ROX_MAX_WD_COLS].
 *   cols   optional, host or device [n_items][n_cols][ld_cols], ld_cols >= n_rays: the columns of
 *          every ray, NaN (every column) for a ray that is not counted.
 *   item   host or device [n_items] rox_wd_item; pivot, sums host or device [n_items][n_cols];
 *          gram host or device [n_items][n_cols][n_cols], symmetric, both triangles written.
 *          cols, item and gram may not all be NULL; pivot and sums go with item, sums with pivot,
 *          gram with all three.
 * Which rays count.  A ray is looked at only if its status is ROX_OK: no row and no aux value of
 * any other ray is read.  An OK ray with an aux value or a column that is not finite adds to n_bad
 * and to nothing else.  Every other OK ray is counted.
 * Columns of an OK ray, in operation order (IEEE double, no FMA: every step is one NumPy float64
 * operation; dot and cross products as rox_surface_transmission defines them).  Columns
 * 0 .. n_aux - 1 are the aux values.  For the selected slot j, k = sel_slot[j], s = slot_ifc[k],
 * p = (x, y, z), d and dst of that slot and b4 the previous slot's d carried into this frame as
 * rox_surface_transmission carries it (rt.v of every interface in between, unfused, in the row's
 * rt_order), the columns n_aux + 11*j + c are
 *          n1 = |n_table[w][s-1]|, n2 = |n_table[w][s]|; at slot 0 b4 = d and n1 = n2 =
 *          |n_table[w][0]|; at the last slot (the image) n2 = 0.
 *          g = (n1*b4.x - n2*d.x, n1*b4.y - n2*d.y, n1*b4.z - n2*d.z): 0 at slot 0; n1*b4 at the
 *          image, where a shift of the slot is a shift of the reference sphere's centre.
 *   c = 0, 1, 2   g.x, g.y, g.z: a shift of the interface along its own axes.
 *   c = 3, 4, 5   cross(p, g): a rotation about the interface's vertex ((r x p).g = r.(p x g)).
 *   c = 6         g.z*(r2/(q*(1.0 + q))), r2 = x*x + y*y, q = sqrt(1.0 - ((ec*cv)*cv)*r2), cv and
 *                 ec of the interface's rox_surface: a change of vertex curvature (d sag / d cv of
 *                 the conic base) for the profiles ROX_SPHERICAL, ROX_CONIC, ROX_EVENPOLY and
 *                 ROX_RADIALPOLY.  For the toroids, ROX_THINLENS, or a radicand that is not > 0:
 *                 g.z*(r2/2.0).
 *   c = 7         g.z*r2: power (a test-plate fit).
 *   c = 8, 9      g.z*(x*x - y*y) and g.z*((x + x)*y): irregularity, astigmatic at 0 and 45 deg.
 *   c = 10        dst: the index of the gap after this interface; 0.0 at the image slot.
 * Reduction.  The pivot of an item is its counted ray of lowest index (an exact integer
 * selection), pivot[c] that ray's column c; sums[c] = sum (col_c - pivot_c) and gram[a][b] = sum
 * (col_a - pivot_a)*(col_b - pivot_b) over the counted rays, so that the host's cov = gram -
 * sums sums^T / n subtracts nothing large (rox_surface_footprints' pivot).  n == 0: pivot is NaN,
 * sums and gram are 0.  The Gram matrix is a rank-n update on the fp64 matrix cores, as
 * rox_focus_zernike's: an item's rays in chunks (their number ceil(n_rays/512), at most 256; a
 * function of n_rays alone), a chunk in tiles of 32 rays whose rows [col - pivot | 1] (zero for a
 * ray that is not counted) are multiplied into 16x16 tiles of the upper triangle with
 * v_mfma_f64_16x16x4_f64; the chunks' records are added in chunk order.  n, n_bad and the pivot
 * ray are integer sums and a minimum.  No floating-point atomics: identical calls, host and
 * device destinations, one call over n items against n calls over one item each, and a job split
 * for the scratch bound give the same bits.  The order of summation inside a tile is the
 * hardware's: sums and gram are not promised bit for bit against a host evaluation; cols, pivot
 * and item are.
 * n_items in [1, ROX_MAX_FOCUS_ITEMS], n_rays in [1, 2^28], ld >= n_rays.  Argument errors return
 * ROX_E_ARG naming the parameter and item before anything is enqueued and leave the outputs
 * untouched.  Scratch per launch is 32 MiB or, where that is more, what one item needs (the
 * columns of one chunk of rays where they do not go to the caller's device memory, up to 8 MiB of
 * chunk records of (n_cols + 1 rounded up to 16)^2 doubles, one running record, the outputs);
 * larger jobs run as consecutive launches over fewer items, ranges of rays and groups of chunks
 * with the same results.  Asynchronous on `stream` unless an output is host memory.          */
#define ROX_WD_SLOT_COLS 11
#define ROX_MAX_WD_AUX 32
#define ROX_MAX_WD_COLS 512
typedef struct rox_wd_item {
    int64_t n;               /* rays counted                                                  */
    int64_t n_bad;           /* OK rays left out for a value that is not finite               */
    int64_t pivot_ray;       /* the counted ray of lowest index; -1 where n == 0              */
} rox_wd_item;               /* 24 bytes */
int rox_wave_differentials(rox_system *sys, uint32_t trace_flags, int32_t n_items, const rox_out *outs,
                           int64_t n_rays, const int32_t *wvl_idx,
                           int32_t n_sel, const int32_t *sel_slot,
                           int32_t n_aux, const double *aux, int64_t aux_stride, int64_t ld_aux,
                           double *cols, int64_t ld_cols,
                           rox_wd_item *item, double *pivot, double *sums, double *gram, void *stream);

/* Image simulation: what a scene looks like through the lens.  rox_varying_blur convolves a
 * picture with a point spread function that changes across it -- given at the nodes of a
 * rectilinear grid and blended between them by hat functions, every SOURCE pixel spreading with
 * its own local PSF -- and rox_image_warp resamples a picture under a displacement field given on
 * such a grid (distortion).  Neither reads a system: the PSF stack is the caller's, for instance
 * rox_weighted_maps of the node fields' packets on the detector's pixel pitch.
 *   scene  host or device [C][H][W] float64; out likewise, written whole.  scene and out may not
 *          overlap.  1 <= C <= 16, 1 <= H, W <= 16384.
 *   psf    host or device [C][GY][GX][S][S], S odd in [1, 65], r = (S - 1)/2: tap [a][b] is the
 *          light displaced by (a - r) rows and (b - r) columns.
 *   node_y HOST [GY], node_x HOST [GX]: finite, strictly increasing pixel coordinates; they may
 *          lie outside the picture or between pixels.  1 <= GY*GX <= ROX_MAX_FOCUS_ITEMS.
 *   flags  ROX_BLUR_EDGE_ZERO or ROX_BLUR_EDGE_REPLICATE.
 * Arithmetic, in operation order (IEEE double, no FMA).  The hat weights wy[0 .. GY - 1] of source
 * row i: with GY == 1, or i < node_y[0], wy[0] = 1; with i >= node_y[GY-1], wy[GY-1] = 1;
 * otherwise, k such that node_y[k] <= i < node_y[k+1], t = (i - node_y[k]) / (node_y[k+1] -
 * node_y[k]), wy[k] = 1 - t and wy[k+1] = t; every other weight is 0.  wx[0 .. GX - 1] of source
 * column j likewise from node_x.  The weighted source of node n = (ky, kx) is
 *          sw_n(i, j) = scene[c][i][j] * (wy[ky] * wx[kx])
 * and an output starts at acc = 0 and takes, over the nodes in row-major order and inside a node
 * over the taps (a, b) in row-major order,
 *          acc = acc + sw_n(i - (a - r), j - (b - r)) * psf[c][n][a][b]
 * A source outside the picture is skipped with ROX_BLUR_EDGE_ZERO; with ROX_BLUR_EDGE_REPLICATE
 * its row and column are clamped into the picture (the weights are those of the clamped pixel).
 * Terms whose hat weight is exactly zero may be skipped: results compare equal with ==, where
 * +0 == -0.  Inputs are finite; anything else is unspecified.  With the zero edge and a stack
 * whose every node sums to g, the output holds g times the scene's light up to what leaves the
 * frame.  Identical calls, and host and device arrays, give the same bits.
 * rox_image_warp:
 *   in     host or device [C][H][W]; out likewise; they may not overlap.
 *   disp   HOST [GY][GX][2] = (dy, dx) in pixels at the nodes, finite.
 * With k, ty the cell and fraction t of OUTPUT row i as above (k = 0, ty = 0 before the first node
 * or with GY == 1; k = GY - 1, ty = 0 from the last node on; a row k + 1 that does not exist is
 * read as row k, its factor being 0), l, tx those of column j and D = disp[.][.][0]:
 *          dy = (1 - ty)*((1 - tx)*D[k][l] + tx*D[k][l+1]) + ty*((1 - tx)*D[k+1][l] + tx*D[k+1][l+1])
 * and dx likewise from disp[.][.][1].  y = i + dy, x = j + dx, y0 = floor(y), fy = y - y0 (x0 and
 * fx likewise) and, I = in[c] with a tap outside the picture read as 0,
 *          out = (1 - fy)*((1 - fx)*I[y0][x0] + fx*I[y0][x0+1]) + fy*((1 - fx)*I[y0+1][x0] + fx*I[y0+1][x0+1])
 * A zero displacement returns the input (its bits, but +0 for -0).
 * Argument errors return ROX_E_ARG naming the parameter before anything is enqueued and without
 * touching a device.  Host pictures and stacks are mirrored in device scratch of their size.
 * Asynchronous on `stream` unless scene / in, psf or out is host memory.                      */
#define ROX_BLUR_EDGE_ZERO 0u
#define ROX_BLUR_EDGE_REPLICATE 1u
int rox_varying_blur(int32_t C, int32_t H, int32_t W, const double *scene,
                     int32_t S, int32_t GY, int32_t GX, const double *psf,
                     const double *node_y, const double *node_x,
                     double *out, uint32_t flags, void *stream);
int rox_image_warp(int32_t C, int32_t H, int32_t W, const double *in,
                   int32_t GY, int32_t GX, const double *node_y, const double *node_x,
                   const double *disp, double *out, void *stream);

/* Huygens point spread functions on the detector's pixel grid, through focus.  Every OK ray is a
 * plane wavelet with its own amplitude, phase and direction of arrival; their complex sum is
 * taken at the pixels of a product grid, for every plane of every item, and squared.  The entry
 * reads no system: the rows are the caller's (analyses.huygens_psf builds them from one
 * ROX_OUT_LAST and one ROX_OUT_OPD launch).
 *   rows   DEVICE [n_items][4][ld] = phi, xi, eta, zeta: phi in cycles, (xi, eta, zeta) =
 *          n (L, M, N) / lambda of the ray at the image, in cycles per system unit.  Only the
 *          first n_rays rays count, and of those only the ones with status ROX_OK; the rows of a
 *          failed ray are never read, and it enters the sum as a zero.
 *   amp    DEVICE [n_items][ld], the wavelets' amplitudes a_r, or NULL (every a_r = 1, with the
 *          bits of an array of ones).
 *   status DEVICE [n_items][ld].
 *   planes HOST [n_items][n_planes][3] = (x0, y0, dz), finite: pixel (a, b) of plane k is the
 *          image point (x0 + a pitch_x, y0 + b pitch_y), displaced dz along the image z axis.
 *   psf    optional, DEVICE [n_items][n_planes][nx][ny]; field optional, DEVICE [...][nx][ny][2]
 *          = (re, im) of U; stats optional, host or device [n_items][n_planes].  Not all NULL.
 * Arithmetic (IEEE double; every product and sum below is one rounding, summed left to right, no
 * contraction into FMA):
 *          t_A = phi + zeta*dz + xi*x0 + eta*y0 + xi*(a*pitch_x)         t_B = eta*(b*pitch_y)
 * each reduced as rox_focus_gmtf reduces its arguments, r = t - rint(t) (exact), (s, c) =
 * sincospi(2 r), and
 *          A[k, a][r] = a_r (c_A + i s_A)      B[b][r] = c_B + i s_B
 *          U[k][a][b] = sum over r of A[k, a][r] B[b][r]      psf = re(U)^2 + im(U)^2
 * The sum over r runs on the fp64 matrix cores in ascending r; its rounding is that of a sum of
 * 2 n_rays products in some fixed order, the same for every element, plane and call.
 * rox_huygens_stats of a plane: n the OK rays; norm = (sum of a_r)^2, the peak of a perfect
 * wavefront; sum the sum of psf over the window; peak its maximum, at pixel (peak_ix, peak_iy)
 * (the first in row-major order); strehl = psf at the pixel nearest the plane's origin, (a, b) =
 * (rint(-x0/pitch_x), rint(-y0/pitch_y)) clamped into the window, over norm -- meaningful when
 * the caller puts the origin on a pixel.  With n == 0 every double is NaN and the pixel is
 * (-1, -1); psf and field are then zero.  Every reduction runs in a fixed order without floating
 * point atomics: identical calls give identical bits, host and device stats alike, however the
 * job is split.
 * n_items in [1, ROX_MAX_FOCUS_ITEMS], n_planes in [1, ROX_MAX_FOCUS_PLANES], nx and ny in
 * [1, 4096], ld in [1, 2^28], n_rays in [1, ld], pitch_x and pitch_y finite and > 0.  Argument
 * errors return ROX_E_ARG naming the parameter before anything is enqueued.  Scratch (the
 * operands and U) is bounded by 1 GiB per launch; larger jobs run as consecutive launches over
 * items, or over the planes of one item, with the same results.  The least a launch holds is one
 * plane: about 16 n_rays (nx' + ny') bytes, nx' and ny' the pixel counts rounded up to 64; a shape
 * whose single plane exceeds the bound is an argument error (n_rays).  Asynchronous on `stream` unless stats is host memory.                                */
typedef struct rox_huygens_stats {
    int64_t n;
    double norm, sum, peak, strehl;
    int32_t peak_ix, peak_iy;
} rox_huygens_stats;         /* 48 bytes */
int rox_huygens_psf(int32_t n_items, int32_t n_planes, int64_t n_rays,
                    const double *rows, int64_t ld, const double *amp, const uint8_t *status,
                    const double *planes, int32_t nx, int32_t ny, double pitch_x, double pitch_y,
                    double *psf, double *field, rox_huygens_stats *stats, void *stream);

/* chief-ray aiming ------------------------------------------------------- */
/* One problem per (field, wavelength): trace.iterate_ray
 * (rayoptics/raytr/trace.py:313-415) as trace.aim_chief_ray calls it
 * (trace.py:627-640, from OpticalSpecs.update_optical_properties,
 * opticalspec.py:263-281): find the aim point (x1, y1) on the paraxial entrance
 * pupil plane such that the ray from pt0 towards (x1, y1, z_enp) meets interface
 * `surf` at (x_target, y_target), every trial ray traced through the whole
 * system (raytrace.trace defaults).  Both branches of the reference run on the
 * device, one lane per problem, all problems in one launch:
 *   two_d = 0  field and target on the y axis (trace.py:376-392): x1 = 0 and y1 by
 *              the secant iteration of scipy.optimize.newton (x0 = 0, tol 1.48e-8,
 *              maxiter 50)
 *   two_d = 1  any other field (trace.py:394-410): scipy.optimize.fsolve from (0, 0)
 *              with epsfcn = 0.0001 * fod.enp_radius -- MINPACK's hybrd (Powell's
 *              hybrid method: forward-difference Jacobian, dog-leg steps, Broyden
 *              updates; xtol 1.49012e-8, maxfev 600, factor 100, internal scaling)
 * probs / aim_xy / result are host memory; synchronous. */
enum { ROX_AIM_CONVERGED = 0,   /* aim = root                                   */
       ROX_AIM_NOT_CONVERGED = 1,/* aim = the last iterate, as iterate_ray keeps it
                                    (results.root; fsolve's x with ier != 1)      */
       ROX_AIM_TRACE_ERROR = 2 };/* a trial ray failed before `surf`: aim = (0, 0) */
typedef struct rox_aim {
    double pt0[3];           /* osp.obj_coords(fld)[0]                         */
    double z_enp;            /* fod.obj_dist + fod.enp_dist                    */
    double y_target;         /* xy_target[1]                                   */
    double z_dir0;           /* seq_model.z_dir[0]                             */
    int32_t wvl_idx;
    int32_t surf;            /* ifcx (the stop surface)                        */
    int32_t flip;            /* not wide angle: dir0 = -dir0 if dir0.z*z_dir0 < 0 */
    int32_t two_d;           /* which branch of iterate_ray (see above)        */
    double x_target;         /* xy_target[0]                                   */
    double epsfcn;           /* two_d: 0.0001 * fod.enp_radius                 */
} rox_aim;                   /* 80 bytes */
/* aim_xy: [n][2] = (x1, y1) per problem */
int rox_aim_chief_rays(rox_system *sys, int32_t n, const rox_aim *probs,
                       double eps, double *aim_xy, int32_t *result, void *stream);

/* rayoptics/raytr/trace.py:866-961 iterate_ray_raw: the same two iterations over an explicit
 * path list -- `sys` is the table of THAT path, e.g. the reversed path along which
 * wideangle.eval_real_image_ht (wideangle.py:620-665; FieldSpec.obj_coords of fields given as
 * real image heights, opticalspec.py:1019-1030, 1059-1070) sends the chief ray back from the
 * image point.  The reference also hands back `rr`, the RayResult of the LAST TRIAL RAY it
 * evaluated (not a ray through the root): last_xy[n][2] = that trial's (x1, y1) on the pupil
 * plane, last_status[n] = its trace status (both NULL: exactly rox_aim_chief_rays).  All the
 * problems of a model -- every field -- are one launch. */
int rox_iterate_ray_raw(rox_system *sys, int32_t n, const rox_aim *probs, double eps,
                        double *aim_xy, int32_t *result, double *last_xy,
                        int32_t *last_status, void *stream);

/* rayoptics/raytr/wideangle.py:86-427 find_real_enp (vselector 'rev1') +
 * find_z_enp_on_interval: the z of the real entrance pupil of a wide-angle
 * field, measured from the first interface -- what trace.aim_chief_ray
 * (trace.py:634-635) stores as fld.aim_info of a wide-angle model.  One lane
 * per (field, wavelength) runs the reference's whole search: the sampled walk
 * from the paraxial pupil, find_edge's bisections, scipy.optimize.newton's
 * secant iteration (tol 1.48e-8, rtol 1e-7) and the brentq fall-back (xtol
 * 2e-12, rtol 1e-7, 100 iterations), every trial ray traced by
 * enp_z_coordinate (wideangle.py:46-83; intersect_obj = False). */
enum { ROX_ENP_FOUND = 0,        /* z_enp as find_real_enp returns it               */
       ROX_ENP_NO_CHIEF_RAY = 1, /* "chief ray trace failed": no ray reaches the stop
                                    centre; z_enp = the last good sample (:283-291) */
       ROX_ENP_REFERENCE_RAISES = 3 }; /* the reference itself raises here (no sample
                                    got through: unpacking None; brentq without a sign
                                    change; a failed last ray indexed at the stop)  */
typedef struct rox_enp {
    double dir0[3];          /* osp.obj_coords(fld)[1]                          */
    double rot[9];           /* rot_v1_into_v2([0,0,1], dir0), row-major         */
    double obj_dist;         /* fod.obj_dist                                    */
    double z_enp_0;          /* fod.enp_dist (the paraxial entrance pupil)      */
    double aim_info;         /* fld.aim_info, NaN if None                       */
    int32_t wvl_idx;
    int32_t surf;            /* stop_idx (1 when the model has no stop surface) */
    int32_t rot_order;       /* ROX_RT_* of rot (np.matmul -> dgemv)            */
    int32_t check_direction; /* find_real_enp_rev1's keyword (True)             */
} rox_enp;                   /* 136 bytes */
/* z_out: [n][2] = (z_enp, z of the last trial ray traced: the `rr` the
 * reference returns beside z_enp is that ray) */
int rox_find_real_enp(rox_system *sys, int32_t n, const rox_enp *probs,
                      double eps, double *z_out, int32_t *result, void *stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* ROXTRACE_H */
