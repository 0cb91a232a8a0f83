// rox_device.hpp -- device code of the sequential real-ray trace for gfx950
// (MI355X, CDNA4): arithmetic, surface intersection, phase elements, packet
// stores and the trace kernel template.  Included by every kernel-instance
// translation unit (inst_*.hip, fast_*.hip, gtab_general.hip; search_*.hip through rox_search.hpp).
//
// Hot path of mjhoptics/ray-optics restated as hand-written HIP (reference
// paths relative to its src/):
//   rayoptics/raytr/raytrace.py:83-264   trace_raw   -> trace_ray() (the loop)
//   rayoptics/raytr/raytrace.py:19-38    bend/reflect -> refract(), mirror()
//   rayoptics/raytr/raytrace.py:41-48, 205-210 phase  -> apply_phase()
//   rayoptics/oprops/doe.py:124-175      DiffractionGrating.phase_ludwig
//   rayoptics/oprops/doe.py:28-54, 272-323 DiffractiveElement.phase + radial_phase_fct
//   rayoptics/oprops/doe.py:375-397      HolographicElement.phase (every ThinLens)
//   rayoptics/oprops/thinlens.py:128-136 ThinLens.normal/intersect
//   rayoptics/elem/profiles.py:310-336   Spherical.intersect  \  quadric_hit()
//   rayoptics/elem/profiles.py:569-593   Conic.intersect      /
//   rayoptics/elem/profiles.py:155-186   intersect_spencer    -> newton_hit()
//   rayoptics/elem/profiles.py:849-885   EvenPolynomial.sag/df \ poly_eval()
//   rayoptics/elem/profiles.py:1070-1113 RadialPolynomial.sag/df/
//   rayoptics/elem/profiles.py:1317-1437 Y/XToroid            /
//   rayoptics/elem/surface.py:198-208, 416-457 point_inside    -> inside_aperture_list()
//   rayoptics/raytr/opticalspec.py:289-400, 1339-1353; trace.py:298-308
//                                         pupil -> (pt0, dir0) -> ray_start()
//
// Execution model: one wavefront lane = one ray; 512-thread workgroups take
// tiles of 512 consecutive rays.  Every per-surface parameter is wave-uniform:
// the surface table is staged once per workgroup in LDS and read with
// same-address (broadcast, conflict-free) ds_reads.  Ray packets are SoA
// [segment][component][ray]: each store is 64 lanes x 8 B = 512 B contiguous.
// All arithmetic is IEEE binary64 with the reference's operation order: this
// code is compiled with -ffp-contract=off, NumPy's BLAS dot sites are spelled
// as explicit fma chains (dot3), division and sqrt are the correctly rounded
// ones.  No MFMA: this is 3-vector arithmetic, not a contraction.
//
// This file only includes the pieces, in dependency order.  The host units (launch.hip and the
// entry units, through rox_system.hpp) include rox_args.hpp and no kernel code; the analysis
// units include the pieces they use.
#pragma once
#include "rox_config.hpp"         // build knobs, workgroup sizes, feature bits, instance lists
#include "rox_args.hpp"           // device row, kernel arguments, launch configuration, tile geometry
#include "rox_math.hpp"           // v3, dot3 / rotate, slim fp64, unit / refract / mirror
#include "rox_math_fast.hpp"      // tolerance-mode arithmetic
#include "rox_profiles.hpp"       // quadric_hit, poly_eval, newton_hit, aperture lists
#include "rox_phase.hpp"          // apply_phase
#include "rox_opd.hpp"            // wave_abr_*
#include "rox_ray.hpp"            // SegOut, CtxT, trace_ray / _reduced / _fast, ray_start
#include "rox_compact.hpp"        // look_back, finish_tile
#include "rox_kernel.hpp"         // trace_tiles, the kernels, launch_instance*, ROX_TRACE_INSTANCE
