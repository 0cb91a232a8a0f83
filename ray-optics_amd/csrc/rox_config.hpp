// rox_config.hpp -- what decides which trace kernels exist and how they are compiled: the build
// knobs, the workgroup size and register budget of every (output mode, feature instance), the
// feature bits and the lists of compiled instances.  No device code; host and device units alike
// include it.
#pragma once

#include "../../include/roxtrace.h"

#pragma clang fp contract(off)

// ---- build-time knobs (defaults = the shipped configuration; the others are
// kept for A/B measurement with tools/ab_bench.py) -------------
#ifndef ROX_MIN_WAVES        // __launch_bounds__ second argument (waves per SIMD)
#define ROX_MIN_WAVES 4       // 128 VGPRs
#endif
#ifndef ROX_SLIM_FP64        // 1: range-guarded slim sqrt / shared-reciprocal division triples
#define ROX_SLIM_FP64 1       //    (bit-identical to sqrt() and `/`; rox_math.hpp slim_*)
#endif
#ifndef ROX_IDENT_RT         // 1: interfaces whose rotation is exactly the identity skip the dgemv chains
#define ROX_IDENT_RT 1        //    (HITS 117.0 -> 111.2 us; FULL keeps the chains: 190.8 vs 194.5 us)
#endif
#ifndef ROX_BLOCK            // workgroup size of the reduced-output modes (HITS sustained: 512 -> 124 us,
#define ROX_BLOCK 512         // 1024 -> 131 us)
#endif
#ifndef ROX_BLOCK_POLY       // ... of the instances that carry Newton code
#define ROX_BLOCK_POLY ROX_BLOCK
#endif
#ifndef ROX_MIN_WAVES_POLY   // waves per SIMD the reduced-output modes of those instances are compiled for
#define ROX_MIN_WAVES_POLY ROX_MIN_WAVES
#endif
#ifndef ROX_KERNEL_ALIGN     // alignment of the trace kernels' code (0: the compiler's 256 bytes)
#define ROX_KERNEL_ALIGN 0
#endif
#if ROX_KERNEL_ALIGN > 0
#define ROX_KERNEL_ALIGNED __attribute__((aligned(ROX_KERNEL_ALIGN)))
#else
#define ROX_KERNEL_ALIGNED
#endif
#ifndef ROX_MIN_WAVES_APLIST_REDUCED  // waves per SIMD the HITS kernels of the aperture-list instance
#define ROX_MIN_WAVES_APLIST_REDUCED 8 // (spherical tables with clear-aperture lists: every Zemax import without
#endif                                 // aspheres -- BASELINE configs[3], configs[4]) are compiled for.  At the
                                       // default 4 hipcc takes 79 VGPRs; held to 64 (56 B of scratch per lane) or 72
                                       // the same source is 8 % faster: lithography lens HITS 421 -> 386 us per 2^20
                                       // rays, RC telescope 46.6 -> 42.9 (7: 389 / 42.9); the lean instance gains
                                       // nothing from it (111.0 -> 113.6) and FULL loses 7-12 %.  profiles/r05_min_waves.txt
#ifndef ROX_MIN_WAVES_FAST   // waves per SIMD the tolerance-mode (F_FAST) instances are compiled for
#define ROX_MIN_WAVES_FAST ROX_MIN_WAVES
#endif
#ifndef ROX_BLOCK_SMALL      // workgroup size of launches that do not fill the chip (block_of() below)
#define ROX_BLOCK_SMALL 256
#endif
#ifndef ROX_BLOCK_COMPACT    // workgroup = tile size of HITS_COMPACT: fewer, larger tiles make the
#define ROX_BLOCK_COMPACT 1024 // look-back cheaper (into pinned memory 128 -> 501, 256 -> 371,
#endif                        // 512 -> 337, 1024 -> 316 us)
#ifndef ROX_MIN_WAVES_COMPACT_LEAN   // waves per SIMD the lean / aplist HITS_COMPACT instances are compiled for
#define ROX_MIN_WAVES_COMPACT_LEAN ROX_MIN_WAVES
#endif
#ifndef ROX_BLOCK_FULL       // workgroup size of FULL mode: with the per-surface barrier the whole
#define ROX_BLOCK_FULL 1024   // workgroup writes its packet rows together (sustained 256 -> 215 us,
#endif                        // 512 -> 198 us, 1024 -> 192.5 us; without the barrier 217 us)
#ifndef ROX_FULL_EARLY_STORES    // 1: FULL packets: a segment's point and normal are stored as soon as they
#define ROX_FULL_EARLY_STORES 1  //    are known (after the intersection / the normalisation) instead of with the
#endif                           //    direction at the end of the iteration: the workgroup's ten row pieces per
                                 //    surface leave in three bursts instead of one -- the store-bound double Gauss
                                 //    192.0 -> 188.2 us per 2^20 rays (5.24 -> 5.34 TB/s), .zmx zoom and phone lens
                                 //    unchanged, lithography lens 669 -> 666 (gpurun_out ab_full, two rounds)
#ifndef ROX_WG_SYNC          // 1: FULL mode: a workgroup barrier per surface keeps the waves of a
#define ROX_WG_SYNC 1         //    workgroup on the same packet rows (218 -> 202 us)
#endif
// FULL mode of the instances that carry Newton code (aspheres, toroids): the iteration counts
// differ per wave, so a 1024-thread workgroup (the only one its CU holds at 99-125 VGPRs) waits
// at every surface for its slowest wave with nothing else to run; four 256-thread workgroups
// per CU, out of step with each other, avoid that (round 3, when these instances always ran
// 256: phone lens 319 -> 290 us).  Since round 5 the choice is made per SYSTEM at launch
// (launch.hip want_small(): by the share of Newton interfaces): the large workgroup is the
// regular one here too and the ROX_BLOCK_SMALL kernels are the alternative.
#ifndef ROX_BLOCK_FULL_POLY
#define ROX_BLOCK_FULL_POLY 1024
#endif
#ifndef ROX_WG_SYNC_POLY     // barrier per surface also there (off: 286 / 483 / 195 -- within the noise)
#define ROX_WG_SYNC_POLY 1
#endif
#ifndef ROX_MIN_WAVES_FULL_POLY  // 5 caps the VGPRs at 96 (five workgroups per CU) at the price of 12-28 B
#define ROX_MIN_WAVES_FULL_POLY ROX_MIN_WAVES  // of scratch per lane: phone lens 273, but the .zmx zoom 386 us
#endif
#ifndef ROX_IDENT_RT_FULL_POLY   // 1: the identity-rotation short cut also in the FULL mode of those
#define ROX_IDENT_RT_FULL_POLY 1 //    instances, which are closer to their VALU bound (283 / 473 / 187 us)
#endif

namespace rox {

constexpr int kBlock = ROX_BLOCK;
constexpr int kWaves = kBlock / 64;
// threads per workgroup (= rays per tile) of an output mode of a feature instance
// (feat & kFeatNewton: the instance carries Newton code -- F_EVEN | F_RADIAL | F_TOROID)
constexpr int kFeatNewton = 1 | 2 | 4;
constexpr int kFeatFast = 64;       // F_FAST: a tolerance-mode instance (ROX_FAST_FP64; reduced-output modes only)
// `small`: the launch does not fill the chip several times over (launch.hip want_small()): it
// runs in workgroups of ROX_BLOCK_SMALL threads, which spread over the CUs wave by wave instead
// of sixteen (FULL) or eight waves at a time.  A CU holds 5 waves per SIMD of the lean FULL
// instance (84 VGPRs) but only ONE 1024-thread workgroup (4 per SIMD); BASELINE configs[3]
// (5 x 256^2 rays = 5120 waves) is 320 such workgroups on 256 CUs -- two rounds -- and 1280
// workgroups of 256 threads on 1280 slots: one.
constexpr int block_of(int out_mode, int feat, bool small = false)
{
    return out_mode == ROX_OUT_HITS_COMPACT ? ROX_BLOCK_COMPACT
         : small ? ROX_BLOCK_SMALL
         : out_mode == ROX_OUT_FULL ? ((feat & kFeatNewton) ? ROX_BLOCK_FULL_POLY : ROX_BLOCK_FULL)
         : ((feat & kFeatNewton) ? ROX_BLOCK_POLY : ROX_BLOCK);
}
// whether a distinct small-workgroup kernel exists for (mode, instance)
constexpr bool has_small(int out_mode, int feat)
{
    return block_of(out_mode, feat, true) != block_of(out_mode, feat, false);
}
constexpr int min_waves_of(int out_mode, int feat, bool small = false)
{
    // (the small-workgroup kernels serve launches that fit the chip once: latency, where the
    // scratch of the tighter budget costs -- configs[3] HITS 18 -> 20 us -- instead of paying)
    return ((feat & kFeatFast) && out_mode != ROX_OUT_FULL) ? ROX_MIN_WAVES_FAST
         : (feat == 8 /* F_APLIST */ && out_mode == ROX_OUT_HITS && !small) ? ROX_MIN_WAVES_APLIST_REDUCED
         : (out_mode == ROX_OUT_FULL && (feat & kFeatNewton)) ? ROX_MIN_WAVES_FULL_POLY
         : (out_mode == ROX_OUT_HITS_COMPACT && !(feat & ~8)) ? ROX_MIN_WAVES_COMPACT_LEAN
         : (out_mode != ROX_OUT_FULL && out_mode != ROX_OUT_HITS_COMPACT && (feat & kFeatNewton))
               ? ROX_MIN_WAVES_POLY
         : ROX_MIN_WAVES;
}

enum { GEN_RAYS = 0, GEN_PUPIL = 1 };
enum { AXIS_LIST = 0, AXIS_PRODUCT = 1 };
// internal output mode of the aiming kernel: no packet stores, the intercept
// at TraceArgs.probe_surf is kept
constexpr int MODE_PROBE = 100;
// internal output mode of the through-focus kernel (rox_trace_through_focus): the ray is traced
// as for ROX_OUT_FAN, then evaluated at every focus plane of FocusArgs (focus_planes() below)
constexpr int MODE_FOCUS = 101;

// system features a launch needs; the host picks the leanest instance
enum { F_EVEN = 1,      // some interface is an EvenPolynomial (Newton code)
       F_RADIAL = 2,    // ... a RadialPolynomial
       F_TOROID = 4,    // ... a Y/XToroid
       F_APLIST = 8,    // some interface carries clear_apertures
       F_PHFILT = 16,   // filter_out_phantoms with phantoms present
       F_PHASE = 32 };  // phase elements / thin lenses
constexpr int F_POLY = F_EVEN | F_RADIAL | F_TOROID;
constexpr int F_ALL = F_POLY | F_APLIST | F_PHFILT | F_PHASE;
// instance flavours beside the feature bits: F_FAST = 64 (tolerance mode, below),
// F_GTAB = 128: the table stays in global memory and is read with scalar
// loads (rox_math.hpp ctblp) -- the instance of tables beyond the LDS (and, ROX_FAST_GTAB, of the
// tolerance-mode kernels)
constexpr int F_GTAB = 128;
// Which kernels read their table that way (beside the instance for tables beyond the LDS):
// ROX_GTAB_EXACT / ROX_GTAB_FAST, bit masks over {1: the reduced-output modes of the instances
// that carry Newton code, 2: ... of the other instances, 4: FULL packets of the Newton
// instances, 8: FULL of the others}.  A value read by a scalar load sits in SGPRs: the Newton
// instances, whose asphere coefficients and row constants otherwise occupy vector registers
// for the whole evaluation, drop from 91-101 to 72-80 VGPRs -- one or two more resident waves
// per SIMD.  Measured per 2^20 rays (gpurun r06t): .zmx zoom HITS 134 -> 124 us, tolerance mode
// 87 -> 76; Nikkor 291 -> 276, 154 -> 143; phone lens 227 -> 226, 151 -> 142; FULL packets gain
// nothing (bound by their stores; phone lens 267 -> 277): shipped for the reduced-output modes
// of the Newton instances, exact and tolerance mode.  Bit-identical either way.
#ifndef ROX_GTAB_EXACT
#define ROX_GTAB_EXACT 1
#endif
#ifndef ROX_GTAB_FAST
#define ROX_GTAB_FAST 1
#endif
// F_GTAB or 0 for (feature set, tolerance mode, output mode): the kernel the host launches
constexpr int gtab_of(int feat, bool fast, int out_mode)
{
    const int mask = fast ? ROX_GTAB_FAST : ROX_GTAB_EXACT;
    const bool newton = (feat & (1 | 2 | 4)) != 0;
    const int bit = (out_mode == ROX_OUT_FULL ? 4 : 1) << (newton ? 0 : 1);
    return ((feat & F_GTAB) || (mask & bit)) ? F_GTAB : 0;
}

// F_FAST: a tolerance-mode instance (ROX_FAST_FP64; its arithmetic is rox_math_fast.hpp)
constexpr int F_FAST = 64;
#ifndef ROX_FAST_NR          // Newton-Raphson steps after v_rcp_f64 / v_rsq_f64: 2 = ~1 ulp,
#define ROX_FAST_NR 2         // 1 = ~2^-45 relative (measured difference: see EXPERIMENTS.md)
#endif

// The feature instances that are compiled, X(name, FEAT) in kInstances order: one translation
// unit each, csrc/inst_<name>.hip (trace_<name>), and a tolerance-mode twin csrc/fast_<name>.hip
// (trace_<name>_fast: FEAT | F_FAST).  The host launches the first one that covers the need.
// (F_EVEN | F_APLIST: what a Zemax import with an EVENASPH surface needs -- every .zmx interface
// carries a clear-aperture list.  BASELINE configs[2]'s file ran on the general instance until
// round 5: 392 wave-VALU per wave-surface against 300 lean, profiles/r05_valu_account.json.)
// Besides these, csrc/gtab_general.hip: the general instance over a table left in global memory
// (trace_general_gtab).
#define ROX_TRACE_INSTANCES(X)                                                                 \
    X(lean, 0) X(even, F_EVEN) X(radial, F_RADIAL) X(poly, F_POLY) X(aplist, F_APLIST)        \
    X(evenap, F_EVEN | F_APLIST) X(general, F_ALL)
#define ROX_INSTANCE_FEAT(name, FEAT) FEAT,
constexpr int kInstances[] = {ROX_TRACE_INSTANCES(ROX_INSTANCE_FEAT)};

// the feature instances the search kernels are compiled for, X(name, FEAT) in kSearchInstances
// order; the host launches the first one that covers the system's features.  Besides these,
// csrc/search_general_gtab.hip: the general instance over a table in global memory.
#define ROX_SEARCH_INSTANCES(X)                                                                \
    X(lean, 0) X(even, F_EVEN) X(radial, F_RADIAL) X(aplist, F_APLIST) X(evenap, F_EVEN | F_APLIST) \
    X(general, F_ALL)
constexpr int kSearchInstances[] = {ROX_SEARCH_INSTANCES(ROX_INSTANCE_FEAT)};
#undef ROX_INSTANCE_FEAT

}  // namespace rox
