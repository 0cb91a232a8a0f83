/* roxtrace_diag.h -- measurement and self-test helpers of libroxtrace.so.
 *
 * NOT part of the drop-in boundary (include/roxtrace.h): nothing in the
 * reference corresponds to these.  bench.py, tools/ and tests/ call them.
 */
#ifndef ROXTRACE_DIAG_H
#define ROXTRACE_DIAG_H

#include "roxtrace.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

/* runs `launches` back-to-back launches of the pupil-grid kernel on `stream`,
 * bracketed by HIP events recorded on that same stream, and returns the mean
 * kernel duration in milliseconds (bench.py's roofline figures). */
int rox_time_pupil_grid(rox_system *sys, const rox_field *fld,
                        const rox_grid *grid, int32_t wvl_idx,
                        const rox_opts *opts, const rox_out *out,
                        void *stream, int32_t launches, double *mean_ms);

/* compares the kernels' exponent-band-guarded sqrt / division paths with the
 * plain IEEE operators on n pseudo-random operand sets (whole exponent range,
 * zeros, denormals, inf, nan, and wave-uniform band-edge classes).
 * counts[0] = sqrt mismatches, counts[1] = division mismatches (both must be
 * 0), counts[2] = operand sets that took a guarded path, counts[3] = operand
 * sets of the band-edge classes that took a guarded path. */
int rox_selftest_fp64(uint64_t n, uint64_t seed, uint64_t counts[4]);

/* how many ROX_OUT_HITS_COMPACT launches this process has issued in each form:
 * counts[0] = fused (compaction inside the trace kernel), counts[1] = two-pass (plain HITS
 * launch + pack kernel; deep tables / Newton instances writing device memory, or
 * ROX_PACK_TWO_PASS=1).  Tests use it to see which form a call took. */
int rox_diag_pack_launches(uint64_t counts[2]);

/* how many trace-kernel launches this process has issued in each form (a batched launch
 * counts once): counts[(inst * 2 + fast) * 2 + small], the first n of 32 counters.
 * inst = 0..6, the compiled feature instances in the order the host tries them (lean, even,
 * radial, poly, aplist, evenap, general), 7 = the general instance over a table in global
 * memory; fast = the tolerance-mode twin; small = the small-workgroup kernels were asked for
 * (ROX_OUT_HITS_COMPACT has no such kernel: its fused launches count under the launch rule's
 * answer all the same).  Entries past the 32nd are set to 0.  Tests use it to see which kernel
 * a call took. */
int rox_diag_trace_launches(uint64_t *counts, int32_t n);

/* the workgroup -> tile map of a ROX_OUT_FULL launch, walked as the kernel walks it: `grid`
 * workgroups stride over n_tiles tiles, tiles[t] = the tile that walk index t (workgroup
 * t % grid on its pass t / grid) traces with `group` tiles per XCD run (0 = identity; the
 * library's own choice, or ROX_FULL_TILE_GROUP, is not consulted).  wg0 = linear id of the
 * launch item's first workgroup (blockIdx.y * gridDim.x of a batched launch).  No device needed. */
int rox_diag_full_tile_map(int64_t n_tiles, int32_t group, int64_t grid, int32_t wg0,
                           int64_t *tiles);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* ROXTRACE_DIAG_H */
