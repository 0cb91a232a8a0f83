#!/usr/bin/env python3
"""The wavefront-differentials pass (rox_wave_differentials, the reduction behind
analyses.tolerance_sensitivity) on the FULL packets of 9 (field, wavelength) items of the double
Gauss (13 slots, 146 columns with 3 aux rows) and of the `.zmx` zoom, at num_rays in `--rays`,
outputs in HBM.

Timed (each figure the median over `--trials` windows of `--reps` back-to-back calls between HIP
events after a warm-up call, with the windows' smallest and largest beside it): the call without
`cols` (the columns pass through the scratch a range of chunks at a time), with `cols` kept in HBM
(one range), and that call without the gram output (sums still need the Gram pass); in the same run on the
same packets rox_segment_foci, which reads the same 7 rows per slot -- the yardstick for the walk,
with the ratio and the bytes per second of the packet rows the walk must read over the whole call that keeps `cols` (7 rows of 8 B per
OK ray and slot, 1 B of status per ray).  `gram_TFLOPS_of_call` is n_ok * CP^2 flops (the upper
triangle of CP = n_cols + 1 rounded up to 16, two flops per multiply-add) over the time of the
WHOLE lean call, walk included, and counts no panel that is read for more than one pair: a floor
on the Gram kernel's own rate, given against the vector fp64 peak.  At the first size of `--rays`
also what a perturbed copy costs today, timed on the nominal table: a new engine
(rox_system_create) plus one OUT_LAST launch of the 9 items -- an OPD launch needs reference-sphere
constants the workload files do not carry and costs no less -- times two signs of the default
tolerance set.  Not timed here: the whole analyses.tolerance_sensitivity call and the host's Monte
Carlo (examples/tolerancing.py prints both).  One JSON object per case.

    python tools/tolerance_bench.py [--rays 64 256 1024] [--reps 10] [--trials 7] [--json out.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_ITEMS = 9
VECTOR_FP64_TFLOPS = 78.6        # MI355X vector fp64 peak


def window_us(torch, fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def timed(torch, fn, reps, trials):
    """median and (min, max) of `trials` windows of `reps` calls, after a warm-up call"""
    fn()
    torch.cuda.synchronize()
    w = [window_us(torch, fn, reps) for _ in range(trials)]
    return float(np.median(w)), [float(min(w)), float(max(w))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rays', nargs='+', type=int, default=[64, 256, 1024])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--trials', type=int, default=7)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    import torch
    import rayoptics_amd  # noqa: F401
    from rayoptics_amd import abi, tolerance, workloads
    from rayoptics_amd.engine import TraceEngine, make_grid, make_opts

    flags = abi.INTERSECT_OBJ | abi.CHECK_APERTURES | abi.APPLY_VIGNETTING
    out = []
    for name in ('dblgauss_c2', 'zmx_evenasph_c3'):
        wl = workloads.load(name)
        eng = TraceEngine(wl.table)
        F, W = len(wl.fields), len(wl.table.wvls)
        flds = [wl.fields[i % F] for i in range(N_ITEMS)]
        wis = [(i // F) % W for i in range(N_ITEMS)]
        n_seg = eng.num_segments(flags)
        for num in args.rays:
            R = num * num
            opts = [make_opts(flags=flags, out_mode=abi.OUT_FULL) for _ in flds]
            res = eng.trace_pupil_grids(flds, wis, make_grid((-1., -1.), (1., 1.), num), opts, want_pupil=False)
            aux = torch.randn((N_ITEMS, 3, R), dtype=torch.float64, device=eng.device)
            item = eng.wave_differentials(res, flags, wis, aux=aux)[0]
            n_ok = int(item['n'].sum())
            n_cols = 3 + 11 * n_seg
            CP = (n_cols + 1 + 15) // 16 * 16
            r = dict(workload=name, num_rays=num, n_items=N_ITEMS, n_seg=n_seg, n_cols=n_cols, n_ok=n_ok)
            t_g = timed(torch, lambda: eng.wave_differentials(res, flags, wis, aux=aux, on_device=True),
                        args.reps, args.trials)
            t_c = timed(torch, lambda: eng.wave_differentials(res, flags, wis, aux=aux, on_device=True,
                                                              want_cols=True), args.reps, args.trials)
            t_w = timed(torch, lambda: eng.wave_differentials(res, flags, wis, aux=aux, on_device=True,
                                                              want_cols=True, want_gram=False),
                        args.reps, args.trials)
            t_f = timed(torch, lambda: eng.segment_foci(res, flags, on_device=True), args.reps, args.trials)
            r['wave_differentials_us'], r['wave_differentials_us_range'] = t_g
            r['wave_differentials_cols_us'], r['wave_differentials_cols_us_range'] = t_c
            r['cols_without_gram_output_us'], r['cols_without_gram_output_us_range'] = t_w
            r['segment_foci_us'], r['segment_foci_us_range'] = t_f
            r['ratio_to_segment_foci'] = t_g[0] / t_f[0]
            read = 56.0 * n_ok * n_seg + R * N_ITEMS
            r['packet_bytes'] = read
            r['call_read_TBps'] = read / (t_c[0] * 1e-6) / 1e12
            r['segment_foci_read_TBps'] = read / (t_f[0] * 1e-6) / 1e12
            flops = float(n_ok) * CP * CP                   # 2 flops per multiply-add, half the matrix
            r['gram_flops'] = flops
            r['gram_TFLOPS_of_call'] = flops / (t_g[0] * 1e-6) / 1e12
            r['gram_fraction_of_vector_fp64_peak'] = r['gram_TFLOPS_of_call'] / VECTOR_FP64_TFLOPS
            # the route of today: a system and a launch per perturbed table (here the nominal one, OUT_LAST)
            if num == args.rays[0]:
                pert = tolerance.Perturbations(wl.table, None, 3, wis, flags)
                Q = len(tolerance.default_tolerances(pert))
                t0 = time.perf_counter()
                for _ in range(5):
                    e2 = TraceEngine(wl.table)
                    e2.trace_pupil_grids(flds, wis, make_grid((-1., -1.), (1., 1.), num),
                                         [make_opts(flags=flags, out_mode=abi.OUT_LAST) for _ in flds],
                                         want_pupil=False)
                    torch.cuda.synchronize()
                    e2.close()
                per = (time.perf_counter() - t0) / 5
                r['default_tolerances'] = Q
                r['per_perturbed_copy_ms'] = per * 1e3
                r['retrace_route_ms'] = 2 * Q * per * 1e3    # + and - of every tolerance
            print(json.dumps(r), flush=True)
            out.append(r)
        eng.close()
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
