#!/usr/bin/env python3
"""One through-focus launch (rox_trace_through_focus, K planes) against K separate ROX_OUT_FAN
launches of the same pupil grid, timed with HIP events around `--reps` back-to-back calls after a
warm-up (the median of `--trials` such runs is reported).

    python tools/through_focus_bench.py [--K 21] [--reps 20] [--trials 5] [--json out.json]

Cases: BASELINE configs[1] (double Gauss, 1024^2 grid) and configs[2] (the .zmx even-asphere
zoom, one field, one wavelength, 512^2 grid).  The planes carry the golden double Gauss fixture's
reference sphere (finite) at K focus shifts: the kernel's per-plane work does not depend on the
values.  Reports the fused launch with statistics only and with rows as well, the K FAN
launches, their ratio and the added time per plane."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def timed(torch, fn, reps, trials):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(trials):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)      # us per call
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--K', type=int, nargs='+', default=[21])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--trials', type=int, default=5)
    ap.add_argument('--json')
    args = ap.parse_args()
    import torch
    import rayoptics_amd  # noqa: F401
    from rayoptics_amd import abi, workloads
    from rayoptics_amd.engine import TraceEngine, make_grid, make_opts
    from rayoptics_amd.table import wavefront_from_array
    import helpers as H
    wf = wavefront_from_array(H.fixture('dblgauss')['opd_f0']['wavefront'])
    flags = abi.INTERSECT_OBJ | abi.CHECK_APERTURES | abi.APPLY_VIGNETTING
    results = []
    for name, num in (('dblgauss_c2', 1024), ('zmx_evenasph_c3', 512)):
        wl = workloads.load(name)
        N = wl.table.n_ifcs
        eng = TraceEngine(wl.table)
        fld = wl.fields[-1]
        wi = wl.ref_wvl_idx
        grid = make_grid((-1., -1.), (1., 1.), num)
        for K in args.K:
            planes = []
            for foc in np.linspace(-0.1, 0.1, K):
                p = abi.FocusPlane()
                p.foc, p.wf = float(foc), wf
                p.image_pt[0], p.image_pt[1] = wl.image_pts[-1][0], wl.image_pts[-1][1]
                planes.append(p)
            opts = make_opts(flags=flags, out_mode=abi.OUT_FAN, first_surf=1, last_surf=N - 2)
            fan_opts = []
            for p in planes:
                o = make_opts(flags=flags, out_mode=abi.OUT_FAN, first_surf=1, last_surf=N - 2,
                              foc=p.foc, image_pt=tuple(p.image_pt), wf=p.wf)
                fan_opts.append(o)
            R = num * num
            res = eng.trace_pupil_grid(fld, grid, wi, fan_opts[0], want_pupil=False)
            stats_dev = torch.empty(K * 72, dtype=torch.uint8, device=eng.device)
            rows = torch.empty((K, 3, R), dtype=torch.float64, device=eng.device)
            import ctypes as C
            p_arr = (abi.FocusPlane * K)(*planes)
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

            def fused(rows_ptr=None, stats_ptr=stats_dev.data_ptr()):
                rc = eng.lib.rox_trace_through_focus(eng._handle, C.byref(fld), C.byref(grid), wi,
                                                     C.byref(opts), K, p_arr, rows_ptr, R, None,
                                                     stats_ptr, st)
                assert rc == 0, eng.lib.rox_last_error()

            def separate():
                for o in fan_opts:
                    eng.trace_pupil_grid(fld, grid, wi, o, want_pupil=False, out=res)

            t_one = timed(torch, lambda: eng.trace_pupil_grid(fld, grid, wi, fan_opts[0], want_pupil=False,
                                                              out=res), args.reps, args.trials)
            t_sep = timed(torch, separate, max(2, args.reps // 4), args.trials)
            t_stats = timed(torch, fused, args.reps, args.trials)
            t_rows = timed(torch, lambda: fused(rows.data_ptr(), None), args.reps, args.trials)
            r = dict(case=name, grid=num, rays=R, K=K, one_fan_us=t_one, k_fan_us=t_sep,
                     fused_stats_us=t_stats, fused_rows_us=t_rows, speedup_stats=t_sep / t_stats,
                     speedup_rows=t_sep / t_rows,
                     added_us_per_plane_stats=(t_stats - t_one) / max(K - 1, 1) if K > 1 else None)
            print(json.dumps(r), flush=True)
            results.append(r)
        eng.close()
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
