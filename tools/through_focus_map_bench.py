#!/usr/bin/env python3
"""One batched through-focus launch over every (field, wavelength) item (rox_trace_through_focus_grids)
against F x W single rox_trace_through_focus calls of the same items, timed with HIP events around
`--reps` back-to-back calls after a warm-up (the median of `--trials` such runs is reported), both
with device statistics.  Also the host side of analyses.through_focus_map: its wall time end to end
minus the wall time of its device call (planes, grids and options built per item).

    python tools/through_focus_map_bench.py [--K 21] [--num 64 128 512] [--reps 20] [--trials 5] [--json out.json]

Cases: the double Gauss (3 fields x 3 wavelengths) and the .zmx even-asphere zoom (every field x
wavelength of tests/golden/through_focus_map.npz), each item over its own field's vignetting box,
its planes K focus shifts across the stored range with the nearest stored reference sphere."""
import argparse
import ctypes as C
import json
import os
import sys
import time

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


def wall(fn, trials):
    fn()
    out = []
    for _ in range(trials):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--K', type=int, default=21)
    ap.add_argument('--num', type=int, nargs='+', default=[64, 128, 512])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--trials', type=int, default=5)
    ap.add_argument('--json')
    args = ap.parse_args()
    import torch
    import rayoptics_amd  # noqa: F401
    from rayoptics_amd import abi, analyses, session
    from rayoptics_amd.engine import make_grid, make_opts
    from rayoptics_amd.trace import _launch_setup
    import focus_map_fixture as FM
    z = FM.load()
    results = []

    class Model(FM.FocusMapFixtureModel):
        """K focus shifts across the stored range, each with the nearest stored sphere (the
        kernel's per-plane work does not depend on the values)"""

        def setup_pupil_coords(self, fld, wvl, foc, image_pt=None, image_delta=None):
            k = int(np.argmin(np.abs(np.array(self.focs) - foc)))
            return super().setup_pupil_coords(fld, wvl, self.focs[k])

    for name in FM.MODELS:
        m = Model(z, name)
        kw = m.map_kwargs()
        focs = [float(f) for f in np.linspace(m.focs[0], m.focs[-1], args.K)]
        eng = session.engine_for(m)
        N = eng.table.n_ifcs
        F, W = len(m.fields), len(m.wvls)
        n = F * W
        planes, fs, wis, opts = [], [], [], []
        for fld in m.fields:
            for wvl in m.wvls:
                planes.append(analyses._focus_planes(m, fld, wvl, focs))
                _e, f, wi, o = _launch_setup(m, fld, wvl, {'check_apertures': True}, abi.OUT_FAN)
                fs.append(f)
                wis.append(wi)
                opts.append(o)
        K = len(focs)
        p_flat = (abi.FocusPlane * (n * K))(*[p for ps in planes for p in ps])
        p_items = [(abi.FocusPlane * K)(*ps) for ps in planes]
        f_arr, w_arr, o_arr = (abi.Field * n)(*fs), (C.c_int32 * n)(*wis), (abi.Opts * n)(*opts)
        stats_dev = torch.empty(n * K * 72, dtype=torch.uint8, device=eng.device)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for num in args.num:
            grids = [make_grid(m.z['bbox'][i // W, 0], m.z['bbox'][i // W, 1], num) for i in range(n)]
            g_arr = (abi.Grid * n)(*grids)

            def batched():
                rc = eng.lib.rox_trace_through_focus_grids(eng._handle, n, f_arr, w_arr, g_arr, o_arr, K,
                                                           p_flat, None, 0, None, stats_dev.data_ptr(), st)
                assert rc == 0, eng.lib.rox_last_error()

            def singles():
                for i in range(n):
                    rc = eng.lib.rox_trace_through_focus(eng._handle, C.byref(fs[i]), C.byref(grids[i]), wis[i],
                                                         C.byref(opts[i]), K, p_items[i], None, 0, None,
                                                         stats_dev.data_ptr() + i * K * 72, st)
                    assert rc == 0, eng.lib.rox_last_error()

            t_batch = timed(torch, batched, args.reps, args.trials)
            t_single = timed(torch, singles, max(2, args.reps // 4), args.trials)
            # analyses.through_focus_map end to end (host statistics: synchronous) and its device call
            t_map = wall(lambda: analyses.through_focus_map(m, focs, num_rays=num, **kw), args.trials)
            t_call = wall(lambda: eng.trace_pupil_grids_focus(fs, wis, grids, opts, planes), args.trials)
            r = dict(case=name, items=n, K=K, grid=num, rays_per_item=num * num, batched_us=t_batch,
                     singles_us=t_single, speedup=t_single / t_batch, map_wall_us=t_map,
                     device_call_wall_us=t_call, host_planes_us=t_map - t_call)
            print(json.dumps(r), flush=True)
            results.append(r)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
