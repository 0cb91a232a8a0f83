#!/usr/bin/env python3
"""Zernike fits through focus (rox_focus_zernike) against copying the rows to the host and
fitting each plane with numpy.linalg.lstsq.  The rows are the device's own through-focus rows of
9 items (fields x wavelengths, each over its own pupil box) of the double Gauss and of the .zmx
zoom at K planes; rox_focus_zernike is timed with HIP events around `--reps` back-to-back calls
after a warm-up (the median of `--trials` runs), outputs in HBM, circle = each box's circle.
Prints one JSON record with a case per (model, rays, J).

    python tools/through_focus_zernike_bench.py [--K 21] [--rays 64 256 1024] [--reps 5] [--trials 3]

bytes: the OPD component and the status read by each of the three passes (moments, refinement,
statistics): 3 x items x K x R x 8 + 3 x items x R; frac_8tbps that over the time at 8 TB/s.
copy_s: the rows and status to the host; lstsq_s: lstsq of every plane (at 1024^2 rays measured
on 3 planes and scaled to items x K)."""
import argparse
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
        out.append(a.elapsed_time(b) * 1e-3 / reps)      # s per call
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--K', type=int, default=21)
    ap.add_argument('--rays', type=int, nargs='+', default=[64, 256, 1024])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--trials', type=int, default=3)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    import torch
    import zernike_ref as ZR
    from rayoptics_amd import abi, workloads, zernike as Z
    from rayoptics_amd.analyses import zernike_circles
    from rayoptics_amd.engine import TraceEngine
    from test_gpu_through_focus import fan_opts, golden_wavefronts, make_planes
    from test_gpu_through_focus_map import boxes

    spot = abi.INTERSECT_OBJ | abi.CHECK_APERTURES | abi.APPLY_VIGNETTING
    n = 9
    cases = []
    for name in ('dblgauss_c2', 'zmx_evenasph_c3'):
        wl = workloads.load(name)
        eng = TraceEngine(wl.table)
        W = len(wl.table.wvls)
        fl = [wl.fields[i % len(wl.fields)] for i in range(n)]
        wi = [(i // len(wl.fields)) % W for i in range(n)]
        planes = [make_planes(a.K, golden_wavefronts(), seed=i) for i in range(n)]
        opts = [fan_opts(spot, wl.table.n_ifcs) for _ in fl]
        ws = np.full(n, 1700.0)
        for num in a.rays:
            grids = boxes(n, num)
            _s, fr = eng.trace_pupil_grids_focus(fl, wi, grids, opts, planes, want_rows=True, want_stats=False)
            circ = zernike_circles(grids, 'bbox', n, 'bench')
            R = num * num
            for J in ([37, 91] if num == max(a.rays) else [37]):
                terms = Z.fringe_terms(37) if J == 37 else Z.noll_terms(91)
                t = timed(torch, lambda: eng.focus_zernike(fr, grids, terms, ws, circ, on_device=True),
                          a.reps, a.trials)
                nbytes = 3 * n * a.K * R * 8 + 3 * n * R
                t0 = time.perf_counter()
                rows, status = fr.to_host()
                copy_s = time.perf_counter() - t0
                sub = 3 if num >= 1024 else n * a.K
                px, py = ZR.axes(tuple(grids[0].start), tuple(grids[0].stop), num)
                fit, _o, x, y = ZR.select(status[0], px, py, tuple(circ[0]))
                t0 = time.perf_counter()
                Zm = Z.zernike_eval(terms, x[fit], y[fit])
                for q in range(sub):
                    i, k = divmod(q, a.K)
                    np.linalg.lstsq(Zm, ws[i] * rows[i, k, 2, :R][fit], rcond=None)
                lstsq_s = (time.perf_counter() - t0) * (n * a.K) / sub
                cases.append(dict(model=name, items=n, K=a.K, rays=R, J=J, zernike_s=t, bytes=nbytes,
                                  gbps=nbytes / t / 1e9, frac_8tbps=nbytes / t / 8e12, copy_s=copy_s,
                                  lstsq_s=lstsq_s))
            del fr
            torch.cuda.empty_cache()
    rec = dict(tool='through_focus_zernike_bench', cases=cases)
    line = json.dumps(rec)
    print(line)
    if a.json:
        with open(a.json, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
