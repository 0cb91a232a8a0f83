#!/usr/bin/env python3
"""MTF through focus (analyses.through_focus_mtf: one trace, rox_focus_psf over every item, then
rox_focus_mtf over the PSFs in HBM) against copying the PSFs to the host and taking the same line
OTFs with NumPy (tests/line_otf.py).  Timed with HIP events around `--reps` back-to-back calls
after a warm-up (the median of `--trials` runs), for the double Gauss's 3 fields x 3 wavelengths
of tests/golden/through_focus_map.npz at K = 21, Q = 8 frequencies up to 0.45 / pitch, and
(ndim, maxdim) in {(32, 128), (64, 256), (128, 512)}.  Prints one JSON line per case.

    python tools/through_focus_mtf_bench.py [--K 21] [--Q 8] [--reps 10] [--trials 5] [--json out.json]

mtf_gbps is the PSF stack's bytes (read once) over the time of the whole rox_focus_mtf call:
its three kernels, launch overheads, the staging of pitch and freqs, and the copy of the OTFs to
the host with its synchronise."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

PITCH = 1e-3        # system units per PSF pixel: the work does not depend on it


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


def host_timed(fn, reps, trials):
    fn()
    out = []
    for _ in range(trials):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        out.append((time.perf_counter() - t0) * 1e6 / reps)
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--K', type=int, default=21)
    ap.add_argument('--Q', type=int, default=8)
    ap.add_argument('--sizes', nargs='+', default=['32,128', '64,256', '128,512'])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--trials', type=int, default=5)
    ap.add_argument('--json')
    args = ap.parse_args()
    import torch
    import rayoptics_amd  # noqa: F401
    from rayoptics_amd import analyses
    from rayoptics_amd.engine import FocusRows
    import focus_map_fixture as FM
    import line_otf as LO

    class Model(FM.FocusMapFixtureModel):
        """any focus shift takes one of the fixture's spheres: the work does not depend on it"""
        def setup_pupil_coords(self, fld, wvl, foc, image_pt=None, image_delta=None):
            k = int(np.argmin(np.abs(np.array(self.focs) - foc)))
            return super().setup_pupil_coords(fld, wvl, self.focs[k], image_pt, image_delta)

    m = Model(FM.load(), 'dblgauss')
    kw = m.map_kwargs()
    F, W, K = len(kw['flds']), len(kw['wvls']), args.K
    focs = np.linspace(m.focs[0], m.focs[-1], K)
    nu = np.linspace(0.0, 0.45 / PITCH, args.Q)
    pitch = np.full((F, W, K), PITCH)
    results = []
    for size in args.sizes:
        n, M = (int(v) for v in size.split(','))
        call = lambda: analyses.through_focus_mtf(m, focs, nu, num_rays=n, maxdim=M, pitch=pitch, **kw)  # noqa: E731
        res = call()
        whole = timed(torch, call, args.reps, args.trials)
        # the PSF stack once more, kept in HBM, for the stage timings
        radii = []
        eng, fs, wis, grids, opts_list, planes = analyses._map_items(m, kw['flds'], kw['wvls'], focs, None, n, {},
                                                                     radii=radii)
        _none, rows = eng.trace_pupil_grids_focus(fs, wis, grids, opts_list, planes, want_rows=True,
                                                  want_stats=False)
        scale = np.array([1 / m.nm_to_sys_units(kw['wvls'][i % W]) for i in range(F * W)])
        rows = FocusRows(rows.rows, rows.status)
        psf, _st = eng.focus_psf(rows, n, M, scale)
        flat = pitch.reshape(F * W, K)
        t_psf = timed(torch, lambda: eng.focus_psf(rows, n, M, scale), args.reps, args.trials)
        t_mtf_host = timed(torch, lambda: eng.focus_mtf(psf, flat, nu), args.reps, args.trials)
        t_mtf_dev = timed(torch, lambda: eng.focus_mtf(psf, flat, nu, on_device=True), args.reps, args.trials)
        t_copy = timed(torch, lambda: psf.cpu(), max(1, args.reps // 5), args.trials)
        host_psf = psf.cpu().numpy()
        t_numpy = host_timed(lambda: LO.line_otf(host_psf, flat, nu), 1, max(1, args.trials // 2))
        got = eng.focus_mtf(psf, flat, nu)
        exp = LO.line_otf(host_psf, flat, nu)
        ok = ~np.isnan(exp)
        nbytes = psf.numel() * 8
        r = {'case': 'dblgauss', 'items': F * W, 'K': K, 'Q': args.Q, 'ndim': n, 'maxdim': M,
             'psf_stack_mb': nbytes / 1e6,
             'through_focus_mtf_us': whole, 'focus_psf_call_us': t_psf,
             'focus_mtf_call_us': t_mtf_host, 'focus_mtf_device_dst_us': t_mtf_dev,
             'mtf_gbps': nbytes / (t_mtf_host * 1e-6) / 1e9,
             'psf_copy_to_host_us': t_copy, 'numpy_line_otf_us': t_numpy,
             'host_path_vs_focus_mtf': (t_copy + t_numpy) / t_mtf_host,
             'max_abs_vs_numpy': float(np.max(np.abs(got[ok] - exp[ok]))), 'finite_otf_entries': int(ok.sum()),
             'otf_entries': int(ok.size), 'min_finite_mtf': float(np.min(np.abs(got[ok]))),
             'same_as_analysis': bool(got.reshape(res.otf.shape).tobytes() == res.otf.tobytes()),
             'best_focus_all': [float(v) for v in res.best_focus_all]}
        print(json.dumps(r), flush=True)
        results.append(r)
        del psf, host_psf, rows
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(results, fh, indent=1)


if __name__ == '__main__':
    main()
