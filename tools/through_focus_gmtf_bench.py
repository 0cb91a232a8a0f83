#!/usr/bin/env python3
"""Geometric MTF through focus (analyses.through_focus_gmtf and its rox_focus_gmtf call) against
what the host route costs: copying the rows the call reads (x, y and status) to the host, and NumPy
forming the same sums there.  Timed with HIP events around `--reps` back-to-back calls after a
warm-up (the median of `--trials` runs), for the double Gauss and the .zmx zoom of
tests/golden/through_focus_map.npz (every field x wavelength item) at K = 21, D = 4 directions
(x, y, t, s) and Q = 16 frequencies, at num_rays in `--rays`.  NumPy runs up to `--numpy-rays`
across (1024^2 is skipped: it is the 256^2 figure times 16).  For context, rox_focus_psf +
rox_focus_mtf of the diffraction route at (ndim, maxdim) = `--psf`.  Prints one JSON line per case.

    python tools/through_focus_gmtf_bench.py [--K 21] [--rays 64 256 1024] [--reps 10] [--trials 5]
                                             [--json out.json]

sincos_per_s is OK rays x D x Q over the call's time.  device_vs_rows_copy is the time of the
device-to-host copy of the rows the call reads over the call's time: the host route cannot begin
before that copy ends."""
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
FREQS = np.linspace(0.0, 100.0, 16)
DIRECTIONS = ('x', 'y', 't', 's')


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


def numpy_gmtf(xy, status, dirs):
    """what a user does on the host: per plane and direction, mean(exp(-2 pi i nu u)) of the OK rays"""
    n_items, K = xy.shape[:2]
    out = np.full((n_items, K, dirs.shape[1], FREQS.size), np.nan + 0j)
    for i in range(n_items):
        ok = status[i] == 0
        if not ok.any():
            continue
        for k in range(K):
            x, y = xy[i, k, 0, ok], xy[i, k, 1, ok]
            for d, (ex, ey) in enumerate(dirs[i]):
                u = ex * x + ey * y
                out[i, k, d] = np.exp(-2j * np.pi * FREQS[:, None] * u[None, :]).mean(axis=1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--K', type=int, default=21)
    ap.add_argument('--rays', nargs='+', type=int, default=[64, 256, 1024])
    ap.add_argument('--numpy-rays', type=int, default=256)
    ap.add_argument('--psf', default='64,256')
    ap.add_argument('--models', nargs='+', default=['dblgauss', 'zmx_evenasph_c3'])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--trials', type=int, default=5)
    ap.add_argument('--json')
    args = ap.parse_args()
    import torch
    import rayoptics_amd  # noqa: F401
    from rayoptics_amd import analyses
    from rayoptics_amd.engine import FocusRows
    import focus_map_fixture as FM

    class Model(FM.FocusMapFixtureModel):
        """any focus shift takes one of the fixture's spheres: the work does not depend on it"""
        def setup_pupil_coords(self, fld, wvl, foc, image_pt=None, image_delta=None):
            k = int(np.argmin(np.abs(np.array(self.focs) - foc)))
            return super().setup_pupil_coords(fld, wvl, self.focs[k], image_pt, image_delta)

    results = []
    for name in args.models:
        m = Model(FM.load(), name)
        kw = m.map_kwargs()
        F, W, K = len(kw['flds']), len(kw['wvls']), args.K
        focs = np.linspace(m.focs[0], m.focs[-1], K)
        ref = kw['wvls'].index(kw['ref_wvl'])
        for n in args.rays:
            call = lambda: analyses.through_focus_gmtf(m, focs, FREQS, num_rays=n, directions=DIRECTIONS, **kw)  # noqa: E731
            res = call()
            whole = timed(torch, call, max(1, args.reps // 5), args.trials)
            eng, fs, wis, grids, opts_list, planes = analyses._map_items(m, kw['flds'], kw['wvls'], focs, None, n, {})
            _stats, rows = eng.trace_pupil_grids_focus(fs, wis, grids, opts_list, planes, want_rows=True)
            ip = analyses._image_pts(planes).reshape(F, W, K, 2)
            dirs, _labels = analyses.gmtf_directions(DIRECTIONS, ip[:, ref, int(np.argmin(np.abs(focs)))])
            dirs = np.repeat(dirs, W, axis=0)
            R, D, Q = n * n, len(DIRECTIONS), FREQS.size
            t_call = timed(torch, lambda: eng.focus_gmtf(rows, R, dirs, FREQS, on_device=True), args.reps, args.trials)
            edges = np.linspace(-0.3, 0.3, 257)
            t_lsf = timed(torch, lambda: eng.focus_gmtf(rows, R, dirs, None, edges=edges, on_device=True), args.reps,
                          args.trials)
            # the rows the call reads: x and y of every plane, and the status bytes
            t_copy = timed(torch, lambda: (rows.rows[:, :, :2].cpu(), rows.status.cpu()), max(1, args.reps // 5),
                           args.trials)
            t_copy_all = timed(torch, lambda: (rows.rows.cpu(), rows.status.cpu()), max(1, args.reps // 5), args.trials)
            otf, _l, n_ok = eng.focus_gmtf(rows, R, dirs, FREQS)
            pairs = float(n_ok.sum()) * D * Q
            r = {'case': name, 'items': F * W, 'K': K, 'rays': R, 'dirs': D, 'freqs': Q,
                 'ok_rays_per_plane_mean': float(n_ok.mean()), 'through_focus_gmtf_us': whole,
                 'focus_gmtf_call_us': t_call, 'focus_gmtf_lsf_256_bins_us': t_lsf, 'sincos_pairs': pairs,
                 'sincos_per_s': pairs / (t_call * 1e-6),
                 'rows_read_mb': (F * W * K * R * 16 + F * W * R) / 1e6,
                 'rows_read_copy_to_host_us': t_copy, 'all_rows_copy_to_host_us': t_copy_all,
                 'device_vs_rows_copy': t_copy / t_call,
                 'best_focus_all': [float(v) for v in res.best_focus_all]}
            if n <= args.numpy_rays:
                xy, h_status = rows.rows[:, :, :2].cpu().numpy(), rows.status.cpu().numpy()
                r['numpy_us'] = host_timed(lambda: numpy_gmtf(xy, h_status, dirs), 1, max(1, args.trials // 2))
                exp = numpy_gmtf(xy, h_status, dirs)
                r['max_abs_vs_numpy'] = float(np.nanmax(np.abs(otf - exp)))
                r['host_path_vs_focus_gmtf'] = (t_copy + r['numpy_us']) / t_call
                del xy
            print(json.dumps(r), flush=True)
            results.append(r)
            del rows
            torch.cuda.empty_cache()
        # context: the diffraction route's two calls
        nd, M = (int(v) for v in args.psf.split(','))
        eng, fs, wis, grids, opts_list, planes = analyses._map_items(m, kw['flds'], kw['wvls'], focs, None, nd, {})
        _none, rows = eng.trace_pupil_grids_focus(fs, wis, grids, opts_list, planes, want_rows=True, want_stats=False)
        scale = np.array([1 / m.nm_to_sys_units(kw['wvls'][i % W]) for i in range(F * W)])
        part = FocusRows(rows.rows, rows.status)
        psf, _st = eng.focus_psf(part, nd, M, scale)
        flat = np.full((F * W, K), PITCH)
        nu = FREQS[FREQS * PITCH <= 0.5]
        t_psf = timed(torch, lambda: eng.focus_psf(part, nd, M, scale), args.reps, args.trials)
        t_mtf = timed(torch, lambda: eng.focus_mtf(psf, flat, nu, on_device=True), args.reps, args.trials)
        r = {'case': name, 'kind': 'diffraction context', 'items': F * W, 'K': K, 'ndim': nd, 'maxdim': M,
             'freqs': int(nu.size), 'focus_psf_call_us': t_psf, 'focus_mtf_call_us': t_mtf}
        print(json.dumps(r), flush=True)
        results.append(r)
        del psf, rows
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(results, fh, indent=1)


if __name__ == '__main__':
    main()
