#!/usr/bin/env python3
"""Encircled energy through focus (analyses.through_focus_ee and its rox_focus_ee /
rox_focus_psf_ee calls) against copying the rows or the PSFs to the host and doing the same in
NumPy (np.sort for the order statistics, searchsorted + bincount + cumsum for the counts and the
PSF sums).  Timed with HIP events around `--reps` back-to-back calls after a warm-up (the median
of `--trials` runs), for the double Gauss and the .zmx zoom of tests/golden/through_focus_map.npz
(every field x wavelength item) at K = 21: geometric at num_rays in `--rays`, diffraction at
(ndim, maxdim) in `--sizes`.  Prints one JSON line per case.

    python tools/through_focus_ee_bench.py [--K 21] [--rays 64 256 1024] [--sizes 32,128 64,256]
                                           [--reps 10] [--trials 5] [--json out.json]

rox_focus_ee is timed with fractions (0.5, 0.8) and 64 radii per plane, its outputs in HBM;
rows_gbps is the x, y and status bytes of one pass over the rows (17 B per ray and plane) over
that call's time (the radix select re-reads them once per pass)."""
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
FRACTIONS = (0.5, 0.8)
NR = 64


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


def numpy_geometric(rows, status, radii):
    """what a user does today on the host: per plane sort the squared distances of the OK rays"""
    n_items, K = rows.shape[:2]
    out = []
    for i in range(n_items):
        ok = status[i] == 0
        for k in range(K):
            x, y = rows[i, k, 0, ok], rows[i, k, 1, ok]
            d2 = np.sort(x * x + y * y)
            n = d2.size
            m = [min(max(int(np.ceil(f * n)), 1), n) for f in FRACTIONS] if n else []
            out.append((np.sqrt(d2[[v - 1 for v in m]]), np.searchsorted(d2, radii[i, k] ** 2, side='right')))
    return out


def numpy_diffraction(psf, radii):
    n_items, K, M, _M = psf.shape
    X = -PITCH * (np.arange(M) - M // 2)
    out = np.empty(radii.shape)
    for i in range(n_items):
        for k in range(K):
            p = psf[i, k]
            tot = p.sum()
            cx, cy = (p.sum(axis=1) * X).sum() / tot, (p.sum(axis=0) * X).sum() / tot
            d2 = ((X[:, None] - cx) ** 2 + (X[None, :] - cy) ** 2).ravel()
            b = np.searchsorted(radii[i, k] ** 2, d2)
            out[i, k] = np.cumsum(np.bincount(b, weights=p.ravel(), minlength=radii.shape[-1] + 1))[:-1] / tot
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--K', type=int, default=21)
    ap.add_argument('--rays', nargs='+', type=int, default=[64, 256, 1024])
    ap.add_argument('--sizes', nargs='+', default=['32,128', '64,256'])
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
        for n in args.rays:
            call = lambda: analyses.through_focus_ee(m, focs, num_rays=n, **kw)  # noqa: E731
            res = call()
            whole = timed(torch, call, max(1, args.reps // 5), args.trials)
            eng, fs, wis, grids, opts_list, planes = analyses._map_items(m, kw['flds'], kw['wvls'], focs, None, n, {})
            stats, rows = eng.trace_pupil_grids_focus(fs, wis, grids, opts_list, planes, want_rows=True)
            cen = np.nan_to_num(np.stack([stats['cx'], stats['cy']], axis=-1))
            R = n * n
            radii = np.sort(np.random.default_rng(n).uniform(0, 0.05, (F * W, K, NR)), axis=-1)
            t_ee = timed(torch, lambda: eng.focus_ee(rows, R, cen, radii, FRACTIONS, on_device=True),
                         args.reps, args.trials)
            t_ee_frac = timed(torch, lambda: eng.focus_ee(rows, R, cen, None, FRACTIONS, on_device=True),
                              args.reps, args.trials)
            t_copy = timed(torch, lambda: (rows.rows.cpu(), rows.status.cpu()), max(1, args.reps // 5), args.trials)
            h_rows, h_status = rows.rows.cpu().numpy(), rows.status.cpu().numpy()
            t_numpy = host_timed(lambda: numpy_geometric(h_rows, h_status, radii), 1, max(1, args.trials // 2))
            r = {'case': name, 'kind': 'geometric', 'items': F * W, 'K': K, 'rays': R, 'radii': NR,
                 'fractions': list(FRACTIONS), 'through_focus_ee_us': whole, 'focus_ee_call_us': t_ee,
                 'focus_ee_fractions_only_us': t_ee_frac,
                 'rows_gbps': F * W * K * R * 17 / (t_ee_frac * 1e-6) / 1e9,
                 'rows_copy_to_host_us': t_copy, 'numpy_sort_us': t_numpy,
                 'host_path_vs_focus_ee': (t_copy + t_numpy) / t_ee,
                 'best_focus_all': [float(v) for v in res.best_focus_all]}
            print(json.dumps(r), flush=True)
            results.append(r)
            del rows, h_rows
            torch.cuda.empty_cache()
        for size in args.sizes:
            n, M = (int(v) for v in size.split(','))
            pitch = np.full((F, W, K), PITCH)
            call = lambda: analyses.through_focus_ee(m, focs, kind='diffraction', num_rays=n, maxdim=M,  # noqa: E731
                                                     pitch=pitch, **kw)
            res = call()
            whole = timed(torch, call, max(1, args.reps // 5), args.trials)
            eng, fs, wis, grids, opts_list, planes = analyses._map_items(m, kw['flds'], kw['wvls'], focs, None, n, {})
            _none, rows = eng.trace_pupil_grids_focus(fs, wis, grids, opts_list, planes, want_rows=True,
                                                      want_stats=False)
            scale = np.array([1 / m.nm_to_sys_units(kw['wvls'][i % W]) for i in range(F * W)])
            psf, _st = eng.focus_psf(FocusRows(rows.rows, rows.status), n, M, scale)
            flat = pitch.reshape(F * W, K)
            radii = np.broadcast_to(np.linspace(0.0, PITCH * M / 2, 256), (F * W, K, 256))
            t_psf = timed(torch, lambda: eng.focus_psf(FocusRows(rows.rows, rows.status), n, M, scale),
                          args.reps, args.trials)
            t_ee = timed(torch, lambda: eng.focus_psf_ee(psf, flat, None, radii), args.reps, args.trials)
            t_copy = timed(torch, lambda: psf.cpu(), max(1, args.reps // 5), args.trials)
            host_psf = psf.cpu().numpy()
            t_numpy = host_timed(lambda: numpy_diffraction(host_psf, radii), 1, max(1, args.trials // 2))
            got, _c = eng.focus_psf_ee(psf, flat, None, radii)
            exp = numpy_diffraction(host_psf, radii)
            nbytes = psf.numel() * 8
            r = {'case': name, 'kind': 'diffraction', 'items': F * W, 'K': K, 'ndim': n, 'maxdim': M,
                 'radii': 256, 'psf_stack_mb': nbytes / 1e6, 'through_focus_ee_us': whole,
                 'focus_psf_call_us': t_psf, 'focus_psf_ee_call_us': t_ee,
                 'psf_ee_gbps': nbytes * 2 / (t_ee * 1e-6) / 1e9,
                 'psf_copy_to_host_us': t_copy, 'numpy_bincount_us': t_numpy,
                 'host_path_vs_focus_psf_ee': (t_copy + t_numpy) / t_ee,
                 'max_abs_vs_numpy': float(np.nanmax(np.abs(got - exp))),
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
