#!/usr/bin/env python3
"""Diffraction through focus (analyses.through_focus_psf: one trace, then rox_focus_psf over the
rows in HBM) against the same rows put through K device-resident rox_calc_psf calls and K
host-array analyses.calc_psf calls.  Timed with HIP events around `--reps` back-to-back calls
after a warm-up (the median of `--trials` runs), for the double Gauss of
tests/golden/through_focus.npz at K in {7, 21} and (ndim, maxdim) in {(32, 128), (64, 256),
(128, 512)}.  Prints one JSON line per case.

    python tools/through_focus_psf_bench.py [--K 7 21] [--reps 10] [--trials 5] [--json out.json]

call_tflops is the batched PSF's 8 M n (n + M) K flop over the time of the whole rox_focus_psf
call: its prepare, GEMM, scale and finishing kernels, launch overheads, and the copy of the
statistics to the host with its synchronise.  It understates the GEMMs' own rate; their kernel
TFLOP/s come from a separate `rocprofv3 --kernel-trace --stats` run."""
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
    ap.add_argument('--K', type=int, nargs='+', default=[7, 21])
    ap.add_argument('--sizes', nargs='+', default=['32,128', '64,256', '128,512'])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--trials', type=int, default=5)
    ap.add_argument('--json')
    args = ap.parse_args()
    import torch
    import rayoptics_amd  # noqa: F401
    from rayoptics_amd import abi, analyses
    from rayoptics_amd.engine import calc_psf
    import focus_fixture as FF

    class Model(FF.FocusFixtureModel):
        """any focus shift takes one of the fixture's spheres: the work does not depend on it"""
        def setup_pupil_coords(self, fld, wvl, foc, image_pt=None, image_delta=None):
            k = int(np.argmin(np.abs(np.array(self.focs) - foc)))
            return super().setup_pupil_coords(fld, wvl, self.focs[k], image_pt, image_delta)

    m = Model(FF.load(), 'dblgauss')
    fld, wvl = m.fields[0], m.wvl
    convert = 1 / m.nm_to_sys_units(wvl)
    results = []
    for K in args.K:
        focs = np.linspace(m.focs[0], m.focs[-1], K)
        for size in args.sizes:
            n, M = (int(v) for v in size.split(','))
            res = analyses.through_focus_psf(m, fld, wvl, focs, num_rays=n, maxdim=M, on_device=True)
            fused = timed(torch, lambda: analyses.through_focus_psf(m, fld, wvl, focs, num_rays=n, maxdim=M,
                                                                     on_device=True), args.reps, args.trials)
            # the rows once more, kept in HBM, for the per-plane paths
            tf_kw = {}
            grid = analyses._focus_grid(m, fld, None, n, tf_kw)
            planes = analyses._focus_planes(m, fld, wvl, list(focs))
            eng, f, wi, opts = analyses._launch_setup(m, fld, wvl, tf_kw, abi.OUT_FAN)
            _st, rows = eng.trace_pupil_grid_focus(f, grid, wi, opts, planes, want_rows=True)
            ok = rows.status == abi.OK
            opd = [torch.where(ok, convert * rows.rows[k, 2], torch.full_like(rows.rows[k, 2], float('nan')))
                   .reshape(n, n).contiguous() for k in range(K)]
            batched = timed(torch, lambda: eng.focus_psf(rows, n, M, convert), args.reps, args.trials)
            singles = timed(torch, lambda: [calc_psf(w, n, M) for w in opd], args.reps, args.trials)
            host_opd = [w.cpu().numpy() for w in opd]
            host = timed(torch, lambda: [analyses.calc_psf(w, n, M) for w in host_opd],
                         max(1, args.reps // 5), args.trials)
            same = all(torch.equal(res.psf[k], calc_psf(opd[k], n, M)) for k in range(K))
            flop = 8.0 * M * n * (n + M) * K
            r = {'case': 'dblgauss', 'K': K, 'ndim': n, 'maxdim': M,
                 'through_focus_psf_us': fused, 'focus_psf_call_us': batched,
                 'k_device_calc_psf_us': singles, 'k_host_calc_psf_us': host,
                 'fused_vs_k_device': singles / batched,
                 'call_tflops': flop / (batched * 1e-6) / 1e12,            # whole call, not kernel time
                 'single_call_tflops': flop / K / (singles / K * 1e-6) / 1e12,
                 'bit_identical': bool(same), 'best_focus_strehl': res.best_focus_strehl}
            print(json.dumps(r), flush=True)
            results.append(r)
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(results, fh, indent=1)


if __name__ == '__main__':
    main()
