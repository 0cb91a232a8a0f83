#!/usr/bin/env python3
"""rox_huygens_psf (csrc/huygens.hip) on the double Gauss: 9 (field, wavelength) items, K focus
planes, R rays, nx x nx pixels, rows and outputs in HBM.

A figure is the median over `--trials` windows of back-to-back calls between HIP events after a
warm-up call, with the windows' range beside it.  Per shape:
  huygens_ms          the whole entry: operands, GEMM, finish
  operands_ms, gemm_ms, finish_ms, gemm_tflops
                      the three kernels per call, from kernel traces: `--entry-only` runs one shape's
                      entry alone under `rocprofv3 --kernel-trace --stats -d <dir>/k<K>_r<rays across>_s<pixels>`,
                      and `--fold <dir>` reads those traces into the records of a later plain run
  gemm_flop           8 K nx ny R per item, what the GEMM of the wavelets costs; call_tflops =
                      gemm_flop over the whole call's time, against the 78.6 TFLOP/s fp64 matrix peak
  focus_psf_*         in the same run rox_focus_psf, whose two GEMMs are the same cgemm_nt, at the
                      nearest shape (ndim = sqrt(R) capped at 256, maxdim = 2 ndim), 8 M n (n + M)
                      flop per plane
  analysis_ms         the whole analyses.huygens_psf call (two trace launches, the rows, the entry,
                      the statistics back), 3 fields x 3 wavelengths
  numpy_ms            tests/huygens_ref.py on rows copied to the host, where it takes under a minute
  direct_sum_ms       K nx ny R sine/cosine pairs per item at the 5.2e11 pairs/s rox_focus_gmtf
                      reached (profiles/r07_through_focus_gmtf_bench.json): the estimate of the
                      unfactorised sum

The last record is made without a GPU: the largest absolute difference between the peak-normalised
Huygens PSF (tests/huygens_ref.py on rows the CPU oracle traced, double Gauss on axis, 32 x 32 rays)
and the reference's FFT PSF of tests/golden at calc_psf's pixels -- what tests/test_huygens_host.py
asserts twice of.  `--fft-only` writes that record alone into an existing `--json`.

    python tools/huygens_psf_bench.py [--json out.json] [--shapes 64:64 128:128 256:128] [--K 1 21]"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

PEAK_MATRIX_TFLOPS = 78.6
GMTF_PAIRS_PER_S = 5.2e11


def window_ms(torch, fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def timed(torch, fn, reps, trials):
    fn()
    torch.cuda.synchronize()
    w = [window_ms(torch, fn, reps) for _ in range(trials)]
    return float(np.median(w)), [float(min(w)), float(max(w))]


def kernel_split(folder, calls):
    """{operands_ms, gemm_ms, finish_ms} per call of the entry from the kernel_stats csv rocprofv3
    left somewhere under ``folder`` for a run of ``calls`` calls, or {} where there is none"""
    import glob
    paths = glob.glob(os.path.join(folder, '**', '*kernel_stats.csv'), recursive=True)
    if not paths:
        return {}
    tot = {'huygens_operands': 0.0, 'cgemm_nt': 0.0, 'huygens_finish': 0.0}
    with open(paths[0]) as fh:
        for row in csv.DictReader(fh):
            for key in tot:
                if key in row['Name']:
                    tot[key] += float(row['TotalDurationNs'])
    return {'operands_ms': tot['huygens_operands'] / calls / 1e6, 'gemm_ms': tot['cgemm_nt'] / calls / 1e6,
            'finish_ms': tot['huygens_finish'] / calls / 1e6}


ENTRY_ONLY_CALLS = 6            # a warm-up and five calls


def fft_comparison():
    """the record of the CPU comparison with the reference's FFT PSF (see the module text)"""
    import test_huygens_host as T
    model, rows = T.on_axis_rows()
    return {'fft_psf_comparison': T.fft_differences(model, rows),
            'what': 'double Gauss on axis, 32 x 32 rays, peak-normalised PSFs at calc_psf pixels: largest absolute '
                    'difference, Huygens restatement on CPU-oracle rows against tests/golden (maxdim 64, 128) and, '
                    'for the wavefront scaled to 2 %, against the NumPy restatement of calc_psf'}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', nargs='+', default=['64:64', '128:128', '256:128'], help='rays across : pixels')
    ap.add_argument('--K', nargs='+', type=int, default=[1, 21])
    ap.add_argument('--model', default='dblgauss_c2')
    ap.add_argument('--pitch', type=float, default=0.001)
    ap.add_argument('--trials', type=int, default=5)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--entry-only', action='store_true', help='the entry alone, a few calls: for a kernel trace')
    ap.add_argument('--fold', help='folder of kernel traces of --entry-only runs to read into the records')
    ap.add_argument('--fft-only', action='store_true', help='(no GPU) refresh the FFT comparison record of --json')
    ap.add_argument('--json')
    args = ap.parse_args()
    if args.fft_only:
        with open(args.json) as fh:
            results = [r for r in json.load(fh) if 'fft_psf_comparison' not in r]
        with open(args.json, 'w') as fh:
            json.dump(results + [fft_comparison()], fh, indent=1)
        return
    import torch
    import rayoptics_amd  # noqa: F401
    import focus_map_fixture as fm
    import huygens_ref as HR
    from rayoptics_amd import analyses
    from rayoptics_amd.engine import FocusRows
    model = fm.FocusMapFixtureModel(fm.load(), 'dblgauss')      # the double Gauss with its reference spheres
    foc = model.focs[7]
    results = []
    for shape in args.shapes:
        num, S = (int(v) for v in shape.split(':'))
        kw = dict(flds=model.fields, wvls=model.wvls, num_rays=num, ref_foc=foc)
        hr = analyses.trace_huygens_rows(model, **kw)
        eng, R = hr.eng, hr.n_rays
        n_items = hr.rows.shape[0]
        for K in args.K:
            focs = list(foc + np.linspace(-0.1, 0.1, K)) if K > 1 else [foc]
            origins = np.stack([analyses.huygens_window(hr.centres.reshape(3, 3, 3)[f, 0, :2], S, args.pitch)
                                for f in range(3)])
            planes = analyses.huygens_planes(hr.centres, origins, focs, 3)
            call = lambda: eng.huygens_psf(hr.rows, hr.status, planes, S, S, args.pitch, args.pitch, n_rays=R,  # noqa: E731
                                           stats_on_device=True)
            flop = 8.0 * n_items * K * S * S * R
            if args.entry_only:
                for _ in range(ENTRY_ONLY_CALLS):
                    call()
                torch.cuda.synchronize()
                continue
            reps = int(max(1, min(20, 2e11 // flop)))
            t_call = timed(torch, call, reps, args.trials)
            # rox_focus_psf at the nearest shape: the same GEMM kernel, in the same run
            n = min(num, 256)
            M = 2 * n
            ld = int(hr.rows.shape[2])
            frows = torch.zeros((n_items, K, 3, ld), dtype=torch.float64, device=eng.device)
            frows[:, :, 2, :] = (hr.rows[:, 0, :] * 0.001)[:, None, :]
            fr = FocusRows(frows, hr.status)
            scale = np.ones(n_items)
            t_fpsf = timed(torch, lambda: eng.focus_psf(fr, n, M, scale), reps, args.trials)
            flop_fpsf = 8.0 * n_items * K * M * n * (n + M)
            del frows, fr
            t_an = timed(torch, lambda: analyses.huygens_psf(model, args.pitch, size=S, focs=focs, on_device=True, **kw),
                         1, args.trials)
            r = {'case': 'dblgauss', 'items': n_items, 'K': K, 'rays': R, 'pixels': [S, S], 'pixel_pitch': args.pitch,
                 'reps': reps, 'trials': args.trials, 'huygens_ms': t_call[0], 'huygens_ms_range': t_call[1],
                 'gemm_flop': flop, 'call_tflops': flop / (t_call[0] * 1e-3) / 1e12,
                 'call_share_of_matrix_peak': flop / (t_call[0] * 1e-3) / 1e12 / PEAK_MATRIX_TFLOPS,
                 'sincos_pairs_operands': float(n_items) * R * (K * S + S),
                 'sincos_pairs_direct': float(n_items) * K * S * S * R,
                 'direct_sum_ms_at_gmtf_rate': float(n_items) * K * S * S * R / GMTF_PAIRS_PER_S * 1e3,
                 'focus_psf_shape': [n, M], 'focus_psf_ms': t_fpsf[0], 'focus_psf_ms_range': t_fpsf[1],
                 'focus_psf_flop': flop_fpsf, 'focus_psf_tflops': flop_fpsf / (t_fpsf[0] * 1e-3) / 1e12,
                 'analysis_ms': t_an[0], 'analysis_ms_range': t_an[1], 'numpy_ms': None, 'max_abs_diff_from_numpy': None}
            if args.fold:
                r.update(kernel_split(os.path.join(args.fold, f'k{K}_r{num}_s{S}'), ENTRY_ONLY_CALLS))
                if r.get('gemm_ms'):
                    r['gemm_tflops'] = flop / (r['gemm_ms'] * 1e-3) / 1e12
                    r['gemm_share_of_matrix_peak'] = r['gemm_tflops'] / PEAK_MATRIX_TFLOPS
            if not args.no_host and float(n_items) * R * (K * S + S) <= 3e8:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                h_rows, h_status = hr.rows.cpu().numpy(), hr.status.cpu().numpy()
                _U, ref, _st = HR.huygens_psf(h_rows, None, h_status, planes, S, S, args.pitch, args.pitch, n_rays=R)
                r['numpy_ms'] = (time.perf_counter() - t0) * 1e3
                psf = call()[0].cpu().numpy()
                r['max_abs_diff_from_numpy'] = float(np.abs(psf - ref).max())
                r['numpy_vs_device'] = r['numpy_ms'] / t_call[0]
            print(json.dumps(r), flush=True)
            results.append(r)
        del hr
        torch.cuda.empty_cache()
    if args.entry_only:
        return
    results.append(fft_comparison())
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(results, fh, indent=1)


if __name__ == '__main__':
    main()
