#!/usr/bin/env python3
"""Fresnel transmission (rox_surface_transmission and analyses.transmission) against what the
packets' only consumer was before: DeviceResult.to_host of the FULL packets and the NumPy
restatement (tests/fresnel_ref.py, formulation A).  Timed with HIP events around `--reps`
back-to-back calls after a warm-up (the median of `--trials` runs), outputs in HBM, for the double
Gauss and the .zmx zoom, 9 (field, wavelength) items, at num_rays in `--rays`; beside it
rox_surface_footprints on the same packets (it reads 8 of a record's 10 rows, this entry 6).
Prints one JSON object per case.

    python tools/transmission_bench.py [--rays 64 256 1024] [--reps 10] [--trials 5] [--json out.json]

read_gbps is the bytes the pass must read (6 of a record's 10 rows of every slot of every OK ray,
and status) over the time of the records-only call; rows_gbps counts the 4 rows written as well."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

N_ITEMS = 9


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
    ap.add_argument('--rays', nargs='+', type=int, default=[64, 256, 1024])
    ap.add_argument('--models', nargs='+', default=['dblgauss_c2', 'zmx_evenasph_c3'])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--trials', type=int, default=5)
    ap.add_argument('--host-rays', type=int, default=256, help='largest num_rays the host path is timed at')
    ap.add_argument('--no-analysis', action='store_true', help='skip the whole transmission() call')
    ap.add_argument('--json')
    args = ap.parse_args()
    import torch
    import rayoptics_amd  # noqa: F401
    from rayoptics_amd import analyses, workloads
    from rayoptics_amd.engine import make_grid
    import fresnel_ref as FR
    results = []
    for name in args.models:
        model = workloads.TableModel(name)
        tbl = model.workload.table
        wvls = list(tbl.wvls)
        F, W = len(model.fields), len(wvls)
        assert F * W == N_ITEMS
        for n in args.rays:
            R = n * n
            eng, _f, _w, _sw, fs, wis, opts, flags = analyses._packet_items(model, model.fields, wvls, n, True,
                                                                            'transmission_bench')
            res = analyses._trace_packets(eng, fs, wis, opts, n)
            _r, surf, item = eng.surface_transmission(res, flags, wis, want_rows=False)
            n_seg = surf.shape[1]
            n_ok = int(item['n_ok'].sum())
            reps = max(1, args.reps // (4 if n >= 1024 else 1))
            t_rec = timed(torch, lambda: eng.surface_transmission(res, flags, wis, want_rows=False, on_device=True),
                          reps, args.trials)
            t_rows = timed(torch, lambda: eng.surface_transmission(res, flags, wis, on_device=True), reps, args.trials)
            t_fp = timed(torch, lambda: eng.surface_footprints(res, flags, ok_only=True, on_device=True), reps,
                         args.trials)
            t_trace = timed(torch, lambda: eng.trace_pupil_grids(fs, wis, make_grid((-1., -1.), (1., 1.), n), opts,
                                                                 want_pupil=False, outs=res), reps, args.trials)
            bytes_read = n_ok * n_seg * 48 + N_ITEMS * R
            r = {'case': name, 'items': N_ITEMS, 'rays': R, 'n_seg': int(n_seg), 'n_ok': n_ok,
                 'packet_mb': N_ITEMS * n_seg * 80 * R / 1e6,
                 'transmission_records_us': t_rec, 'transmission_rows_and_records_us': t_rows,
                 'footprints_stats_ok_only_us': t_fp, 'full_trace_us': t_trace,
                 'read_gbps': bytes_read / (t_rec * 1e-6) / 1e9,
                 'rows_gbps': (bytes_read + N_ITEMS * R * 32) / (t_rows * 1e-6) / 1e9,
                 'mean_T': float(item['t_sum'].sum() / max(n_ok, 1))}
            if not args.no_analysis:
                call = lambda: analyses.transmission(model, flds=model.fields, wvls=wvls, num_rays=n)  # noqa: E731
                r['transmission_analysis_us'] = timed(torch, call, max(1, reps // 5), args.trials)
                r['transmission_analysis_items'] = F * W
            if n <= args.host_rays:
                t0 = time.perf_counter()
                host = [x.to_host(want=('seg', 'status')) for x in res]
                t_copy = (time.perf_counter() - t0) * 1e6
                t0 = time.perf_counter()
                for h, wi in zip(host, wis):
                    FR.transmission_a(tbl, flags, h.seg, h.status, wi)
                t_numpy = (time.perf_counter() - t0) * 1e6
                r.update(packets_to_host_us=t_copy, numpy_restatement_us=t_numpy,
                         host_path_vs_transmission=(t_copy + t_numpy) / t_rows)
            print(json.dumps(r), flush=True)
            results.append(r)
            del res
            torch.cuda.empty_cache()
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(results, fh, indent=1)


if __name__ == '__main__':
    main()
