#!/usr/bin/env python3
"""Beam footprints (analyses.beam_footprints and its rox_surface_footprints call) against what
the packets' only consumer was before: DeviceResult.to_host of the FULL packets and the NumPy
restatement (tests/footprint_ref.py without fsum).  Timed with HIP events around `--reps`
back-to-back calls after a warm-up (the median of `--trials` runs), for the double Gauss and the
.zmx zoom, 9 (field, wavelength) items, at num_rays in `--rays`.  Prints one JSON object per case.

    python tools/beam_footprints_bench.py [--rays 64 256 1024] [--reps 10] [--trials 5] [--json out.json]

read_gbps is the bytes the statistics pass must read (8 of a record's 10 rows of every counted
slot, status and fail_surf) over its time."""
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
    ap.add_argument('--no-analysis', action='store_true', help='skip the whole beam_footprints call')
    ap.add_argument('--json')
    args = ap.parse_args()
    import torch
    import rayoptics_amd  # noqa: F401
    from rayoptics_amd import analyses, workloads
    from rayoptics_amd.engine import make_grid
    import footprint_ref as FR
    results = []
    for name in args.models:
        model = workloads.TableModel(name)
        tbl = model.workload.table
        wvls = list(tbl.wvls)
        F, W = len(model.fields), len(wvls)
        assert F * W == N_ITEMS
        for n in args.rays:
            R = n * n
            eng, _f, _w, _sw, fs, wis, opts, flags = analyses._packet_items(model, model.fields, wvls, n, False,
                                                                            'beam_footprints_bench')
            res = analyses._trace_packets(eng, fs, wis, opts, n)
            rec, _m = eng.surface_footprints(res, flags)
            n_seg = rec.shape[1]
            hw = np.sqrt(np.maximum(rec['r2_max'].max(axis=0), 1e-12)) * analyses.FOOTPRINT_MAP_MARGIN
            reps = max(1, args.reps // (4 if n >= 1024 else 1))
            t_stats = timed(torch, lambda: eng.surface_footprints(res, flags, on_device=True), reps, args.trials)
            t_maps = timed(torch, lambda: eng.surface_footprints(res, flags, half_width=hw, n_bins=128, on_device=True),
                           reps, args.trials)
            t_maps_only = timed(torch, lambda: eng.surface_footprints(res, flags, half_width=hw, n_bins=128,
                                                                      on_device=True, want_records=False),
                                reps, args.trials)
            t_trace = timed(torch, lambda: eng.trace_pupil_grids(fs, wis, make_grid((-1., -1.), (1., 1.), n), opts,
                                                                 want_pupil=False, outs=res), reps, args.trials)
            bytes_read = int(rec['n'].sum()) * 64 + N_ITEMS * R * 3
            r = {'case': name, 'items': N_ITEMS, 'rays': R, 'n_seg': int(n_seg),
                 'packet_mb': N_ITEMS * n_seg * 80 * R / 1e6,
                 'footprints_stats_us': t_stats, 'footprints_stats_and_128_maps_us': t_maps,
                 'footprints_128_maps_only_us': t_maps_only, 'full_trace_us': t_trace,
                 'read_gbps': bytes_read / (t_stats * 1e-6) / 1e9}
            if not args.no_analysis:
                call = lambda: analyses.beam_footprints(model, flds=model.fields, wvls=wvls, num_rays=n, maps=128)  # noqa: E731
                r['beam_footprints_us'] = timed(torch, call, max(1, reps // 5), args.trials)
                r['beam_footprints_items'] = F * W
            if n <= args.host_rays:
                t0 = time.perf_counter()
                host = [x.to_host(want=('seg', 'status', 'fail_surf')) for x in res]
                t_copy = (time.perf_counter() - t0) * 1e6
                t0 = time.perf_counter()
                for h in host:
                    FR.footprints(tbl, flags, h.seg, h.status, h.fail_surf, exact=False)
                t_numpy = (time.perf_counter() - t0) * 1e6
                r.update(packets_to_host_us=t_copy, numpy_restatement_us=t_numpy,
                         host_path_vs_footprints=(t_copy + t_numpy) / t_stats)
            print(json.dumps(r), flush=True)
            results.append(r)
            del res
            torch.cuda.empty_cache()
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(results, fh, indent=1)


if __name__ == '__main__':
    main()
