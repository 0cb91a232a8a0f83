#!/usr/bin/env python3
"""The projected solid angle pass (rox_projected_solid_angle, the kernel behind
analyses.relative_illumination) against the ROX_OUT_LAST launch that feeds it and against the host
route: DeviceResult.to_host of the same rows, then the NumPy restatement
(tests/solidangle_ref.py).  Timed with HIP events around `--reps` back-to-back calls after a
warm-up (the median of `--trials` runs), outputs in HBM, for the double Gauss, 9 (field,
wavelength) items, at num_rays in `--rays`: records only, records and cells, and both again with
the transmission rows of the FULL packets as weights.  Prints one JSON object per case.

    python tools/relative_illumination_bench.py [--rays 64 256 1024] [--reps 10] [--trials 5] [--json out.json]

read_gbps is the bytes the pass must read -- status of every ray and L, M of every OK ray: 17 B
per ray, 25 B with weights -- over the time of the records-only call; cells_gbps counts the 8 B
per cell written as well."""
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
    ap.add_argument('--model', default='dblgauss_c2')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--trials', type=int, default=5)
    ap.add_argument('--host-rays', type=int, default=1024, help='largest num_rays the host route is timed at')
    ap.add_argument('--json')
    args = ap.parse_args()
    import torch
    import rayoptics_amd  # noqa: F401
    from rayoptics_amd import abi, analyses, workloads
    from rayoptics_amd.engine import SA_ITEM_DTYPE, make_grid, records_view
    import solidangle_ref as SR
    model = workloads.TableModel(args.model)
    wvls = list(model.workload.table.wvls)
    assert len(model.fields) * len(wvls) == N_ITEMS
    results = []
    for n in args.rays:
        R = n * n
        eng, _f, _w, _sw, fs, wis, opts, flags = analyses._packet_items(model, model.fields, wvls, n, True,
                                                                        'relative_illumination_bench', abi.OUT_LAST)
        last = analyses._trace_packets(eng, fs, wis, opts, n)
        grid = make_grid((-1., -1.), (1., 1.), n)
        reps = max(1, args.reps // (4 if n >= 1024 else 1))
        sa = lambda res, **kw: eng.projected_solid_angle(res, n, on_device=True, **kw)     # noqa: E731
        items = records_view(sa(last)[0], SA_ITEM_DTYPE)
        n_ok = int(items['n_ok'].sum())
        t_rec = timed(torch, lambda: sa(last), reps, args.trials)
        t_cells = timed(torch, lambda: sa(last, want_cells=True), reps, args.trials)
        t_trace = timed(torch, lambda: eng.trace_pupil_grids(fs, wis, grid, opts, want_pupil=False, outs=last), reps,
                        args.trials)
        # the weighted pass reads the image slot of FULL packets and the transmission rows
        _e, _f, _w, _sw, ffs, fwis, fopts, fflags = analyses._packet_items(model, model.fields, wvls, n, True,
                                                                           'relative_illumination_bench')
        full = analyses._trace_packets(eng, ffs, fwis, fopts, n)
        rows, _s, _i = eng.surface_transmission(full, fflags, fwis, on_device=True)
        t_wrec = timed(torch, lambda: sa(full, weight=rows), reps, args.trials)
        t_wcells = timed(torch, lambda: sa(full, weight=rows, want_cells=True), reps, args.trials)
        del full, rows
        bytes_read = N_ITEMS * R + 16 * n_ok
        cell_bytes = N_ITEMS * (n - 1) * (n - 1) * 8
        r = {'case': args.model, 'items': N_ITEMS, 'rays': R, 'n_ok': n_ok,
             'solid_angle_records_us': t_rec, 'solid_angle_records_and_cells_us': t_cells,
             'weighted_records_us': t_wrec, 'weighted_records_and_cells_us': t_wcells,
             'last_trace_us': t_trace, 'entry_vs_last_trace': t_rec / t_trace,
             'bytes_read': bytes_read, 'read_gbps': bytes_read / (t_rec * 1e-6) / 1e9,
             'weighted_read_gbps': (bytes_read + 8 * n_ok) / (t_wrec * 1e-6) / 1e9,
             'cells_gbps': (bytes_read + cell_bytes) / (t_cells * 1e-6) / 1e9,
             'ri': analyses.RelativeIllumination(items.reshape(len(model.fields), len(wvls)),
                                                 [1.0] * len(wvls)).poly_ri.tolist()}
        if n <= args.host_rays:
            t0 = time.perf_counter()
            host = [x.to_host(want=('seg', 'status')) for x in last]
            t_copy = (time.perf_counter() - t0) * 1e6
            t0 = time.perf_counter()
            for h in host:
                SR.of_packet(h.seg, h.status, n)
            t_numpy = (time.perf_counter() - t0) * 1e6
            r.update(rows_to_host_us=t_copy, numpy_restatement_us=t_numpy,
                     host_route_vs_entry=(t_copy + t_numpy) / t_cells)
        print(json.dumps(r), flush=True)
        results.append(r)
        del last
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(results, fh, indent=1)


if __name__ == '__main__':
    main()
