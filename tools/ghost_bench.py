#!/usr/bin/env python3
"""The segment-foci pass (rox_segment_foci, the reduction behind analyses.ghost_analysis) on the
packets of one double Gauss ghost, against rox_surface_footprints on the same packets (the
yardstick: the sibling pass over the same rows) and against the host route: DeviceResult.to_host
of the packets, then the NumPy restatement (tests/segfoci_ref.py).  Timed with HIP events around
`--reps` back-to-back calls after a warm-up (the median of `--trials` runs), outputs in HBM, 9
(field, wavelength) items, at num_rays in `--rays`.  Then the whole analyses.ghost_analysis call
over all pairs of the double Gauss at `--analysis-rays`, split into table and system creation,
trace, thin-film walk and foci (host clocks around synchronised steps).  One JSON object per case.

    python tools/ghost_bench.py [--rays 64 256 1024] [--pair 7 3] [--reps 10] [--trials 5] [--json out.json]

read_gbps is the bytes the pass must read -- the status of every ray, and of every OK ray its
weight and 7 of a record's 10 rows at every slot: 1 + 8*(1 + 7*n_seg) B -- over the time of the
weighted call; footprints_read_gbps counts the 1 + 2 + 8*8*n_seg B per ray of that pass (status,
fail_surf and 8 rows)."""
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
    ap.add_argument('--pair', nargs=2, type=int, default=[7, 3])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--trials', type=int, default=5)
    ap.add_argument('--host-rays', type=int, default=256, help='largest num_rays the host route is timed at')
    ap.add_argument('--analysis-rays', type=int, default=64)
    ap.add_argument('--json')
    args = ap.parse_args()
    import torch
    import rayoptics_amd  # noqa: F401
    from rayoptics_amd import abi, analyses, ghost, session, workloads
    from rayoptics_amd.engine import SEG_FOCUS_DTYPE, records_view
    import segfoci_ref as SR
    model = workloads.TableModel(args.model)
    table = model.workload.table
    wvls = list(table.wvls)
    assert len(model.fields) * len(wvls) == N_ITEMS
    j, i = args.pair
    unf = ghost.unfold(table, j, i)
    geng = session.engine_for_table(unf.table)
    ct = ghost.coating_tables(table, unf, None)
    results = []
    for n in args.rays:
        R = n * n
        _e, _f, _w, _sw, fs, wis, opts, flags = analyses._packet_items(model, model.fields, wvls, n, True, 'ghost_bench')
        gopts = []
        for o in opts:
            g = abi.Opts.from_buffer_copy(bytes(o))
            g.last_surf = unf.table.n_ifcs - 2
            gopts.append(g)
        res = analyses._trace_packets(geng, fs, wis, gopts, n)
        wv = [float(table.wvls[w]) for w in wis]
        rows, _s, _i = geng.surface_thinfilm(res, flags, wis, wv, on_device=True, **ct)
        reps = max(1, args.reps // (4 if n >= 1024 else 1))
        rec = records_view(geng.segment_foci(res, flags, weight=rows, on_device=True), SEG_FOCUS_DTYPE)
        n_seg = rec.shape[1]
        n_ok = int(rec['n'][:, 0].sum() + rec['n_flat'][:, 0].sum() + rec['n_bad'][:, 0].sum())
        t_w = timed(torch, lambda: geng.segment_foci(res, flags, weight=rows, on_device=True), reps, args.trials)
        t_u = timed(torch, lambda: geng.segment_foci(res, flags, on_device=True), reps, args.trials)
        t_win = timed(torch, lambda: geng.segment_foci(res, flags, weight=rows, window=(12.0, 18.0), on_device=True),
                      reps, args.trials)
        t_fp = timed(torch, lambda: geng.surface_footprints(res, flags, ok_only=True, on_device=True), reps, args.trials)
        t_film = timed(torch, lambda: geng.surface_thinfilm(res, flags, wis, wv, on_device=True, **ct), reps, args.trials)
        bytes_read = N_ITEMS * R + 8 * n_ok * (1 + 7 * n_seg)
        fp_bytes = 3 * N_ITEMS * R + 8 * n_ok * 8 * n_seg
        r = {'case': args.model, 'pair': [j, i], 'items': N_ITEMS, 'rays': R, 'n_seg': n_seg, 'n_ok': n_ok,
             'segment_foci_weighted_us': t_w, 'segment_foci_unweighted_us': t_u, 'segment_foci_window_us': t_win,
             'footprints_stats_ok_only_us': t_fp, 'thinfilm_walk_us': t_film,
             'bytes_read': bytes_read, 'read_gbps': bytes_read / (t_w * 1e-6) / 1e9,
             'footprints_bytes_read': fp_bytes, 'footprints_read_gbps': fp_bytes / (t_fp * 1e-6) / 1e9}
        r['gbps_vs_footprints'] = r['read_gbps'] / r['footprints_read_gbps']
        if n <= args.host_rays:
            t0 = time.perf_counter()
            host = [x.to_host(want=('seg', 'status')) for x in res]
            wh = rows.cpu().numpy()
            t_copy = (time.perf_counter() - t0) * 1e6
            t0 = time.perf_counter()
            for h, w in zip(host, wh):
                SR.segment_foci(np.asarray(h.seg), h.status, w[0])
            t_numpy = (time.perf_counter() - t0) * 1e6
            r.update(packets_to_host_us=t_copy, numpy_restatement_us=t_numpy,
                     host_route_vs_entry=(t_copy + t_numpy) / t_w)
        print(json.dumps(r), flush=True)
        results.append(r)
        del res, rows
        torch.cuda.empty_cache()

    # the whole analysis over all pairs, and where its time goes
    n = args.analysis_rays
    analyses.ghost_analysis(model, flds=model.fields, wvls=wvls, num_rays=n)       # warm: engines, scratch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g = analyses.ghost_analysis(model, flds=model.fields, wvls=wvls, num_rays=n)
    torch.cuda.synchronize()
    t_all = (time.perf_counter() - t0) * 1e6
    _e, _f, _w, _sw, fs, wis, opts, flags = analyses._packet_items(model, model.fields, wvls, n, True, 'ghost_bench')
    wv = [float(table.wvls[w]) for w in wis]
    split = dict(tables_us=0.0, systems_us=0.0, trace_us=0.0, thinfilm_us=0.0, foci_us=0.0)
    session.clear()                                      # system creation counted: cold engines

    def clock(key, fn):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        split[key] += (time.perf_counter() - t0) * 1e6
        return out

    for pj, pi in g.pairs:
        u = clock('tables_us', lambda: (ghost.unfold(table, pj, pi)))
        c = clock('tables_us', lambda: ghost.coating_tables(table, u, None))
        e = clock('systems_us', lambda: session.engine_for_table(u.table))
        gopts = []
        for o in opts:
            q = abi.Opts.from_buffer_copy(bytes(o))
            q.last_surf = u.table.n_ifcs - 2
            gopts.append(q)
        res = clock('trace_us', lambda: analyses._trace_packets(e, fs, wis, gopts, n))
        rows = clock('thinfilm_us', lambda: e.surface_thinfilm(res, flags, wis, wv, on_device=True, **c)[0])
        clock('foci_us', lambda: e.segment_foci(res, flags, weight=rows))
    r = {'case': args.model, 'analysis': 'ghost_analysis', 'pairs': len(g.pairs), 'items': N_ITEMS, 'rays': n * n,
         'ghost_analysis_us': t_all, 'worst': [[list(g.pairs[p]), fig] for p, fig in g.ranking()[:3]],
         'internal_foci': len(g.internal_foci), **split}
    print(json.dumps(r), flush=True)
    results.append(r)
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(results, fh, indent=1)


if __name__ == '__main__':
    main()
