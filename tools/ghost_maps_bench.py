#!/usr/bin/env python3
"""The weighted-map pass (rox_weighted_maps, the histogram behind analyses.ghost_analysis(maps=))
on the packets of two double Gauss ghosts -- (7, 3), whose patch is spread over the detector, and
the ghost with the smallest image-side RMS patch among those that land on the detector, which is
concentrated -- 9 (field, wavelength) items into 3 polychromatic maps over an 18 x 12 half-width
detector at the image slot, at num_rays in `--rays` and bins in `--bins`, outputs in HBM.

Timed: the default scatter path and both forced ones (ROX_WMAPS_PATH=lds / global), alternating
within every trial so that drifting clocks and neighbours on the machine hit all three alike; each
trial is a window of `--reps` back-to-back calls between HIP events after a warm-up call of the
same shape, and a figure is the median over `--trials` windows, with the windows' smallest and
largest beside it (`*_us_range`) -- the run-to-run spread the acceptance condition is read
against: `default_ok` says the default's median is no slower than the faster forced path's by
more than the larger relative half-range of the two.  In the same run on the same packets:
rox_surface_footprints' ROX_FP_OK_ONLY count maps (all slots, also given per slot),
rox_segment_foci (weighted), and the host route -- the image slot's x and y rows, the status and
the T row copied to the host, then numpy.histogram2d(weights=) per field (timed once: it takes
seconds at 1024^2).  One JSON object per case.

    python tools/ghost_maps_bench.py [--rays 64 256 1024] [--bins 128 512] [--reps 20] [--trials 7] [--json out.json]

bytes_read is what the two passes of a call must read: the status of every ray twice, of every OK
ray the weight twice and x and y once: 2 + 32*n_ok/R B per ray."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_ITEMS = 9
DETECTOR = (18.0, 12.0)
PATHS = ('default', 'lds', 'global')


def window_us(torch, fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def timed(torch, fn, reps, trials):
    """median and (min, max) of `trials` windows of `reps` calls, after a warm-up call"""
    fn()
    torch.cuda.synchronize()
    w = [window_us(torch, fn, reps) for _ in range(trials)]
    return float(np.median(w)), [float(min(w)), float(max(w))]


def timed_paths(torch, fn, reps, trials):
    """{path: (median, [min, max])} with the three paths alternating inside every trial"""
    w = {p: [] for p in PATHS}
    for p in PATHS:                                       # warm every path
        os.environ['ROX_WMAPS_PATH'] = '' if p == 'default' else p
        fn()
    torch.cuda.synchronize()
    for _ in range(trials):
        for p in PATHS:
            os.environ['ROX_WMAPS_PATH'] = '' if p == 'default' else p
            w[p].append(window_us(torch, fn, reps))
    os.environ.pop('ROX_WMAPS_PATH', None)
    return {p: (float(np.median(v)), [float(min(v)), float(max(v))]) for p, v in w.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rays', nargs='+', type=int, default=[64, 256, 1024])
    ap.add_argument('--bins', nargs='+', type=int, default=[128, 512])
    ap.add_argument('--model', default='dblgauss_c2')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--trials', type=int, default=7)
    ap.add_argument('--json')
    args = ap.parse_args()
    import torch
    import rayoptics_amd  # noqa: F401
    from rayoptics_amd import abi, analyses, ghost, session, workloads
    from rayoptics_amd.engine import SEG_FOCUS_DTYPE, WMAP_ITEM_DTYPE, records_view
    model = workloads.TableModel(args.model)
    table = model.workload.table
    wvls = list(table.wvls)
    F, W = len(model.fields), len(wvls)
    assert F * W == N_ITEMS
    # the concentrated ghost: the smallest image-side patch among the ghosts the detector collects
    g = analyses.ghost_analysis(model, flds=model.fields, wvls=wvls, num_rays=33, detector=DETECTOR)
    share = np.array([analyses._weighted_mean(x, g.spectral_wts) for x in g.in_detector])
    patch = np.where((share > 0.5) & np.isfinite(g.poly_rms_patch), g.poly_rms_patch, np.inf).min(axis=1)
    tight = g.pairs[int(np.argmin(patch))]
    session.clear()
    s = np.asarray(g.spectral_wts, dtype=np.float64)
    kw = dict(slot=-1, weight_row=0, item_factor=np.tile(s / s.sum(), F), item_map=np.repeat(np.arange(F), W), n_maps=F,
              window=(0.0, 0.0) + DETECTOR, on_device=True, raw=True)
    results = []
    for what, (j, i) in (('spread', (7, 3)), ('concentrated', tight)):
        unf = ghost.unfold(table, j, i)
        geng = session.engine_for_table(unf.table)
        ct = ghost.coating_tables(table, unf, None)
        for n in args.rays:
            R = n * n
            _e, _f, _w, _sw, fs, wis, opts, flags = analyses._packet_items(model, model.fields, wvls, n, True,
                                                                           'ghost_maps_bench')
            gopts = []
            for o in opts:
                q = abi.Opts.from_buffer_copy(bytes(o))
                q.last_surf = unf.table.n_ifcs - 2
                gopts.append(q)
            res = analyses._trace_packets(geng, fs, wis, gopts, n)
            rows, _s, _i = geng.surface_thinfilm(res, flags, wis, [float(table.wvls[w]) for w in wis], on_device=True,
                                                 **ct)
            n_seg = geng.num_segments(flags)
            reps = max(2, args.reps // (4 if n >= 1024 else 1))
            t_foci = timed(torch, lambda: geng.segment_foci(res, flags, weight=rows, on_device=True), reps, args.trials)
            rec = records_view(geng.segment_foci(res, flags, weight=rows, on_device=True), SEG_FOCUS_DTYPE)
            rms = float(np.sqrt(np.nanmean(rec['m_aa'][:, -1] / rec['w_sum'][:, -1])))
            for nb in args.bins:
                call = lambda: geng.weighted_maps(res, flags, weight=rows, bins=nb, want_counts=True, **kw)  # noqa: E731
                item = records_view(call()[3], WMAP_ITEM_DTYPE)
                n_ok = int(item['n_in'].sum() + item['n_out'].sum() + item['n_bad'].sum())
                t = timed_paths(torch, call, reps, args.trials)
                hw = np.full(n_seg, DETECTOR[0])
                t_fp = timed(torch, lambda: geng.surface_footprints(res, flags, ok_only=True, half_width=hw, n_bins=nb,
                                                                    on_device=True, want_records=False),
                             max(2, reps // 4), args.trials)
                bytes_read = 2 * N_ITEMS * R + 32 * n_ok
                r = {'case': args.model, 'ghost': what, 'pair': [j, i], 'items': N_ITEMS, 'maps': F, 'rays': R,
                     'bins': [nb, nb], 'n_seg': n_seg, 'n_ok': n_ok, 'n_in': int(item['n_in'].sum()),
                     'image_rms_patch': rms, 'reps': reps, 'trials': args.trials}
                for p in PATHS:
                    r[f'{p}_us'], r[f'{p}_us_range'] = t[p]
                half = lambda p: (t[p][1][1] - t[p][1][0]) / 2 / t[p][0]                         # noqa: E731
                best = min(('lds', 'global'), key=lambda p: t[p][0])
                r['spread_rel'] = max(half('default'), half(best))
                r['default_over_best_forced'] = t['default'][0] / t[best][0]
                r['default_ok'] = bool(r['default_over_best_forced'] <= 1.0 + r['spread_rel'])
                r['bytes_read'] = bytes_read
                r['default_read_gbps'] = bytes_read / (t['default'][0] * 1e-6) / 1e9
                r['footprint_count_maps_us'], r['footprint_count_maps_us_range'] = t_fp
                r['footprint_count_maps_us_per_slot'] = t_fp[0] / n_seg
                r['segment_foci_weighted_us'], r['segment_foci_weighted_us_range'] = t_foci
                # the host route, once
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                xy = [x.seg[-1, 0:2].cpu().numpy() for x in res]
                st = [x.status.cpu().numpy() for x in res]
                T = rows[:, 0, :R].cpu().numpy()
                t_copy = (time.perf_counter() - t0) * 1e6
                t0 = time.perf_counter()
                host = np.zeros((F, nb, nb))
                for k in range(N_ITEMS):
                    ok = (st[k] == abi.OK) & np.isfinite(T[k]) & (T[k] >= 0)
                    h, _xe, _ye = np.histogram2d(xy[k][0][ok], xy[k][1][ok], bins=(nb, nb),
                                                 range=[[-DETECTOR[0], DETECTOR[0]], [-DETECTOR[1], DETECTOR[1]]],
                                                 weights=T[k][ok] * kw['item_factor'][k])
                    host[k // W] += h
                t_numpy = (time.perf_counter() - t0) * 1e6
                wm, _c, e, _it = call()
                dev = np.ldexp(wm.cpu().numpy().astype(np.float64), -e.cpu().numpy()[:, None, None])
                r.update(rows_to_host_us=t_copy, numpy_histogram2d_us=t_numpy,
                         host_route_vs_default=(t_copy + t_numpy) / t['default'][0],
                         max_abs_diff_from_numpy=float(np.abs(dev - host).max()), map_max=float(host.max()))
                print(json.dumps(r), flush=True)
                results.append(r)
            del res, rows
            torch.cuda.empty_cache()
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(results, fh, indent=1)


if __name__ == '__main__':
    main()
