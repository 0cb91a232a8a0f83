#!/usr/bin/env python3
"""Thin-film transmission (rox_surface_thinfilm) against the bare entry on the same packets in the
same run, and against what the host would do: DeviceResult.to_host of the FULL packets and the
NumPy restatement (tests/thinfilm_ref.py).  The double Gauss and the .zmx zoom, 9 (field,
wavelength) items at num_rays in `--rays`, outputs in HBM; stacks of `--layers` layers (1.38 / 2.1
alternating, 60 nm each) on every glass-air surface.  Timed as tools/transmission_bench.py does:
HIP events around `--reps` back-to-back calls after a warm-up call of the same shape, the median of
`--trials` windows; the bare entry is timed before and after the stacks so that a drift of the
clocks shows.  Prints one JSON object per case.

    python tools/thinfilm_bench.py [--rays 64 256 1024] [--layers 0 1 4 16] [--json out.json]

layer_gflops counts the arithmetic of the layer loop only, FLOP_PER_LAYER per ray and layer (below),
over the time the call takes beyond the 0-layer call; fp64_share is that over the vector fp64 peak
DESIGN.md quotes (78.6 TFLOP/s).  read_gbps is the bytes the walk must read (6 of a record's 10 rows
of every slot of every OK ray, and status) over the time of the rows-and-records call."""
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
# one layer of one ray in fresnel_kernel<C3, FilmArgs> (csrc/fresnel.hip), a division, a square root, sincos and
# exp counted as one operation each: g = sqrt(N^2 - a2) 10, 1/g 5, the phase 2, sincos 2, exp and
# the scaled cosh / sinh 6, cs and sn 5, the sum of Im delta 1, the p admittance and its reciprocal
# 12, and two characteristic-matrix updates of six complex products and two complex sums each, 80
FLOP_PER_LAYER = 123
FP64_VECTOR_PEAK = 78.6e12


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
    return float(np.median(out)), float(max(out) - min(out))


def glass_air(table):
    """(interface, whether the air comes first) of every glass-air surface"""
    from rayoptics_amd import abi
    nt = np.asarray(table.n_table)
    out = []
    for i in range(1, table.n_ifcs - 1):
        a0, a1 = bool((nt[:, i - 1] == 1.0).all()), bool((nt[:, i] == 1.0).all())
        row = table.rows[i]
        if row.mode == abi.TRANSMIT and a0 != a1 and row.profile != abi.THINLENS and row.ph.kind == abi.PH_NONE:
            out.append((i, a0))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rays', nargs='+', type=int, default=[64, 256, 1024])
    ap.add_argument('--layers', nargs='+', type=int, default=[0, 1, 4, 16])
    ap.add_argument('--models', nargs='+', default=['dblgauss_c2', 'zmx_evenasph_c3'])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--trials', type=int, default=5)
    ap.add_argument('--host-rays', type=int, default=256, help='largest num_rays the host path is timed at')
    ap.add_argument('--json')
    args = ap.parse_args()
    import torch
    import rayoptics_amd  # noqa: F401
    from rayoptics_amd import abi, analyses, coatings, workloads
    from rayoptics_amd.coatings import Coating
    import thinfilm_ref as TR
    results = []
    for name in args.models:
        model = workloads.TableModel(name)
        tbl = model.workload.table
        wvls = list(tbl.wvls)
        assert len(model.fields) * len(wvls) == N_ITEMS
        surfaces = glass_air(tbl)
        for n in args.rays:
            R = n * n
            eng, _f, _w, _sw, fs, wis, opts, flags = analyses._packet_items(model, model.fields, wvls, n, True,
                                                                            'thinfilm_bench')
            res = analyses._trace_packets(eng, fs, wis, opts, n)
            wv = [wvls[w] for w in wis]
            reps = max(1, args.reps // (4 if n >= 1024 else 1))
            bare = lambda **kw: eng.surface_transmission(res, flags, wis, on_device=True, **kw)      # noqa: E731
            _r, surf, item = eng.surface_transmission(res, flags, wis, want_rows=False)
            n_seg, n_ok = int(surf.shape[1]), int(item['n_ok'].sum())
            bytes_read = n_ok * n_seg * 48 + N_ITEMS * R
            r = {'case': name, 'items': N_ITEMS, 'rays': R, 'n_seg': n_seg, 'n_ok': n_ok,
                 'coated_surfaces': len(surfaces), 'bare_mean_T': float(item['t_sum'].sum() / max(n_ok, 1))}
            r['bare_rows_and_records_us'], r['bare_spread_us'] = timed(torch, bare, reps, args.trials)
            r['bare_records_us'], _s = timed(torch, lambda: bare(want_rows=False), reps, args.trials)
            t0_rows = None
            for L in args.layers:
                c = Coating([(1.38 if j % 2 == 0 else 2.1, 60.0) for j in range(L)])
                stacks = {i: c if air else c.reversed() for i, air in surfaces}
                first, thick, index, sub = coatings.stack_tables(tbl, stacks)
                kind = np.zeros(tbl.n_ifcs, np.int32)
                kind[list(stacks)] = abi.COAT_STACK
                kw = dict(coat_kind=kind, coat_value=np.ones((tbl.n_ifcs, 2)), stack_first=first, layer_thickness=thick,
                          layer_index=index, sub_index=sub, on_device=True)
                film = lambda **k: eng.surface_thinfilm(res, flags, wis, wv, **dict(kw, **k))        # noqa: E731
                t_rows, spread = timed(torch, film, reps, args.trials)
                t_rec, _s = timed(torch, lambda: film(want_rows=False), reps, args.trials)
                _r, _s, it = eng.surface_thinfilm(res, flags, wis, wv, want_rows=False, **dict(kw, on_device=False))
                e = {'rows_and_records_us': t_rows, 'spread_us': spread, 'records_us': t_rec,
                     'vs_bare': t_rows / r['bare_rows_and_records_us'],
                     'read_gbps': bytes_read / (t_rows * 1e-6) / 1e9,
                     'mean_T': float(it['t_sum'].sum() / max(n_ok, 1))}
                if L == 0:
                    t0_rows = t_rows
                elif t0_rows is not None and t_rows > t0_rows:
                    flop = float(n_ok) * len(surfaces) * L * FLOP_PER_LAYER
                    e['layer_gflops'] = flop / ((t_rows - t0_rows) * 1e-6) / 1e9
                    e['fp64_share'] = e['layer_gflops'] * 1e9 / FP64_VECTOR_PEAK
                r[f'layers_{L}'] = e
                if L == 4 and n <= args.host_rays:
                    t0 = time.perf_counter()
                    host = [x.to_host(want=('seg', 'status')) for x in res]
                    t_copy = (time.perf_counter() - t0) * 1e6
                    sd = TR.stack_dict(first, thick, index, sub)
                    t0 = time.perf_counter()
                    for h, wi in zip(host, wis):
                        TR.thinfilm(tbl, flags, h.seg, h.status, wi, wvls[wi], kind, kw['coat_value'], sd)
                    t_numpy = (time.perf_counter() - t0) * 1e6
                    r.update(packets_to_host_us=t_copy, numpy_restatement_4_layers_us=t_numpy,
                             host_path_vs_thinfilm_4_layers=(t_copy + t_numpy) / t_rows)
            r['bare_rows_and_records_after_us'], _s = timed(torch, bare, reps, args.trials)
            print(json.dumps(r), flush=True)
            results.append(r)
            del res
            torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as fh:
            json.dump(results, fh, indent=1)
            fh.write('\n')


if __name__ == '__main__':
    main()
