#!/usr/bin/env python3
"""Row pitch of the FULL packet buffer under the shipped kernel: bench.py's step (the pupil
grid of a workload traced into FULL packets, event-timed back-to-back launches as
tools/sustained_probe.py times them) with the packet rows `ld = n rounded up to 4 KiB + pad`
apart, the pads taken in turn, `--rounds` times over.  One JSON line per (round, pad).  The
tile map is the process's (ROX_FULL_TILE_GROUP is read once): one run per group.

    [ROX_FULL_TILE_GROUP=G] python tools/full_placement_sweep.py --pads 0,256,4352 [--rounds 3]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pads', default='', help='comma-separated pads in doubles; empty: the library pitch only')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--launches', type=int, default=500)
    ap.add_argument('--workload', default='dblgauss_c2')
    ap.add_argument('--field', type=int, default=0)
    ap.add_argument('--num', type=int, default=1024)
    ap.add_argument('--batched-fields', default='',
                    help='comma-separated fields: time them as ONE rox_trace_pupil_grids launch at the '
                         'library pitch instead (BASELINE configs[3]: --workload rc_telescope_c4 '
                         '--batched-fields 0,1,2,3,4 --num 256)')
    args = ap.parse_args()
    import torch
    import rayoptics_amd  # noqa: F401
    from rayoptics_amd import abi, workloads
    from rayoptics_amd.engine import TraceEngine, make_opts, make_grid, DeviceResult, padded_ld
    wl = workloads.load(args.workload)
    N = wl.n_ifcs
    eng = TraceEngine(wl.table)
    fld = wl.fields[args.field]
    flags = abi.INTERSECT_OBJ | abi.CHECK_APERTURES | abi.APPLY_VIGNETTING
    if fld.kind == abi.FLD_EPD_WIDE or fld.z_dir0 == 0.0:
        flags &= ~abi.INTERSECT_OBJ
    o = make_opts(flags=flags, out_mode=abi.OUT_FULL, first_surf=1, last_surf=N - 2, foc=wl.foc,
                  image_pt=wl.image_pts[args.field])
    R = args.num * args.num
    grid = make_grid((-1., -1.), (1., 1.), args.num)
    group = os.environ.get('ROX_FULL_TILE_GROUP', '')
    if args.batched_fields:
        batched(args, torch, abi, wl, eng, grid, R, group)
        return
    lds = [(None, padded_ld(R))] if not args.pads else \
        [(int(p), (R + 511) // 512 * 512 + int(p)) for p in args.pads.split(',')]
    for rnd in range(args.rounds):
        for pad, ld in lds:
            out = DeviceResult(torch, eng.device, eng.num_segments(flags), R, abi.OUT_FULL,
                               want_pupil=True, nan_fill=False, ld=ld)
            eng.time_pupil_grid(fld, grid, wl.ref_wvl_idx, o, out, 400)     # clocks, first touch
            ms = eng.time_pupil_grid(fld, grid, wl.ref_wvl_idx, o, out, args.launches)
            print(json.dumps({'workload': args.workload, 'num': args.num, 'group': group, 'round': rnd,
                              'pad': pad, 'ld': ld, 'us': round(ms * 1e3, 2)}), flush=True)
            del out
            torch.cuda.empty_cache()


def batched(args, torch, abi, wl, eng, grid, R, group):
    """bench.py's configs leg for one configuration: every field's grid in one launch, median of
    5 event-timed batches of 50 passes after 0.1 s of untimed ones"""
    import time
    from rayoptics_amd.engine import make_opts, DeviceResult
    N = wl.n_ifcs
    fis = [int(f) for f in args.batched_fields.split(',')]
    base = abi.CHECK_APERTURES | abi.APPLY_VIGNETTING
    wide = [abi.INTERSECT_OBJ if (f.kind != abi.FLD_EPD_WIDE and f.z_dir0 != 0.0) else 0 for f in wl.fields]
    ress = [DeviceResult(torch, eng.device, eng.num_segments(0), R, abi.OUT_FULL, want_pupil=True,
                         nan_fill=False) for _ in fis]
    optl = [make_opts(flags=base | wide[f], out_mode=abi.OUT_FULL, first_surf=1, last_surf=N - 2,
                      foc=wl.foc, image_pt=wl.image_pts[f]) for f in fis]
    fldl = [wl.fields[f] for f in fis]
    wvll = [wl.ref_wvl_idx for _ in fis]
    for rnd in range(args.rounds):
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.1:
            for _ in range(16):
                eng.trace_pupil_grids(fldl, wvll, grid, optl, outs=ress)
            torch.cuda.synchronize()
        ts = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(50):
                eng.trace_pupil_grids(fldl, wvll, grid, optl, outs=ress)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / 50)
        print(json.dumps({'workload': args.workload, 'num': args.num, 'group': group, 'round': rnd,
                          'grids_in_one_launch': len(fis), 'ld': ress[0].ld,
                          'us': round(sorted(ts)[2] * 1e3, 2)}), flush=True)


if __name__ == '__main__':
    main()
