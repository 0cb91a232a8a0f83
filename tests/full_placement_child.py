"""Child process of tests/test_gpu_full_placement.py: ROX_FULL_TILE_GROUP, ROX_SMALL_BLOCKS and
ROX_RAYS_PER_LAUNCH are read once per process, so every setting gets a process of its own.

    python tests/full_placement_child.py <dir with the oracle's <case>.npz>

Traces every case into FULL packets at three row pitches over buffers whose row pads hold a
sentinel, compares with the oracle bit for bit and prints one JSON line: {"failures": [...]}."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SENTINEL = -1.2345e300
NUM = 364                       # 364^2 = 132496 rays: 130 tiles of 1024, 518 of 256
WVL = 1
# case -> (fields of the items, pupil rows [row_begin, row_begin + row_count) of grid `num`)
CASES = {
    'ragged': ((2,), 46, 0, 45),            # 45 x 46 rays: 3 tiles, the last one ragged
    'grid': ((2,), NUM, 0, 0),
    'row_block': ((2,), NUM, 100, 37),
    'two_items': ((2, 0), NUM, 0, 0),       # rox_trace_pupil_grids
}


def setup():
    import rayoptics_amd  # noqa: F401
    from rayoptics_amd import abi, workloads
    wl = workloads.load('dblgauss_c2')
    flags = abi.INTERSECT_OBJ | abi.CHECK_APERTURES | abi.APPLY_VIGNETTING
    return wl, flags


def case_args(wl, flags, name, make_grid, make_opts):
    from rayoptics_amd import abi
    fis, num, rb, rc = CASES[name]
    grid = make_grid((-1., -1.), (1., 1.), num, row_begin=rb, row_count=rc)
    opts = make_opts(flags=flags, out_mode=abi.OUT_FULL, first_surf=1, last_surf=wl.n_ifcs - 2)
    return [wl.fields[f] for f in fis], grid, opts


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype.kind != 'f':
        return bool(np.array_equal(a, b))
    nan = np.isnan(a) & np.isnan(b)
    return bool(((a == b) | nan).all() and np.array_equal(np.signbit(a[~nan]), np.signbit(b[~nan])))


def main():
    refdir = sys.argv[1]
    import torch
    from rayoptics_amd import abi
    from rayoptics_amd.engine import TraceEngine, DeviceResult, make_grid, make_opts, grid_rays, load_library
    wl, flags = setup()
    eng = TraceEngine(wl.table, device='cuda:0')
    lib = load_library()
    failures = []
    for name in CASES:
        flds, grid, opts = case_args(wl, flags, name, make_grid, make_opts)
        R = grid_rays(grid)
        refs = [np.load(os.path.join(refdir, f'{name}_{i}.npz')) for i in range(len(flds))]
        for ld in (int(lib.rox_packet_ld(R)), R, R + 1):
            outs = [DeviceResult(torch, eng.device, eng.num_segments(flags), R, abi.OUT_FULL,
                                 want_pupil=True, nan_fill=True, ld=ld) for _ in flds]
            for o in outs:
                o._seg[..., R:] = SENTINEL
                o._pupil[:, R:] = SENTINEL
            if len(flds) == 1:
                eng.trace_pupil_grid(flds[0], grid, WVL, opts, out=outs[0])
            else:
                eng.trace_pupil_grids(flds, [WVL] * len(flds), grid, [opts] * len(flds), outs=outs)
            torch.cuda.synchronize()
            for i, (o, ref) in enumerate(zip(outs, refs)):
                seg, pupil = o._seg.cpu().numpy(), o._pupil.cpu().numpy()
                got = {'seg': seg[..., :R], 'pupil': pupil[:, :R], 'op': o.op.cpu().numpy(),
                       'status': o.status.cpu().numpy(), 'fail_surf': o.fail_surf.cpu().numpy()}
                for key, val in got.items():
                    if not same_bits(val, ref[key]):
                        failures.append(f'{name} item {i} ld {ld}: {key} differs from the oracle')
                if not ((seg[..., R:] == SENTINEL).all() and (pupil[:, R:] == SENTINEL).all()):
                    failures.append(f'{name} item {i} ld {ld}: the row pad was written')
            del outs
    eng.close()
    print(json.dumps({'failures': failures}))


if __name__ == '__main__':
    main()
