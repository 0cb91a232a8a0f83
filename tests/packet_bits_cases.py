"""The calls whose output bits tests/golden/packet_bits.json records, shared by the generator
(tests/golden/make_packet_bits.py) and the test (tests/test_gpu_packet_bits.py): every entry that
walks the FULL packets of finished launches, each call once with host destinations and once with
``on_device=True``.

The packets: the bundled double Gauss, three items of 65 x 65 rays over [-1.05, 1.05]^2 of the
pupil with the apertures checked, so that the rim fails.  4225 rays are 5 tiles of 1024 with a last
tile of 129 rays (two full waves, one wave of one ray, one empty wave), 9 tiles of 512 for
fresnel.hip and 64 cells per row -- two strips -- for solidangle.hip.  One more packet holds a
single ray."""
import contextlib
import hashlib
import os

import numpy as np

from packets_fixture import trace_packets, upload
from rayoptics_amd import abi, workloads

SYSTEM = 'dblgauss_c2'
FLAGS = abi.INTERSECT_OBJ | abi.CHECK_APERTURES | abi.APPLY_VIGNETTING
NUM = 65
SPAN = 1.05
FIELDS, WVLS = [0, 2, 1], [0, 2, 1]         # fields 0 and 2 at the wavelengths 0 and 2, field 1 at 1
ITEM_MAP = [0, 1, 0]                        # three items into two maps
PATHS = ['', 'lds', 'global']               # ROX_WMAPS_PATH
MAP_SLOT = 3                                # a lens surface: the pupil grid lands there as a grid
TILE = 1024                                 # rays of a workgroup of wmaps.hip
LDS_BINS = 4096                             # bins of its LDS window


@contextlib.contextmanager
def forced(path):
    """sets ROX_WMAPS_PATH for the library (read per call) and restores it"""
    saved = os.environ.get('ROX_WMAPS_PATH')
    os.environ['ROX_WMAPS_PATH'] = path
    try:
        yield
    finally:
        if saved is None:
            os.environ.pop('ROX_WMAPS_PATH', None)
        else:
            os.environ['ROX_WMAPS_PATH'] = saved


def _host(a):
    """an output of either destination as a contiguous NumPy array (a tensor's bytes as they are)"""
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, 'cpu') else a)


def make_world(torch):
    """-> (engine, the three packets in HBM, the one-ray packet, the workload's table)"""
    from rayoptics_amd.engine import TraceEngine
    wl = workloads.load(SYSTEM)
    eng = TraceEngine(wl.table)
    res = trace_packets(eng, FLAGS, [wl.fields[f] for f in FIELDS], WVLS, NUM, span=SPAN)
    # the single ray: the centre ray of item 0, copied out and put back as a packet of its own
    h = res[0].to_host(want=('seg', 'status', 'fail_surf'))
    mid = (NUM // 2) * NUM + NUM // 2
    assert int(np.asarray(h.status)[mid]) == abi.OK
    one = upload(eng, np.array(h.seg)[:, :, mid:mid + 1], np.array(h.status)[mid:mid + 1],
                 np.array(h.fail_surf)[mid:mid + 1])
    return eng, res, one, wl.table


def statuses(res):
    """[the status row of every item on the host]"""
    return [np.array(r.to_host(want=('status',)).status) for r in res]


def wide_window(eng, res):
    """a window at MAP_SLOT a tenth of the beam's radius wide, a quarter of the radius off the axis
    in x: the rows of the pupil grid that reach it lie in the middle of the third tile of 1024 rays,
    which so reaches every bin of it -- a box of 80 x 80 bins, over the LDS window
    -> (window, the largest number of bins in the box of one tile)"""
    rec, _m = eng.surface_footprints(res, FLAGS, ok_only=True)
    rad = float(np.sqrt(rec['r2_max'][:, MAP_SLOT].max()))
    cx, h = 0.25 * rad, 0.1 * rad
    window = (cx, 0.0, h, h)
    box = 0
    for r, st in zip(res, statuses(res)):
        seg = np.array(r.to_host(want=('seg',)).seg)
        x, y = seg[MAP_SLOT, 0], seg[MAP_SLOT, 1]
        for t0 in range(0, NUM * NUM, TILE):
            s = slice(t0, t0 + TILE)
            ok = (st[s] == abi.OK) & (np.abs(x[s] - cx) <= h) & (np.abs(y[s]) <= h)
            if ok.any():
                bx = np.minimum(((x[s][ok] - cx + h) / (2 * h) * 80).astype(int), 79)
                by = np.minimum(((y[s][ok] + h) / (2 * h) * 80).astype(int), 79)
                box = max(box, int((bx.max() - bx.min() + 1) * (by.max() - by.min() + 1)))
    return window, box


def run(eng, res, one, table):
    """every call -> {name: array}, in the order the calls are made"""
    from rayoptics_amd import analyses
    from rayoptics_amd.coatings import Coating, stack_tables
    out = {}

    def put(name, arrays, names):
        for n, a in zip(names, arrays):
            if a is not None:
                out[f'{name}/{n}'] = _host(a)

    n_seg = eng.num_segments(FLAGS)
    wvls_nm = [float(table.wvls[w]) for w in WVLS]
    rec, _m = eng.surface_footprints(res, FLAGS, ok_only=True)
    hw = np.sqrt(rec['r2_max'].max(axis=0)) * 0.5           # some rays outside the box
    assert hw.shape == (n_seg,) and np.isfinite(hw).all() and (hw > 0).all()
    kind, value, stacks = analyses._coating_tables(table, Coating.quarter_wave(1.38, 550.0))
    first, thick, index, sub = stack_tables(table, stacks, 'packet_bits')
    fixed_kind = np.where(kind == abi.COAT_STACK, abi.COAT_FIXED, abi.COAT_BARE).astype(np.int32)
    fixed_value = np.tile([0.99, 0.97], (table.n_ifcs, 1))
    assert (fixed_kind == abi.COAT_FIXED).sum() >= 4
    T = eng.surface_transmission(res, FLAGS, WVLS, on_device=True)[0]        # row 0 weighs the rays
    window16 = (0.0, 0.0, float(hw[-1]), float(hw[-1]))
    window80, _box = wide_window(eng, res)

    for dev in (False, True):
        d = 'device' if dev else 'host'
        for partial in (False, True):
            for ok_only in (False, True):
                put(f'footprints/partial{int(partial)}_ok{int(ok_only)}/{d}',
                    eng.surface_footprints(res, FLAGS, partial=partial, ok_only=ok_only, half_width=hw, n_bins=8,
                                           on_device=dev), ('records', 'maps'))
        for fields in (False, True):
            put(f'transmission/bare_fields{int(fields)}/{d}',
                eng.surface_transmission(res, FLAGS, WVLS, fields=fields, on_device=dev), ('rows', 'surf', 'item'))
            put(f'transmission/fixed_fields{int(fields)}/{d}',
                eng.surface_transmission(res, FLAGS, WVLS, coat_kind=fixed_kind, coat_value=fixed_value, fields=fields,
                                         on_device=dev), ('rows', 'surf', 'item'))
        put(f'thinfilm/quarter_wave/{d}',
            eng.surface_thinfilm(res, FLAGS, WVLS, wvls_nm, coat_kind=kind, coat_value=value, stack_first=first,
                                 layer_thickness=thick, layer_index=index, sub_index=sub, on_device=dev),
            ('rows', 'surf', 'item'))
        put(f'solid_angle/plain/{d}', eng.projected_solid_angle(res, NUM, want_cells=True, on_device=dev),
            ('items', 'cells'))
        put(f'solid_angle/weighted/{d}',
            eng.projected_solid_angle(res, NUM, weight=T, want_cells=True, on_device=dev), ('items', 'cells'))
        put(f'segment_foci/plain/{d}', [eng.segment_foci(res, FLAGS, on_device=dev)], ('records',))
        put(f'segment_foci/weighted/{d}', [eng.segment_foci(res, FLAGS, weight=T, on_device=dev)], ('records',))
        put(f'segment_foci/windowed/{d}',
            [eng.segment_foci(res, FLAGS, weight=T, window=(float(hw[-1]), 0.5 * float(hw[-1])), on_device=dev)],
            ('records',))
        for path in PATHS:
            with forced(path):
                for bins, slot, window in ((16, -1, window16), (80, MAP_SLOT, window80)):
                    put(f'weighted_maps/bins{bins}_path_{path or "default"}/{d}',
                        eng.weighted_maps(res, FLAGS, slot=slot, weight=T, item_factor=[1.0, 0.5, 2.0],
                                          item_map=ITEM_MAP, n_maps=2, window=window, bins=bins, want_counts=True,
                                          on_device=dev, raw=True), ('wmaps', 'counts', 'scale_exp', 'item'))
        # the packet of one ray
        T1 = T[:1, :, NUM * NUM // 2:NUM * NUM // 2 + 1].contiguous()
        put(f'one_ray/footprints/{d}',
            eng.surface_footprints(one, FLAGS, half_width=hw, n_bins=8, on_device=dev), ('records', 'maps'))
        put(f'one_ray/transmission/{d}', eng.surface_transmission(one, FLAGS, WVLS[:1], fields=True, on_device=dev),
            ('rows', 'surf', 'item'))
        put(f'one_ray/segment_foci/{d}', [eng.segment_foci(one, FLAGS, weight=T1, on_device=dev)], ('records',))
        put(f'one_ray/weighted_maps/{d}',
            eng.weighted_maps(one, FLAGS, weight=T1, window=window16, bins=16, want_counts=True, on_device=dev,
                              raw=True), ('wmaps', 'counts', 'scale_exp', 'item'))
    return out


def digests(arrays):
    """{name: SHA-256 of the array's bytes}"""
    return {name: hashlib.sha256(a.tobytes()).hexdigest() for name, a in arrays.items()}
