"""-m gpu: rox_trace_through_focus_grids -- n_items through-focus scans in one launch.  Every
item's rows, status and statistics must be bit-identical to its single rox_trace_through_focus
call (itself checked against K ROX_OUT_FAN launches and the oracle in test_gpu_through_focus.py),
across the instance kinds (lean, Newton, clear-aperture lists, grating, a table beyond the LDS),
tolerance mode, item counts, plane counts, a different pupil box per item and fans; a batch large
enough to be split into several launches must give the same statistics; and
analyses.through_focus_map on the stored fixture must equal through_focus and the reference."""
import ctypes as C

import numpy as np
import pytest

from rayoptics_amd import abi, workloads
from rayoptics_amd.table import field_struct
import helpers as H
from test_gpu_through_focus import fan_opts, golden_wavefronts, make_planes

pytestmark = pytest.mark.gpu

SPOT = abi.INTERSECT_OBJ | abi.CHECK_APERTURES | abi.APPLY_VIGNETTING


def boxes(n, num, seed=0, fan=False):
    """n grids of one kind and size, each over its own pupil box (the vignetting boxes of
    trace_wavefront differ per field); a few repeat, so that items share axis slots"""
    from rayoptics_amd.engine import make_grid
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        if i % 4 == 3:
            out.append(out[i - 1])
            continue
        lo, hi = rng.uniform(-1.0, -0.6), rng.uniform(0.6, 1.0)
        if fan:
            out.append(make_grid((0., lo), (0., hi), num, abi.GRID_FAN))
        else:
            out.append(make_grid((lo, rng.uniform(-1.0, -0.6)), (hi, rng.uniform(0.6, 1.0)), num))
    return out


def items_of(flds, n_wvls, n, K, seed):
    """n items cycling over the fields and wavelengths, each with its own K planes"""
    fl = [flds[i % len(flds)] for i in range(n)]
    wi = [(i // len(flds)) % n_wvls for i in range(n)]
    planes = [make_planes(K, golden_wavefronts(), seed=seed + i) for i in range(n)]
    return fl, wi, planes


def check_items(eng, flds, wis, grids, flags, N, planes, what, rows=True):
    """the batched call == one single call per item: rows, status and statistics bit for bit,
    host and device statistics alike, twice the same"""
    opts = [fan_opts(flags, N) for _ in flds]
    if rows:
        stats, fr = eng.trace_pupil_grids_focus(flds, wis, grids, opts, planes, want_rows=True)
        brows, bstatus = fr.to_host()
    else:
        stats = eng.trace_pupil_grids_focus(flds, wis, grids, opts, planes)
    n_ok = 0
    for i in range(len(flds)):
        if rows:
            s, sr = eng.trace_pupil_grid_focus(flds[i], grids[i], wis[i], opts[i], planes[i], want_rows=True)
            r, st = sr.to_host()
            np.testing.assert_array_equal(bstatus[i], st, err_msg=f'{what} item {i}')
            assert np.array_equal(brows[i], r, equal_nan=True), f'{what} item {i}: rows differ'
            n_ok += int((st == abi.OK).sum())
        else:
            s = eng.trace_pupil_grid_focus(flds[i], grids[i], wis[i], opts[i], planes[i])
            n_ok += int(s['n'][0])
        assert stats[i].tobytes() == s.tobytes(), f'{what} item {i}: statistics differ'
    again = eng.trace_pupil_grids_focus(flds, wis, grids, opts, planes)
    assert again.tobytes() == stats.tobytes(), f'{what}: statistics not reproducible'
    return stats, n_ok


def _workload(name):
    wl = workloads.load(name)
    return wl.table, wl.fields, len(wl.table.wvls)


@pytest.mark.parametrize('n', [1, 2, 9, 17, 64])
def test_items_equal_single_calls_lean(n):
    """the lean instance (double Gauss), K = 21, a different box per item"""
    from rayoptics_amd.engine import TraceEngine
    tbl, flds, W = _workload('dblgauss_c2')
    eng = TraceEngine(tbl)
    fl, wi, planes = items_of(flds, W, n, 21, seed=n)
    _s, n_ok = check_items(eng, fl, wi, boxes(n, 40, seed=n), SPOT, tbl.n_ifcs, planes, f'dblgauss n={n}')
    assert n_ok > 100 * n
    eng.close()


@pytest.mark.parametrize('K', [1, 256])
def test_plane_counts(K):
    from rayoptics_amd.engine import TraceEngine
    tbl, flds, W = _workload('dblgauss_c2')
    eng = TraceEngine(tbl)
    fl, wi, planes = items_of(flds, W, 9, K, seed=100 + K)
    check_items(eng, fl, wi, boxes(9, 24 if K > 1 else 77, seed=K), SPOT, tbl.n_ifcs, planes, f'K={K}')
    eng.close()


@pytest.mark.parametrize('name', ['zmx_evenasph_c3', 'cell_phone'])
@pytest.mark.parametrize('fast', [False, True])
def test_newton_instances_and_tolerance_mode(name, fast):
    """Newton instances (.zmx even asphere with clear-aperture lists, phone lens), exact and
    ROX_FAST_FP64; grids and fans"""
    from rayoptics_amd.engine import TraceEngine
    tbl, flds, W = _workload(name)
    eng = TraceEngine(tbl)
    flags = SPOT | (abi.FAST_FP64 if fast else 0)
    fl, wi, planes = items_of(flds, W, 9, 21, seed=7)
    _s, n_ok = check_items(eng, fl, wi, boxes(9, 45, seed=3), flags, tbl.n_ifcs, planes, f'{name} fast={fast}')
    assert n_ok > 1000
    check_items(eng, fl, wi, boxes(9, 333, seed=4, fan=True), flags, tbl.n_ifcs, planes, f'{name} fans')
    eng.close()


def test_grating_aperture_lists_and_a_table_beyond_the_lds():
    from rayoptics_amd.engine import TraceEngine
    from test_gpu_r06 import long_chain
    rng = np.random.default_rng(11)
    tbl, _k = H.phase_table(rng, 'grating')
    fld = field_struct([0.0, 0.0, 0.0], (0., 0.), 2.0, 40.0)
    eng = TraceEngine(tbl)
    fl, wi, planes = items_of([fld], 3, 6, 7, seed=21)
    check_items(eng, fl, wi, boxes(6, 45, seed=5), abi.CHECK_APERTURES, tbl.n_ifcs, planes, 'grating')
    eng.close()
    far = field_struct([0.0, -1.0e10 * np.tan(np.deg2rad(0.05)), 0.0], (0., 0.), 9.0, 1.0e10)
    for n_lenses, what in ((12, 'clear-aperture lists'), (150, 'F_GTAB')):
        tbl = long_chain(n_lenses, np.random.default_rng(n_lenses))
        eng = TraceEngine(tbl)
        fl, wi, planes = items_of([far], 1, 3, 7, seed=n_lenses)
        _s, n_ok = check_items(eng, fl, [0] * 3, boxes(3, 40, seed=6), SPOT, tbl.n_ifcs, planes, what)
        assert n_ok > 100
        eng.close()


def test_device_statistics_and_a_split_batch():
    """statistics into device memory equal those into host memory; 9 items of 2^20 rays at
    K = 256 hold 9 x 75 MB of partial records, more than one launch may: the host splits the
    batch, and every item's statistics still equal its single call's"""
    import torch
    from rayoptics_amd.engine import TraceEngine, load_library, FOCUS_STATS_DTYPE
    tbl, flds, W = _workload('dblgauss_c2')
    eng = TraceEngine(tbl)
    lib = load_library()
    fl, wi, planes = items_of(flds, W, 9, abi.MAX_FOCUS_PLANES, seed=33)
    grids = boxes(9, 1024, seed=8)
    opts = [fan_opts(SPOT, tbl.n_ifcs) for _ in fl]
    host = check_items(eng, fl, wi, grids, SPOT, tbl.n_ifcs, planes, 'split', rows=False)[0]
    K = abi.MAX_FOCUS_PLANES
    dev = torch.empty((9 * K * FOCUS_STATS_DTYPE.itemsize,), dtype=torch.uint8, device=eng.device)
    with torch.cuda.device(eng.device):
        rc = lib.rox_trace_through_focus_grids(
            eng._handle, 9, (abi.Field * 9)(*fl), (C.c_int32 * 9)(*wi), (abi.Grid * 9)(*grids),
            (abi.Opts * 9)(*opts), K, (abi.FocusPlane * (9 * K))(*[p for ps in planes for p in ps]),
            None, 0, None, C.c_void_p(dev.data_ptr()), eng._stream())
        assert rc == 0, lib.rox_last_error()
        torch.cuda.synchronize()
    assert dev.cpu().numpy().tobytes() == host.tobytes()
    assert host['n'].min() > 500000
    eng.close()


@pytest.mark.parametrize('name,case', [('dblgauss', 'opd_f2'), ('nikkor', 'opd_f1')])
def test_rows_equal_the_oracle(name, case):
    """a subset of items, every plane: rows == an oracle FAN launch, bit for bit"""
    from oracle import oracle
    from rayoptics_amd.engine import TraceEngine
    from test_oracle_golden import opd_opts
    fx = H.fixture(name)
    c = fx[case]
    fld = H.field_from_arr(c['field'])
    wi = int(c['wvl_idx'])
    o = opd_opts(c)
    eng = TraceEngine(fx.table)
    grids = boxes(3, 32, seed=9)
    planes = [make_planes(4, [o.wf], scale=0.1, seed=40 + i) for i in range(3)]
    opts = fan_opts(int(c['flags']) | abi.APPLY_VIGNETTING, fx.table.n_ifcs)
    opts.first_surf, opts.last_surf = int(c['first_surf']), int(c['last_surf'])
    _s, fr = eng.trace_pupil_grids_focus([fld] * 3, [wi] * 3, grids, [opts] * 3, planes, want_rows=True)
    rows, status = fr.to_host()
    for i in (0, 2):
        g = grids[i]
        ogrid = oracle.make_grid((g.start[0], g.start[1]), (g.stop[0], g.stop[1]), g.num)
        for k, p in enumerate(planes[i]):
            of = fan_opts(opts.flags, fx.table.n_ifcs, p)
            of.first_surf, of.last_surf = opts.first_surf, opts.last_surf
            orc = oracle.trace_pupil_grid(fx.table, fld, ogrid, wi, of)
            np.testing.assert_array_equal(status[i], orc.status)
            ok = orc.status == abi.OK
            assert ok.sum() > 100
            H.bit_equal(rows[i, k][:, ok], orc.seg[0][:, ok] if orc.seg.ndim == 3 else orc.seg[:, ok],
                        f'{name} item {i} plane {k}')
    eng.close()


def _pooled_poly(m, f, k, ref):
    """the polychromatic statistics of field f at plane k straight from the rows"""
    X, Y, D, S = [], [], [], []
    for w in range(len(m.wvls)):
        ok = m.status[f, w] == abi.OK
        x, y, op = (m.rows[f, w, k, c, ok] for c in range(3))
        X.append(x + m.image_pts[f, w, k, 0])
        Y.append(y + m.image_pts[f, w, k, 1])
        D.append(op - op.mean() if len(op) else op)
        S.append(np.full(len(x), m.spectral_wts[w]))
    X, Y, D, S = map(np.concatenate, (X, Y, D, S))
    N = S.sum()
    cx, cy = (S * X).sum() / N, (S * Y).sum() / N
    return dict(cx=cx, cy=cy, rms_spot=np.sqrt((S * ((X - cx) ** 2 + (Y - cy) ** 2)).sum() / N),
                rms_spot_ref_pt=np.sqrt((S * ((X - m.image_pts[f, ref, k, 0]) ** 2 +
                                              (Y - m.image_pts[f, ref, k, 1]) ** 2)).sum() / N),
                rms_wavefront=np.sqrt((S * D ** 2).sum() / N))


@pytest.mark.parametrize('name', ['dblgauss', 'zmx_evenasph_c3'])
def test_python_map_on_the_fixture(name):
    """analyses.through_focus_map on the fixture's TableModel: stats[f, w] == through_focus bit for
    bit, poly == NumPy on the pooled rows, rows at the stored focus values == the reference's
    focus_wavefront / focus_fan, and best foci inside the scan"""
    import focus_map_fixture as FM
    from rayoptics_amd import analyses
    m = FM.FocusMapFixtureModel(FM.load(), name)
    kw = m.map_kwargs()
    res = analyses.through_focus_map(m, m.focs, num_rays=13, rows=True, **kw)
    F, W, K = len(m.fields), len(m.wvls), len(m.focs)
    assert res.stats.shape == (F, W, K) and res.poly.shape == (F, K)
    for f, fld in enumerate(m.fields):
        for w, wvl in enumerate(m.wvls):
            single = analyses.through_focus(m, fld, wvl, m.focs, num_rays=13, rows=True)
            assert res.stats[f, w].tobytes() == single.stats.tobytes(), (name, f, w)
            assert np.array_equal(res.rows[f, w], single.rows, equal_nan=True)
            assert res.best_focus_spot[f, w] == single.best_focus_spot
            assert res.best_focus_wavefront[f, w] == single.best_focus_wavefront
            for j, k in enumerate(m.ref_focs):
                np.testing.assert_array_equal(res.rows[f, w, k, 2],
                                              m.z['focus_wavefront'][f, w, j][:, :, 2].reshape(-1))
    ref = m.wvls.index(m.central_wvl)
    for f in range(F):
        for k in range(K):
            exp = _pooled_poly(res, f, k, ref)
            for key, v in exp.items():
                assert abs(res.poly[key][f, k] - v) <= 1e-10 * max(1.0, abs(v)), (name, f, k, key)
    assert np.all((res.best_focus_field >= m.focs[0]) & (res.best_focus_field <= m.focs[-1]))
    assert m.focs[0] <= res.best_focus <= m.focs[-1]
    fan = analyses.through_focus_map(m, [m.focs[k] for k in m.ref_focs], num_rays=15, xy=1, rows=True, **kw)
    for f in range(F):
        for w in range(W):
            for j in range(len(m.ref_focs)):
                assert np.array_equal(fan.rows[f, w, j], m.z['focus_fan'][f, w, j][:, 2:5].T,
                                      equal_nan=True), (name, f, w, j)


def _device_stats_call(eng, fld, wi, grid, opts, planes, batched):
    """a stats-only call with its statistics in a device tensor, through the single entry or as a
    one-item batch: the raw bytes of the statistics"""
    import torch
    from rayoptics_amd.engine import load_library, FOCUS_STATS_DTYPE
    lib = load_library()
    K = len(planes)
    dev = torch.zeros((K * FOCUS_STATS_DTYPE.itemsize,), dtype=torch.uint8, device=eng.device)
    p_arr = (abi.FocusPlane * K)(*planes)
    with torch.cuda.device(eng.device):
        if batched:
            rc = lib.rox_trace_through_focus_grids(
                eng._handle, 1, C.byref(fld), (C.c_int32 * 1)(wi), C.byref(grid), C.byref(opts), K, p_arr,
                None, 0, None, C.c_void_p(dev.data_ptr()), eng._stream())
        else:
            rc = lib.rox_trace_through_focus(
                eng._handle, C.byref(fld), C.byref(grid), wi, C.byref(opts), K, p_arr,
                None, 0, None, C.c_void_p(dev.data_ptr()), eng._stream())
        assert rc == 0, lib.rox_last_error()
        torch.cuda.synchronize()
    return dev.cpu().numpy().tobytes()


def test_single_and_batched_calls_share_one_workspace():
    """both entries carve the same per-stream block: a single call of 13 x 13 rays (a partial last
    wave) at K = 3, a batch of 4 items at K = 5 (rows and host statistics) and a stats-only single
    call of 8 x 8 rays at K = 1 into a device tensor give the same rows, status and statistics
    bytes whichever comes first on the engine's stream, and each single call equals item 0 of a
    one-item batch -- rows-only and stats-only calls included"""
    from rayoptics_amd.engine import TraceEngine, make_grid
    tbl, flds, W = _workload('dblgauss_c2')
    N = tbl.n_ifcs
    opts = fan_opts(SPOT, N)
    wfs = golden_wavefronts()
    g13, g8 = make_grid((-1., -1.), (1., 1.), 13), make_grid((-0.9, -0.8), (0.7, 1.), 8)
    p3, p1 = make_planes(3, wfs, seed=61), make_planes(1, wfs, seed=62)
    fl, wi, p5 = items_of(flds, W, 4, 5, seed=63)
    g4 = boxes(4, 21, seed=12)

    def first(eng):
        s, fr = eng.trace_pupil_grid_focus(flds[1], g13, 1, opts, p3, want_rows=True)
        return fr.to_host() + (s.tobytes(),)

    def second(eng):
        s, fr = eng.trace_pupil_grids_focus(fl, wi, g4, [opts] * 4, p5, want_rows=True)
        return fr.to_host() + (s.tobytes(),)

    def third(eng):
        return (_device_stats_call(eng, flds[2], 0, g8, opts, p1, batched=False),)

    def same(a, b, what):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            if isinstance(x, bytes):
                assert x == y, f'{what}: statistics differ'
            else:
                assert np.array_equal(x, y, equal_nan=x.dtype.kind == 'f'), f'{what}: rows or status differ'

    calls = [first, second, third]
    eng = TraceEngine(tbl)
    forward = [c(eng) for c in calls]
    eng.close()
    eng = TraceEngine(tbl)
    backward = [c(eng) for c in reversed(calls)][::-1]
    for i, (a, b) in enumerate(zip(forward, backward)):
        same(a, b, f'call {i + 1} in either order')
    assert int((forward[0][1] == abi.OK).sum()) > 20 and int((forward[1][1] == abi.OK).sum()) > 200

    # ... and the single entry == a batch of one item, on the workspace the calls above left
    s, fr = eng.trace_pupil_grids_focus([flds[1]], [1], [g13], [opts], [p3], want_rows=True)
    r, st = fr.to_host()
    same(forward[0], (r[0], st[0], s[0].tobytes()), 'single call against a one-item batch')
    assert forward[2][0] == _device_stats_call(eng, flds[2], 0, g8, opts, p1, batched=True)
    _n, only_rows = eng.trace_pupil_grid_focus(flds[1], g13, 1, opts, p3, want_rows=True, want_stats=False)
    _n, batch_rows = eng.trace_pupil_grids_focus([flds[1]], [1], [g13], [opts], [p3], want_rows=True,
                                                 want_stats=False)
    assert _n is None
    same(only_rows.to_host(), tuple(x[0] for x in batch_rows.to_host()), 'rows-only call')
    same(only_rows.to_host(), forward[0][:2], 'rows-only call against rows and statistics')
    # the small call's host statistics right behind the batch, whose partial records were larger
    same(second(eng), forward[1], 'the batch once more')
    assert eng.trace_pupil_grid_focus(flds[2], g8, 0, opts, p1).tobytes() == forward[2][0]
    only_stats = eng.trace_pupil_grid_focus(flds[1], g13, 1, opts, p3)
    assert only_stats.tobytes() == forward[0][2]
    assert only_stats.tobytes() == eng.trace_pupil_grids_focus([flds[1]], [1], [g13], [opts], [p3])[0].tobytes()
    eng.close()


def test_argument_errors_with_a_system_leave_the_stream_usable():
    """a wvl_idx outside the system's wavelengths names its item; nothing was enqueued, and the
    next call on the stream gives what it gives on its own"""
    from rayoptics_amd.engine import TraceEngine, load_library
    tbl, flds, W = _workload('dblgauss_c2')
    eng = TraceEngine(tbl)
    lib = load_library()
    fl, wi, planes = items_of(flds, W, 3, 5, seed=50)
    grids = boxes(3, 20, seed=10)
    opts = [fan_opts(SPOT, tbl.n_ifcs) for _ in fl]
    first = eng.trace_pupil_grids_focus(fl, wi, grids, opts, planes)
    summ = (abi.FocusStats * 15)()
    bad = list(wi)
    bad[1] = len(tbl.wvls)
    rc = lib.rox_trace_through_focus_grids(
        eng._handle, 3, (abi.Field * 3)(*fl), (C.c_int32 * 3)(*bad), (abi.Grid * 3)(*grids),
        (abi.Opts * 3)(*opts), 5, (abi.FocusPlane * 15)(*[p for ps in planes for p in ps]),
        None, 0, None, summ, eng._stream())
    assert rc == -1 and b'item 1: wvl_idx' in lib.rox_last_error()
    assert eng.trace_pupil_grids_focus(fl, wi, grids, opts, planes).tobytes() == first.tobytes()
    eng.close()
