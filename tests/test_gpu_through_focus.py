"""-m gpu: rox_trace_through_focus -- one trace of a pupil grid evaluated at K focus planes.
Its rows must be bit-identical to K ROX_OUT_FAN launches of the same grid with each plane's
foc / image_pt / wf, and to the oracle; its statistics must agree with NumPy on those rows and be
bit-reproducible.  Systems cover every kind of instance the host picks: the lean one (double
Gauss), Newton instances (.zmx even asphere, phone lens), clear-aperture lists, a grating and a
table beyond the LDS (F_GTAB)."""
import ctypes as C

import numpy as np
import pytest

from rayoptics_amd import abi, workloads
from rayoptics_amd.table import field_struct
import helpers as H

pytestmark = pytest.mark.gpu

SPOT = abi.INTERSECT_OBJ | abi.CHECK_APERTURES | abi.APPLY_VIGNETTING
TOL = 1e-10


def golden_wavefronts():
    """real rox_wavefront constants from the golden fixtures: finite and infinite spheres"""
    from rayoptics_amd.table import wavefront_from_array
    out = []
    for name, case in (('dblgauss', 'opd_f0'), ('dblgauss', 'opd_f2'), ('telecentric', 'opd_f0')):
        out.append(wavefront_from_array(H.fixture(name)[case]['wavefront']))
    assert {w.kind for w in out} >= {abi.WF_FINITE, abi.WF_INF_FULL}
    return out


def make_planes(K, wfs, scale=0.05, seed=0):
    """K planes cycling through the given wavefronts (finite and infinite among them, INF_FULL
    and INF_SPLIT both), foc across [-scale, scale], small image-point shifts"""
    rng = np.random.default_rng(seed)
    planes = []
    for k in range(K):
        p = abi.FocusPlane()
        p.foc = float(np.linspace(-scale, scale, K)[k]) if K > 1 else 0.013
        p.image_pt[0], p.image_pt[1] = rng.uniform(-0.02, 0.02, 2)
        p.wf = abi.Wavefront.from_buffer_copy(bytes(wfs[k % len(wfs)]))
        if p.wf.kind != abi.WF_FINITE and k % 2:
            p.wf.kind = abi.WF_INF_SPLIT
        planes.append(p)
    return planes


def fan_opts(flags, N, plane=None):
    from rayoptics_amd.engine import make_opts
    o = make_opts(flags=flags, out_mode=abi.OUT_FAN, first_surf=1, last_surf=N - 2)
    if plane is not None:
        o.foc, o.image_pt[0], o.image_pt[1], o.wf = plane.foc, plane.image_pt[0], plane.image_pt[1], plane.wf
    return o


def k_fan_launches(eng, fld, grid, wi, flags, N, planes):
    rows, status = [], None
    for p in planes:
        r = eng.trace_pupil_grid(fld, grid, wi, fan_opts(flags, N, p), want_pupil=False,
                                 nan_fill=True).to_host(('seg', 'status'))
        rows.append(r.seg)
        status = r.status
    return np.stack(rows), status


def numpy_stats(rows, status):
    """the documented statistics on rows [K, 3, R]"""
    ok = status == abi.OK
    out = []
    for k in range(rows.shape[0]):
        x, y, w = rows[k, 0, ok], rows[k, 1, ok], rows[k, 2, ok]
        if not len(x):
            out.append(None)
            continue
        cx, cy = x.mean(), y.mean()
        out.append(dict(n=len(x), cx=cx, cy=cy,
                        rms_spot=np.sqrt(np.mean((x - cx) ** 2 + (y - cy) ** 2)),
                        rms_spot_image_pt=np.sqrt(np.mean(x ** 2 + y ** 2)),
                        opd_mean=w.mean(), opd_rms=np.sqrt(np.mean((w - w.mean()) ** 2)),
                        opd_min=w.min(), opd_max=w.max()))
    return out


def check_stats(stats, rows, status, what):
    for k, exp in enumerate(numpy_stats(rows, status)):
        if exp is None:
            assert stats['n'][k] == 0 and np.isnan(stats['cx'][k]), what
            continue
        assert stats['n'][k] == exp['n'], (what, k)
        for key, v in exp.items():
            if key == 'n':
                continue
            got = float(stats[key][k])
            assert abs(got - v) <= TOL * max(1.0, abs(v)), f'{what} plane {k} {key}: {got!r} vs {v!r}'


def check_against_fans(eng, fld, grid, wi, flags, N, planes, what, stats_checks=True):
    """one through-focus launch == K FAN launches (rows and status, NaN for failed rays);
    statistics == NumPy on the rows; stats twice bit-identical; stats-only and rows-only calls
    equal the call that asks for both.  Returns the number of rays through."""
    exp_rows, exp_status = k_fan_launches(eng, fld, grid, wi, flags, N, planes)
    opts = fan_opts(flags, N)
    stats, fr = eng.trace_pupil_grid_focus(fld, grid, wi, opts, planes, want_rows=True)
    rows, status = fr.to_host()
    np.testing.assert_array_equal(status, exp_status)
    assert np.array_equal(rows, exp_rows, equal_nan=True), f'{what}: rows differ from {len(planes)} FAN launches'
    if stats_checks:
        check_stats(stats, rows, status, what)
        again = eng.trace_pupil_grid_focus(fld, grid, wi, opts, planes)
        assert again.tobytes() == stats.tobytes(), f'{what}: statistics not reproducible'
        _s, only_rows = eng.trace_pupil_grid_focus(fld, grid, wi, opts, planes, want_rows=True,
                                                   want_stats=False)
        assert _s is None
        assert np.array_equal(only_rows.to_host()[0], rows, equal_nan=True), what
    return int((status == abi.OK).sum())


def _workload_case(name):
    wl = workloads.load(name)
    return wl.table, wl.fields[-1], 1 if len(wl.table.wvls) > 1 else 0


@pytest.mark.parametrize('name', ['dblgauss_c2', 'zmx_evenasph_c3', 'cell_phone', 'rc_telescope_c4'])
@pytest.mark.parametrize('K', [1, 7, 64])
def test_rows_equal_k_fan_launches(name, K):
    """product grids of 77^2 rays (not a multiple of the workgroup) and fans of 1 and 333 rays"""
    from rayoptics_amd.engine import TraceEngine, make_grid
    tbl, fld, wi = _workload_case(name)
    N = tbl.n_ifcs
    eng = TraceEngine(tbl)
    planes = make_planes(K, golden_wavefronts(), seed=K)
    n_ok = check_against_fans(eng, fld, make_grid((-1., -1.), (1., 1.), 77), wi, SPOT, N, planes,
                              f'{name} K={K} grid')
    assert n_ok > 100
    for num in (1, 333):
        fan = make_grid((0., -1.), (0., 1.), num, abi.GRID_FAN)
        check_against_fans(eng, fld, fan, wi, SPOT, N, planes, f'{name} K={K} fan {num}',
                           stats_checks=(K == 7))
    eng.close()


def test_max_planes_and_2_20_rays():
    """K = ROX_MAX_FOCUS_PLANES on a small grid; 2^20 rays with K = 7 (statistics over a million
    rays against NumPy, reproducible)"""
    from rayoptics_amd.engine import TraceEngine, make_grid
    tbl, fld, wi = _workload_case('dblgauss_c2')
    eng = TraceEngine(tbl)
    planes = make_planes(abi.MAX_FOCUS_PLANES, golden_wavefronts(), seed=3)
    check_against_fans(eng, fld, make_grid((-1., -1.), (1., 1.), 24), wi, SPOT, tbl.n_ifcs, planes,
                       'K=max', stats_checks=False)
    planes = make_planes(7, golden_wavefronts(), seed=4)
    n_ok = check_against_fans(eng, fld, make_grid((-1., -1.), (1., 1.), 1024), wi, SPOT, tbl.n_ifcs,
                              planes, '2^20 rays')
    assert n_ok > 500000
    eng.close()


def test_grating_system_and_clear_aperture_lists():
    """a DiffractionGrating system (F_PHASE: the general instance) and clear-aperture lists"""
    from rayoptics_amd.engine import TraceEngine, make_grid
    rng = np.random.default_rng(11)
    tbl, _k = H.phase_table(rng, 'grating')
    fld = field_struct([0.0, 0.0, 0.0], (0., 0.), 2.0, 40.0)
    eng = TraceEngine(tbl)
    planes = make_planes(7, golden_wavefronts(), seed=5)
    check_against_fans(eng, fld, make_grid((-1., -1.), (1., 1.), 45), 1, abi.CHECK_APERTURES,
                       tbl.n_ifcs, planes, 'grating')
    eng.close()
    from test_gpu_r06 import long_chain
    tbl = long_chain(12, rng)           # every ninth lens carries a clear-aperture list
    assert any(r.n_ap for r in tbl.rows)
    fld = field_struct([0.0, -1.0e10 * np.tan(np.deg2rad(0.05)), 0.0], (0., 0.), 9.0, 1.0e10)
    eng = TraceEngine(tbl)
    check_against_fans(eng, fld, make_grid((-1., -1.), (1., 1.), 50), 1, SPOT, tbl.n_ifcs, planes,
                       'clear-aperture lists')
    eng.close()


def test_table_beyond_the_lds():
    """302 interfaces: the general instance over the table in global memory (F_GTAB)"""
    from rayoptics_amd.engine import TraceEngine, make_grid
    from test_gpu_r06 import long_chain
    tbl = long_chain(150, np.random.default_rng(150))
    assert tbl.n_ifcs * 736 > 160 * 1024
    fld = field_struct([0.0, -1.0e10 * np.tan(np.deg2rad(0.05)), 0.0], (0., 0.), 9.0, 1.0e10)
    eng = TraceEngine(tbl)
    planes = make_planes(7, golden_wavefronts(), seed=6)
    n_ok = check_against_fans(eng, fld, make_grid((-1., -1.), (1., 1.), 40), 1, SPOT, tbl.n_ifcs, planes,
                              'F_GTAB')
    assert n_ok > 100
    eng.close()


@pytest.mark.parametrize('name,case', [('dblgauss', 'opd_f2'), ('telecentric', 'opd_f2'),
                                       ('nikkor', 'opd_f1')])
def test_rows_equal_the_oracle(name, case):
    """every plane's rows == an oracle FAN launch, bit-exact (real reference spheres)"""
    from oracle import oracle
    from rayoptics_amd.engine import TraceEngine, make_grid
    from test_oracle_golden import opd_opts
    fx = H.fixture(name)
    c = fx[case]
    fld = H.field_from_arr(c['field'])
    wi = int(c['wvl_idx'])
    o = opd_opts(c)
    planes = make_planes(5, [o.wf], scale=0.1, seed=7)
    eng = TraceEngine(fx.table)
    grid = make_grid((-1., -1.), (1., 1.), 48)
    opts = fan_opts(int(c['flags']) | abi.APPLY_VIGNETTING, fx.table.n_ifcs)
    opts.first_surf, opts.last_surf = int(c['first_surf']), int(c['last_surf'])
    _stats, fr = eng.trace_pupil_grid_focus(fld, grid, wi, opts, planes, want_rows=True)
    rows, status = fr.to_host()
    ogrid = oracle.make_grid((-1., -1.), (1., 1.), 48)
    for k, p in enumerate(planes):
        of = fan_opts(opts.flags, fx.table.n_ifcs, p)
        of.first_surf, of.last_surf = opts.first_surf, opts.last_surf
        orc = oracle.trace_pupil_grid(fx.table, fld, ogrid, wi, of)
        np.testing.assert_array_equal(status, orc.status)
        ok = orc.status == abi.OK
        assert ok.sum() > 100
        H.bit_equal(rows[k][:, ok], orc.seg[0][:, ok] if orc.seg.ndim == 3 else orc.seg[:, ok],
                    f'{name} plane {k}')
    eng.close()


@pytest.mark.parametrize('name', ['dblgauss_c2', 'zmx_evenasph_c3', 'cell_phone'])
def test_tolerance_mode(name):
    """ROX_FAST_FP64: the rows equal K tolerance-mode FAN launches bit for bit, and lie within
    1e-10 max(1, |exact|) of the exact rows.  A ray whose status differs between the two paths
    must sit on a decision boundary: its exact packet (the oracle's) passes within 1e-10 of an
    aperture edge, the critical angle or a grazing miss at the interface where the paths part
    (H.boundary_margin, as test_gpu_fast.py checks its flips)"""
    from oracle import oracle
    from rayoptics_amd.engine import TraceEngine, make_grid, make_opts
    tbl, fld, wi = _workload_case(name)
    N = tbl.n_ifcs
    eng = TraceEngine(tbl)
    planes = make_planes(7, golden_wavefronts(), seed=8)
    grid = make_grid((-1., -1.), (1., 1.), 96)
    check_against_fans(eng, fld, grid, wi, SPOT | abi.FAST_FP64, N, planes, f'{name} fast')
    _s, fe = eng.trace_pupil_grid_focus(fld, grid, wi, fan_opts(SPOT, N), planes, want_rows=True)
    _s, ff = eng.trace_pupil_grid_focus(fld, grid, wi, fan_opts(SPOT | abi.FAST_FP64, N), planes,
                                        want_rows=True)
    (re, se), (rf, sf) = fe.to_host(), ff.to_host()
    flip = se != sf
    if flip.any():
        # where each path stopped (FAN launches report fail_surf), and the exact FULL packets
        fs = [eng.trace_pupil_grid(fld, grid, wi, fan_opts(f, N, planes[0]), want_pupil=False,
                                   nan_fill=True).to_host(('status', 'fail_surf')).fail_surf
              for f in (SPOT, SPOT | abi.FAST_FP64)]
        full = make_opts(flags=SPOT, out_mode=abi.OUT_FULL, first_surf=1, last_surf=N - 2)
        orc = oracle.trace_pupil_grid(tbl, fld, grid, wi, full)
        for r in np.flatnonzero(flip):
            surfs = [int(f[r]) for f in fs if f[r] >= 0]
            assert surfs, (name, r)
            m = H.boundary_margin(tbl, wi, full, orc.seg[:, :, r], min(surfs))
            assert m and min(m.values()) <= TOL, f'{name}: ray {r} changed status off a boundary: {m}'
    ok = ~flip & (se == abi.OK)
    worst = H.scaled_err(re[:, :, ok], rf[:, :, ok])
    assert worst <= TOL, worst
    H.record('through_focus_tolerance_mode', workload=name, worst_scaled_error=worst,
             status_flips=int(flip.sum()))
    eng.close()


def test_argument_errors_with_a_system():
    """a wvl_idx outside the system's wavelengths is rejected (the other argument errors are
    covered without a device in test_through_focus_host.py)"""
    from rayoptics_amd.engine import TraceEngine, make_grid, load_library
    tbl, fld, wi = _workload_case('dblgauss_c2')
    eng = TraceEngine(tbl)
    lib = load_library()
    planes = (abi.FocusPlane * 1)(*make_planes(1, golden_wavefronts()))
    summ = (abi.FocusStats * 1)()
    grid = make_grid((-1., -1.), (1., 1.), 4)
    rc = lib.rox_trace_through_focus(eng._handle, C.byref(fld), C.byref(grid), len(tbl.wvls),
                                     C.byref(fan_opts(SPOT, tbl.n_ifcs)), 1, planes, None, 16, None,
                                     summ, None)
    assert rc == -1 and b'wvl_idx' in lib.rox_last_error()
    eng.close()


@pytest.mark.parametrize('name', ['dblgauss', 'zmx_evenasph_c3'])
def test_python_through_focus_on_the_references_focus_sequence(name):
    """analyses.through_focus end to end on a workloads.TableModel that hands out the reference's
    own reference sphere at each focus (tests/golden/through_focus.npz): at every focus the OPD
    grid equals the reference's focus_wavefront (RayGrid route) and the fan rows its focus_fan,
    bit for bit; the statistics agree with NumPy on the rows; both the RMS spot and the RMS
    wavefront curves have their minimum inside the scan and the best focus of each lies between
    the sampled minimum's neighbours"""
    import focus_fixture as FF
    from rayoptics_amd import analyses
    m = FF.FocusFixtureModel(FF.load(), name)
    focs = np.array(m.focs)
    res = analyses.through_focus(m, m.fields[0], m.wvl, focs, num_rays=13, rows=True)
    assert res.rows.shape == (len(focs), 3, 13 * 13)
    for k in range(len(focs)):
        np.testing.assert_array_equal(res.rows[k, 2], FF.focus_wavefront_rows(m.z['focus_wavefront'][k]))
    check_stats(res.stats, res.rows, res.status, name)
    for curve, best, kind in ((res.rms_spot, res.best_focus_spot, res.best_focus_spot_kind),
                              (res.rms_wavefront, res.best_focus_wavefront, res.best_focus_wavefront_kind)):
        i = int(np.nanargmin(curve))
        assert 0 < i < len(focs) - 1 and kind == 'vertex', (name, curve)
        assert focs[i - 1] <= best <= focs[i + 1]
    assert abs(res.best_focus_spot - res.best_focus_wavefront) < 0.3
    fan = analyses.through_focus(m, m.fields[0], m.wvl, focs, num_rays=15, xy=1, rows=True)
    for k in range(len(focs)):
        assert np.array_equal(fan.rows[k], FF.focus_fan_rows(m.z['focus_fan'][k]), equal_nan=True), k


def test_rows_equal_k_fan_launches_on_the_references_focus_sequence():
    """the fixture's real per-focus planes (foc, image point and sphere of each focus) on a 2^20-ray
    grid: one launch == K FAN launches, statistics as NumPy and reproducible"""
    import focus_fixture as FF
    from rayoptics_amd.engine import TraceEngine, make_grid
    from rayoptics_amd.table import wavefront_from_array
    for name in FF.MODELS:
        m = FF.FocusFixtureModel(FF.load(), name)
        planes = []
        for k, foc in enumerate(m.focs):
            p = abi.FocusPlane()
            p.foc = foc
            p.image_pt[0], p.image_pt[1] = m.z['image_pt'][k]
            p.wf = wavefront_from_array(m.z['wavefront'][k])
            planes.append(p)
        tbl = m.workload.table
        eng = TraceEngine(tbl)
        b = m.z['bbox']
        n_ok = check_against_fans(eng, m.workload.fields[0], make_grid(b[0], b[1], 1024), int(m.z['wvl_idx']),
                                  abi.INTERSECT_OBJ | abi.CHECK_APERTURES, tbl.n_ifcs, planes, name)
        assert n_ok > 1000
        eng.close()
