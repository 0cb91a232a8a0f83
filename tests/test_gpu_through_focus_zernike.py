"""rox_focus_zernike on the device: exact recovery of known coefficients (Fringe 37 and Noll 91,
an off-centre circle, failed rays and OK rays outside the circle); the device's own
through-focus rows of the double Gauss and the .zmx zoom (exact and ROX_FAST_FP64) against the
NumPy restatement (tests/zernike_ref.py, SVD least squares); the double Gauss of
tests/golden/through_focus_mtf.npz against the restatement over the reference's own OPD grids;
bit-identical repeats, host / device destinations and a batch split into several launches;
degenerate planes; analyses.through_focus_zernike against the engine entry and
through_focus_map's RMS wavefront."""
import os

import numpy as np
import pytest

import zernike_ref as ZR
from rayoptics_amd import abi, workloads
from test_gpu_through_focus import fan_opts, golden_wavefronts, make_planes
from test_gpu_through_focus_map import boxes

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'through_focus_mtf.npz')
SPOT = abi.INTERSECT_OBJ | abi.CHECK_APERTURES | abi.APPLY_VIGNETTING


@pytest.fixture(scope='module')
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch


def _engine():
    from rayoptics_amd.engine import TraceEngine
    from rayoptics_amd import SurfaceTable
    tbl = SurfaceTable.from_prescription([dict(cv=0, thi=10.0), dict(cv=0.02, thi=3.0, n=1.5), dict(cv=0, thi=0)])
    return TraceEngine(tbl)


def _grid_tuple(g):
    return (tuple(g.start), tuple(g.stop), g.num)


def _bbox_circles(grids):
    from rayoptics_amd.analyses import zernike_circles
    return zernike_circles(grids, 'bbox', len(grids), 'test')


def synthetic(torch, n_items, K, num, terms, seed, ws=0.5, circle=(0.05, -0.03, 0.9), fail=0.1):
    """rows whose OPD is sum_j c_j Z_j / ws at every ray (NaN rows for failed rays), with known
    c [n_items, K, J]"""
    from rayoptics_amd.engine import FocusRows, make_grid
    from rayoptics_amd.zernike import zernike_eval
    rng = np.random.default_rng(seed)
    J = len(terms)
    R = num * num
    g = make_grid((-1.0, -1.0), (1.0, 1.0), num)
    px, py = ZR.axes(tuple(g.start), tuple(g.stop), num)
    X, Y = np.meshgrid(px, py, indexing='ij')
    x, y = ((X - circle[0]) / circle[2]).reshape(-1), ((Y - circle[1]) / circle[2]).reshape(-1)
    Z = zernike_eval(terms, x, y)                                       # [R, J]
    c = rng.uniform(-1.0, 1.0, (n_items, K, J))
    status = np.where(rng.uniform(size=(n_items, R)) < fail, abi.BLOCKED, abi.OK).astype(np.uint8)
    rows = np.full((n_items, K, 3, R), np.nan)
    rows[:, :, 2] = np.einsum('rj,ikj->ikr', Z, c) / ws
    rows[:, :, 2][np.broadcast_to((status != abi.OK)[:, None], (n_items, K, R))] = np.nan
    fr = FocusRows(torch.from_numpy(rows).cuda(), torch.from_numpy(status).cuda())
    return fr, g, c, rows, status


@pytest.mark.parametrize('basis', ['fringe37', 'noll91'])
def test_synthetic_exact_recovery(torch, basis):
    """known coefficients come back within 1e-12 max(1, max|W|), the residual below 1e-12, and the
    fitted and outside counts are NumPy's exactly"""
    from rayoptics_amd import zernike as Z
    terms = Z.fringe_terms(37) if basis == 'fringe37' else Z.noll_terms(91)
    circle = (0.05, -0.03, 0.9)
    fr, g, c, rows, status = synthetic(torch, 2, 3, 256, terms, seed=1, circle=circle)
    eng = _engine()
    coef, st = eng.focus_zernike(fr, g, terms, 0.5, circle)
    wmax = np.nanmax(np.abs(0.5 * rows[:, :, 2]))
    assert np.all(st['fit'] == 0), st
    assert np.abs(coef - c).max() <= 1e-12 * max(1.0, wmax), np.abs(coef - c).max()
    assert st['rms_residual'].max() <= 1e-12, st['rms_residual']
    px, py = ZR.axes(tuple(g.start), tuple(g.stop), g.num)
    for i in range(2):
        fit, out, _x, _y = ZR.select(status[i], px, py, circle)
        assert (st['n'][i] == fit.sum()).all() and (st['n_outside'][i] == out.sum()).all()
        assert out.sum() > 0 and (status[i] != abi.OK).sum() > 0


def traced(torch, name, n, num, fast=False, seed=0, K=5):
    from rayoptics_amd.engine import TraceEngine
    wl = workloads.load(name)
    eng = TraceEngine(wl.table)
    W = len(wl.table.wvls)
    fl = [wl.fields[i % len(wl.fields)] for i in range(n)]
    wi = [(i // len(wl.fields)) % W for i in range(n)]
    planes = [make_planes(K, golden_wavefronts(), seed=seed + i) for i in range(n)]
    flags = SPOT | (abi.FAST_FP64 if fast else 0)
    opts = [fan_opts(flags, wl.table.n_ifcs) for _ in fl]
    grids = boxes(n, num, seed=seed)
    _stats, fr = eng.trace_pupil_grids_focus(fl, wi, grids, opts, planes, want_rows=True)
    return eng, fr, grids


@pytest.mark.parametrize('name,fast,num', [('dblgauss_c2', False, 64), ('zmx_evenasph_c3', False, 64),
                                           ('zmx_evenasph_c3', True, 64), ('dblgauss_c2', False, 1024),
                                           ('zmx_evenasph_c3', True, 1024)])
def test_traced_rows_against_the_restatement(torch, name, fast, num):
    """the device's own rows: coefficients and residual RMS within 1e-10 max(1, max|W|) of the
    SVD least-squares fit of the same rows on the host; counts exact"""
    from rayoptics_amd import zernike as Z
    n = 3
    eng, fr, grids = traced(torch, name, n, num, fast=fast)
    terms = Z.fringe_terms(37)
    ws = np.array([1700.0, 1900.0, 1500.0])
    circ = _bbox_circles(grids)
    coef, st = eng.focus_zernike(fr, grids, terms, ws, circ)
    rows, status = fr.to_host()
    ec, es = ZR.focus_zernike(rows, status, [_grid_tuple(g) for g in grids], terms, ws, circ)
    assert np.array_equal(st['n'], es['n']) and np.array_equal(st['n_outside'], es['n_outside'])
    assert np.all(st['fit'] == 0), st['fit']
    for i in range(n):
        ok = status[i, :num * num] == abi.OK
        wmax = max(1.0, np.abs(ws[i] * rows[i, :, 2, :num * num][:, ok]).max())
        d = np.abs(coef[i] - ec[i]).max()
        assert d <= 1e-10 * wmax, (i, d, wmax, st['cond'][i])
        dr = np.abs(st['rms_residual'][i] - es['rms_residual'][i]).max()
        assert dr <= 1e-10 * wmax, (i, dr)
        assert np.allclose(st['rms'][i], es['rms'][i], rtol=1e-12, atol=0)


def _fixture_model():
    import focus_map_fixture as FM
    return FM.FocusMapFixtureModel(np.load(GOLDEN), 'dblgauss')


def test_double_gauss_against_the_reference_opd(torch):
    """the device fit of the rows traced from the fixture model equals, within 1e-10 max(1, max|W|),
    the restatement's fit of the reference's own OPD grids over the same pupil grid"""
    from rayoptics_amd import analyses
    m = _fixture_model()
    z = m.z
    n = int(z['ndim'])
    res = analyses.through_focus_zernike(m, m.focs, num_rays=n, circle='bbox', **m.map_kwargs())
    opd = z['opd']                                                        # [F, W, K, n, n] waves
    F, W, K = opd.shape[:3]
    terms = res.terms
    for f in range(F):
        for w in range(W):
            lo, hi = z['bbox'][f, 0], z['bbox'][f, 1]
            grid = (tuple(lo), tuple(hi), n)
            rows = np.zeros((1, K, 3, n * n))
            rows[0, :, 2] = opd[f, w].reshape(K, n * n)
            status = np.where(np.isnan(opd[f, w, 0]).reshape(1, n * n), abi.BLOCKED, abi.OK).astype(np.uint8)
            ec, es = ZR.focus_zernike(rows, status, [grid], terms, [1.0], res.circle[f, w][None])
            assert np.array_equal(res.stats['n'][f, w], es['n'][0]), (f, w)
            wmax = max(1.0, np.nanmax(np.abs(opd[f, w])))
            d = np.abs(res.coef[f, w] - ec[0]).max()
            assert d <= 1e-10 * wmax, (f, w, d)
            assert np.abs(res.stats['rms_residual'][f, w] - es['rms_residual'][0]).max() <= 1e-10 * wmax


def test_determinism_destinations_and_split_launches(torch):
    """repeat calls are bit-identical, host and device destinations identical; a Noll-91 batch of
    20 items x 256 planes, which the scratch bound splits into several launches, equals
    item-by-item calls"""
    from rayoptics_amd import zernike as Z
    from rayoptics_amd.engine import FocusRows, zernike_stats_view
    terms = Z.noll_terms(91)
    fr, g, _c, _rows, _status = synthetic(torch, 20, 256, 64, terms, seed=7)
    eng = _engine()
    ws = np.linspace(0.5, 2.0, 20)
    c1, s1 = eng.focus_zernike(fr, g, terms, ws, (0.05, -0.03, 0.9))
    c2, s2 = eng.focus_zernike(fr, g, terms, ws, (0.05, -0.03, 0.9))
    assert np.array_equal(c1, c2) and s1.tobytes() == s2.tobytes()
    cd, sd = eng.focus_zernike(fr, g, terms, ws, (0.05, -0.03, 0.9), on_device=True)
    assert np.array_equal(c1, cd.cpu().numpy()) and s1.tobytes() == zernike_stats_view(sd).tobytes()
    for i in (0, 7, 15, 19):
        one = FocusRows(fr.rows[i:i + 1], fr.status[i:i + 1])
        ci, si = eng.focus_zernike(one, g, terms, ws[i:i + 1], (0.05, -0.03, 0.9))
        assert np.array_equal(ci[0], c1[i]) and si[0].tobytes() == s1[i].tobytes(), i


def test_degenerate_planes(torch):
    """no ray OK: n = 0, fit 1, NaN; one pupil column OK: fit 2, NaN; neither faults, and the
    other item of the call is fitted"""
    from rayoptics_amd import zernike as Z
    terms = Z.fringe_terms(16)
    fr, g, c, _rows, status = synthetic(torch, 3, 2, 64, terms, seed=3, fail=0.0, circle=(0.0, 0.0, 1.5))
    st = fr.status.cpu().numpy()
    st[0] = abi.BLOCKED
    st[1] = abi.BLOCKED
    st[1, 20 * 64:21 * 64] = abi.OK                                      # one x: one pupil column
    fr.status.copy_(torch.from_numpy(st))
    eng = _engine()
    coef, s = eng.focus_zernike(fr, g, terms, 0.5, (0.0, 0.0, 1.5))
    assert (s['n'][0] == 0).all() and (s['fit'][0] == 1).all() and np.isnan(coef[0]).all()
    assert np.isnan(s['rms_residual'][0]).all() and np.isnan(s['pv_residual'][0]).all()
    assert (s['n'][1] == 64).all() and (s['fit'][1] == 2).all() and np.isnan(coef[1]).all()
    assert np.isnan(s['rms_residual'][1]).all()
    assert (s['fit'][2] == 0).all() and np.abs(coef[2] - c[2]).max() < 1e-11


def test_analysis_against_the_engine_and_the_map(torch):
    """through_focus_zernike equals focus_zernike over the rows trace_pupil_grids_focus returns for
    the same items, bit for bit; with no OK ray outside the circle, stats.rms is
    through_focus_map's opd_rms in waves within 1e-12 relative"""
    from rayoptics_amd import analyses
    m = _fixture_model()
    kw = m.map_kwargs()
    res = analyses.through_focus_zernike(m, m.focs, num_rays=64, circle='bbox', **kw)
    F, W, K = len(m.fields), len(m.wvls), len(m.focs)
    eng, fs, wis, grids, opts_list, planes = analyses._map_items(m, m.fields, m.wvls, m.focs, None, 64, {})
    _s, fr = eng.trace_pupil_grids_focus(fs, wis, grids, opts_list, planes, want_rows=True, want_stats=False)
    scale = [1 / m.nm_to_sys_units(m.wvls[i % W]) for i in range(F * W)]
    coef, st = eng.focus_zernike(fr, grids, res.terms, scale, res.circle.reshape(F * W, 3))
    assert np.array_equal(res.coef, coef.reshape(F, W, K, -1), equal_nan=True)
    assert res.stats.tobytes() == st.reshape(F, W, K).tobytes()
    mp = analyses.through_focus_map(m, m.focs, num_rays=64, **kw)
    wide = analyses.through_focus_zernike(m, m.focs, num_rays=64, n_terms=4, circle=(0.0, 0.0, 10.0), **kw)
    assert (wide.stats['n_outside'] == 0).all() and (wide.stats['n'] == mp.stats['n']).all()
    assert np.allclose(wide.stats['rms'], mp.stats['opd_rms'], rtol=1e-12, atol=0)
    assert res.defocus_zero.shape == (F, W) and res.names[3] == 'defocus'
