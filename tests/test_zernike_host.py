"""Zernike fits through focus, host side: the Fringe and Noll tables against the written-out
polynomials; zernike_eval against mpmath closed forms up to n = 20; Noll orthonormality by
quadrature; the ctypes mirrors; every ROX_E_ARG path of rox_focus_zernike (before any device is
touched); ThroughFocusZernike and the zero-crossing rule over an engine double; and the NumPy
restatement's fit of the reference's OPD grids (tests/golden/through_focus_mtf.npz)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import zernike_ref as ZR
from rayoptics_amd import abi
from rayoptics_amd import zernike as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'through_focus_mtf.npz')


@pytest.fixture(scope='module')
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        'rox_build', os.path.join(ROOT, 'ray-optics_amd', 'build.py'))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return abi.declare(C.CDLL(b.build()))


RNG = np.random.default_rng(5)
PTS = RNG.uniform(-0.7, 0.7, (2, 200))


def _polar(x, y):
    return np.hypot(x, y), np.arctan2(y, x)


FRINGE = {   # Z_j(rho, theta), written out
    1: lambda r, t: 1 + 0 * r,
    2: lambda r, t: r * np.cos(t),
    3: lambda r, t: r * np.sin(t),
    4: lambda r, t: 2 * r ** 2 - 1,
    5: lambda r, t: r ** 2 * np.cos(2 * t),
    6: lambda r, t: r ** 2 * np.sin(2 * t),
    7: lambda r, t: (3 * r ** 3 - 2 * r) * np.cos(t),
    8: lambda r, t: (3 * r ** 3 - 2 * r) * np.sin(t),
    9: lambda r, t: 6 * r ** 4 - 6 * r ** 2 + 1,
    10: lambda r, t: r ** 3 * np.cos(3 * t),
    11: lambda r, t: r ** 3 * np.sin(3 * t),
    12: lambda r, t: (4 * r ** 4 - 3 * r ** 2) * np.cos(2 * t),
    13: lambda r, t: (4 * r ** 4 - 3 * r ** 2) * np.sin(2 * t),
    14: lambda r, t: (10 * r ** 5 - 12 * r ** 3 + 3 * r) * np.cos(t),
    15: lambda r, t: (10 * r ** 5 - 12 * r ** 3 + 3 * r) * np.sin(t),
    16: lambda r, t: 20 * r ** 6 - 30 * r ** 4 + 12 * r ** 2 - 1,
    37: lambda r, t: (924 * r ** 12 - 2772 * r ** 10 + 3150 * r ** 8 - 1680 * r ** 6 + 420 * r ** 4
                      - 42 * r ** 2 + 1),
}

NOLL = {
    1: lambda r, t: 1 + 0 * r,
    2: lambda r, t: 2 * r * np.cos(t),
    3: lambda r, t: 2 * r * np.sin(t),
    4: lambda r, t: math.sqrt(3) * (2 * r ** 2 - 1),
    5: lambda r, t: math.sqrt(6) * r ** 2 * np.sin(2 * t),
    6: lambda r, t: math.sqrt(6) * r ** 2 * np.cos(2 * t),
    7: lambda r, t: math.sqrt(8) * (3 * r ** 3 - 2 * r) * np.sin(t),
    8: lambda r, t: math.sqrt(8) * (3 * r ** 3 - 2 * r) * np.cos(t),
    9: lambda r, t: math.sqrt(8) * r ** 3 * np.sin(3 * t),
    10: lambda r, t: math.sqrt(8) * r ** 3 * np.cos(3 * t),
    11: lambda r, t: math.sqrt(5) * (6 * r ** 4 - 6 * r ** 2 + 1),
    22: lambda r, t: math.sqrt(7) * (20 * r ** 6 - 30 * r ** 4 + 12 * r ** 2 - 1),
    37: lambda r, t: 3 * (70 * r ** 8 - 140 * r ** 6 + 90 * r ** 4 - 20 * r ** 2 + 1),
}


@pytest.mark.parametrize('table,terms', [(FRINGE, Z.fringe_terms(37)), (NOLL, Z.noll_terms(91))])
def test_tables_against_the_written_out_polynomials(table, terms):
    x, y = PTS
    r, t = _polar(x, y)
    v = Z.zernike_eval(terms, x, y)
    for j, f in table.items():
        assert np.allclose(v[:, j - 1], f(r, t), rtol=0, atol=1e-12), j


def test_term_lists():
    f = Z.fringe_terms(37)
    assert len(f) == 37 and f[35][:2] == (10, 0) and f[36][:2] == (12, 0) and f[24][:2] == (8, 0)
    n = Z.noll_terms(91)
    assert len(n) == 91 and max(t[0] for t in n) == 12 and len(set((t[0], t[1]) for t in n)) == 91
    assert Z.term_names(f[:9]) == ['piston', 'tilt x', 'tilt y', 'defocus', 'astigmatism 0', 'astigmatism 45',
                                   'coma x', 'coma y', 'spherical']
    with pytest.raises(ValueError):
        Z.fringe_terms(38)
    with pytest.raises(ValueError):
        Z.check_terms([(3, 2, 1.0)])


def test_eval_against_mpmath_up_to_order_20():
    """every (n, m) with n <= 20 against the closed form of R_n^m in mpmath at 50 digits"""
    mp = pytest.importorskip('mpmath')
    mp.mp.dps = 50
    pts = [(0.3, -0.2), (0.61, 0.55), (-0.9, 0.1), (0.0, 0.999), (0.05, 0.02)]
    terms = [(n, m, 1.0) for n in range(21) for m in range(-n, n + 1, 2)]
    for xs, ys in pts:
        got = Z.zernike_eval(terms, xs, ys)
        x, y = mp.mpf(xs), mp.mpf(ys)
        rho, th = mp.sqrt(x * x + y * y), mp.atan2(y, x)
        for j, (n, m, _s) in enumerate(terms):
            mm = abs(m)
            R = sum((-1) ** k * mp.factorial(n - k) / (mp.factorial(k) * mp.factorial((n + mm) // 2 - k)
                                                       * mp.factorial((n - mm) // 2 - k)) * rho ** (n - 2 * k)
                    for k in range((n - mm) // 2 + 1))
            want = R * (1 if m == 0 else mp.cos(m * th) if m > 0 else mp.sin(mm * th))
            assert abs(got[j] - float(want)) <= 2e-10, (n, m, xs, ys, got[j], float(want))


def test_noll_orthonormal_by_quadrature():
    """Gauss-Legendre in rho^2 times a uniform rule in theta: <Z_i Z_j> over the disk is I"""
    terms = Z.noll_terms(91)
    u, wu = np.polynomial.legendre.leggauss(20)
    s = 0.5 * (u + 1)                                   # rho^2 in (0, 1), d(area)/pi = ds dtheta / 2pi
    nt = 64
    th = 2 * np.pi * np.arange(nt) / nt
    rho = np.sqrt(s)
    x = (rho[:, None] * np.cos(th)[None]).reshape(-1)
    y = (rho[:, None] * np.sin(th)[None]).reshape(-1)
    w = (0.5 * wu[:, None] * np.full(nt, 1.0 / nt)[None]).reshape(-1)
    V = Z.zernike_eval(terms, x, y)
    G = V.T @ (w[:, None] * V)
    assert np.abs(G - np.eye(91)).max() < 1e-10


def test_struct_mirrors():
    assert C.sizeof(abi.ZernikeTerm) == 16 and C.sizeof(abi.ZernikeStats) == 56
    from rayoptics_amd.engine import ZERNIKE_STATS_DTYPE
    assert ZERNIKE_STATS_DTYPE.itemsize == 56
    assert 'rox_focus_zernike' in abi.EXPORTS
    assert abi.MAX_ZERNIKE_TERMS == 91 and abi.MAX_ZERNIKE_ORDER == 20


def test_c_argument_errors_without_a_device(lib):
    """every check of rox_focus_zernike comes before it touches a device: each returns ROX_E_ARG
    and names its parameter (and item)"""
    from rayoptics_amd.engine import make_grid
    rows = np.zeros(2 * 3 * 16)
    status = np.zeros(16, dtype=np.uint8)
    coef = np.zeros(2 * 3)
    stats = np.zeros(2 * 56, dtype=np.uint8)
    ws = np.array([1.0])
    circ = np.array([0.0, 0.0, 1.0])

    def grid(**kw):
        g = make_grid((-1, -1), (1, 1), kw.pop('num', 4), kw.pop('kind', abi.GRID_PRODUCT), **kw)
        return (abi.Grid * 1)(g)

    def terms(*nm):
        return (abi.ZernikeTerm * len(nm))(*[abi.ZernikeTerm(n, m, s) for n, m, s in nm])

    good = dict(n_items=1, n_planes=2, rows=rows.ctypes.data, ld=16, status=status.ctypes.data, grids=grid(),
                circle=circ.ctypes.data, wave_scale=ws.ctypes.data, n_terms=3,
                terms=terms((0, 0, 1.0), (1, 1, 1.0), (1, -1, 1.0)), coef=coef.ctypes.data,
                stats=stats.ctypes.data)
    order = list(good)

    def call(**kw):
        a = dict(good, **kw)
        return lib.rox_focus_zernike(*[a[k] for k in order], None), lib.rox_last_error()

    bad_ws = np.array([np.nan])
    cases = [
        (dict(n_items=0), b'n_items'), (dict(n_items=abi.MAX_FOCUS_ITEMS + 1), b'n_items'),
        (dict(n_planes=0), b'n_planes'), (dict(n_planes=abi.MAX_FOCUS_PLANES + 1), b'n_planes'),
        (dict(n_terms=0), b'n_terms'), (dict(n_terms=92), b'n_terms'),
        (dict(rows=None), b'null rows'), (dict(status=None), b'null rows'), (dict(grids=None), b'null rows'),
        (dict(wave_scale=None), b'null rows'), (dict(terms=None), b'null rows'),
        (dict(coef=None, stats=None), b'null coef and stats'),
        (dict(terms=terms((0, 0, 1.0), (2, 1, 1.0), (1, 1, 1.0))), b'terms[1]'),
        (dict(terms=terms((0, 0, 1.0), (21, 1, 1.0), (1, 1, 1.0))), b'terms[1]'),
        (dict(terms=terms((0, 0, 1.0), (1, 3, 1.0), (1, 1, 1.0))), b'terms[1]'),
        (dict(terms=terms((0, 0, 1.0), (1, 1, np.inf), (1, 1, 1.0))), b'terms[1].scale'),
        (dict(grids=grid(kind=abi.GRID_FAN)), b'item 0: grid kind'),
        (dict(grids=grid(row_begin=1, row_count=2)), b'item 0: partial grid'),
        (dict(grids=grid(row_count=2)), b'item 0: partial grid'),
        (dict(grids=grid(num=1)), b'item 0: grid num'),
        (dict(ld=15), b'item 0: ld'),
        (dict(wave_scale=bad_ws.ctypes.data), b'item 0: wave_scale'),
    ]
    for rad in (0.0, -1.0, np.nan, np.inf):
        c = np.array([0.0, 0.0, rad])
        cases.append((dict(circle=c.ctypes.data, _keep=c), b'item 0: circle radius'))
    c = np.array([np.nan, 0.0, 1.0])
    cases.append((dict(circle=c.ctypes.data, _keep=c), b'item 0: circle centre'))
    for kw, name in cases:
        kw = {k: v for k, v in kw.items() if k != '_keep'}
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith(b'rox_focus_zernike') and name in msg, (kw, msg)


# ---- the analysis over an engine double ------------------------------------------------------
def test_zero_crossing_rule():
    from rayoptics_amd.analyses import zero_crossing
    assert zero_crossing([0, 1, 2], [2.0, 1.0, -1.0]) == (1.5, 'crossing')
    assert zero_crossing([0, 1, 2], [2.0, 0.0, -1.0]) == (1.0, 'sample')
    f, k = zero_crossing([0, 1, 2, 3], [-1.0, np.nan, 3.0, 4.0])
    assert k == 'crossing' and f == 0 + (2 - 0) * (-1.0) / (-1.0 - 3.0)
    f, k = zero_crossing([0, 1], [1.0, 2.0])
    assert math.isnan(f) and k == 'none'
    f, k = zero_crossing([0, 1], [np.nan, np.nan])
    assert math.isnan(f) and k == 'none'


class _Rows:
    def __init__(self, rows, status):
        self.rows, self.status = rows, status


class _NumpyZernikeEngine:
    """the device entries through_focus_zernike uses, served on the host: the rows carry the
    reference's OPD grids of through_focus_mtf.npz; focus_zernike is the restatement"""

    def __init__(self, model):
        import torch
        self.torch = torch
        self.model = model
        g = model.z['opd']                                     # [F, W, K, n, n] waves
        F, W, K, n, _n = g.shape
        units = model.z['units_per_nm'] * model.z['wvls']
        rows = np.full((F * W, K, 3, n * n), np.nan)
        rows[:, :, 2] = (g * units[None, :, None, None, None]).reshape(F * W, K, n * n)
        bad = np.isnan(g[:, :, 0]).reshape(F * W, n * n)
        self.rows = rows
        self.status = np.where(bad, abi.BLOCKED, abi.OK).astype(np.uint8)
        self.calls = []

    def trace_pupil_grids_focus(self, flds, wvls, grids, opts_list, planes, want_rows=False, want_stats=True):
        self.calls.append(('trace', len(flds), len(planes[0]), want_rows, want_stats))
        W = len(self.model.wvls)
        items = [self.model.fields.index(f) * W + self.model.wvls.index(float(w)) for f, w in zip(flds, wvls)]
        return None, _Rows(self.rows[items], self.status[items])

    def focus_zernike(self, focus_rows, grids, terms, wave_scale, circle=None, on_device=False):
        from rayoptics_amd.engine import ZERNIKE_STATS_DTYPE
        self.calls.append(('zernike', len(grids), len(terms)))
        coef, st = ZR.focus_zernike(focus_rows.rows, focus_rows.status,
                                    [(tuple(g.start), tuple(g.stop), g.num) for g in grids], terms,
                                    wave_scale, circle)
        out = np.zeros(coef.shape[:2], dtype=ZERNIKE_STATS_DTYPE)
        for k in st:
            out[k] = st[k]
        return coef, out


def _fixture(monkeypatch):
    pytest.importorskip('torch')
    import focus_map_fixture as FM
    from rayoptics_amd import analyses
    m = FM.FocusMapFixtureModel(np.load(GOLDEN), 'dblgauss')
    eng = _NumpyZernikeEngine(m)
    monkeypatch.setattr(analyses, '_launch_setup', lambda _m, fld, wvl, _kw, _mode: (eng, fld, wvl, None))
    return m, eng


def test_result_assembled_from_an_engine_double(monkeypatch):
    """one trace, one fit; coef and stats in [F, W, K] order; the defocus zero crossing per item
    is zero_crossing of its defocus curve and the per-field one is ref_wvl's"""
    from rayoptics_amd import analyses
    m, eng = _fixture(monkeypatch)
    z = m.z
    F, W, K = z['opd'].shape[:3]
    n = int(z['ndim'])
    res = analyses.through_focus_zernike(m, m.focs, num_rays=n, circle='bbox', **m.map_kwargs())
    assert eng.calls == [('trace', F * W, K, True, False), ('zernike', F * W, 37)]
    assert res.coef.shape == (F, W, K, 37) and res.stats.shape == (F, W, K) and res.names[3] == 'defocus'
    assert np.allclose(res.circle[..., :2], 0.5 * (z['bbox'][:, None, 0] + z['bbox'][:, None, 1]))
    ref = m.wvls.index(m.central_wvl)
    for f in range(F):
        for w in range(W):
            assert (res.defocus_zero[f, w], res.defocus_zero_kind[f, w]) == analyses.zero_crossing(
                m.focs, res.coef[f, w, :, 3]) or np.isnan(res.defocus_zero[f, w])
        assert res.defocus_zero_field[f] == res.defocus_zero[f, ref] or np.isnan(res.defocus_zero_field[f])
    with pytest.raises(ValueError):
        analyses.through_focus_zernike(m, m.focs, num_rays=n, circle='disk', **m.map_kwargs())
    with pytest.raises(ValueError):
        analyses.through_focus_zernike(m, m.focs, num_rays=n, terms='legendre', **m.map_kwargs())


def test_restatement_fits_the_reference_grids():
    """the restatement over the reference's OPD grids: the fit reconstructs the wavefront (residual
    RMS <= total RMS), and the defocus term changes through focus"""
    z = np.load(GOLDEN)
    opd = z['dblgauss/opd']
    bbox = z['dblgauss/bbox']
    F, W, K, n, _n = opd.shape
    terms = Z.fringe_terms(37)
    for f in range(F):
        lo, hi = bbox[f, 0], bbox[f, 1]
        circ = np.array([[0.5 * (lo[0] + hi[0]), 0.5 * (lo[1] + hi[1]), 0.5 * max(hi - lo)]])
        for w in range(W):
            rows = np.zeros((1, K, 3, n * n))
            rows[0, :, 2] = opd[f, w].reshape(K, n * n)
            status = np.where(np.isnan(opd[f, w, 0]).reshape(1, n * n), abi.BLOCKED, abi.OK).astype(np.uint8)
            coef, st = ZR.focus_zernike(rows, status, [(tuple(lo), tuple(hi), n)], terms, [1.0], circ)
            assert (st['n'] > 37).all()
            assert (st['rms_residual'] <= st['rms']).all()
            d = coef[0, :, 3]
            assert np.ptp(d) > 1e-3 * np.abs(d).max()
            # reconstruction of the fitted rays
            px, py = ZR.axes(tuple(lo), tuple(hi), n)
            fit, _out, x, y = ZR.select(status[0], px, py, tuple(circ[0]))
            rec = Z.zernike_eval(terms, x[fit], y[fit]) @ coef[0, 0]
            r = rows[0, 0, 2][fit] - rec
            assert abs(np.sqrt((r * r).mean()) - st['rms_residual'][0, 0]) < 1e-10
