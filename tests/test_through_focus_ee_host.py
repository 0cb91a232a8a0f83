"""CPU-side checks of the encircled energy through focus (rox_focus_ee, rox_focus_psf_ee,
analyses.through_focus_ee): the NumPy restatement's own invariants (tests/ee_ref.py), the
restatement on a perfect circular pupil against the Airy encircled energy, the polychromatic
merges on synthetic input, argument errors (C and Python) without a device, and the result
assembled from an engine double over tests/golden/through_focus_ee.npz and
tests/golden/through_focus_mtf.npz."""
import ctypes as C
import os

import numpy as np
import pytest

import ee_ref as ER
import line_otf as LO
from rayoptics_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')


@pytest.fixture(scope='module')
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        'rox_build', os.path.join(ROOT, 'ray-optics_amd', 'build.py'))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return abi.declare(C.CDLL(b.build()))


# ---- the restatement ----------------------------------------------------------------------------
def test_restatement_invariants():
    rng = np.random.default_rng(3)
    R = 1000
    x, y = rng.normal(size=R), rng.normal(size=R) * 0.5
    ok = rng.random(R) > 0.1
    n = int(ok.sum())
    d = np.sqrt((x[ok] - 0.1) ** 2 + (y[ok] + 0.2) ** 2)
    radii = np.sort(rng.uniform(0, 3, 40))
    fr = np.array([1e-9, 0.1, 0.5, 0.8, 0.999, 1.0])
    counts, rad, nn = ER.plane_ee(x, y, ok, (0.1, -0.2), radii, fr)
    assert nn == n and (np.diff(counts) >= 0).all() and counts[-1] <= n
    assert rad[-1] == np.sqrt(ER.d2_of(x[ok], y[ok], 0.1, -0.2).max())          # fraction 1: the farthest
    assert rad[0] == np.sqrt(ER.d2_of(x[ok], y[ok], 0.1, -0.2).min())           # rank 1: the nearest
    for q, f in enumerate(fr):
        m = ER.rank_of(f, n)
        # the m-th smallest: at least m rays within it, fewer than m strictly inside
        assert (d <= rad[q] * (1 + 1e-15)).sum() >= m and (d < rad[q] * (1 - 1e-15)).sum() < m
    assert ER.rank_of(0.5, 7) == 4 and ER.rank_of(1e-12, 7) == 1 and ER.rank_of(1.0, 7) == 7
    # no ray: zero counts, NaN radii; ties: every ray on one point
    c0, r0, n0 = ER.plane_ee(x, y, np.zeros(R, bool), None, radii, fr)
    assert n0 == 0 and (c0 == 0).all() and np.isnan(r0).all()
    c1, r1, _n = ER.plane_ee(np.full(9, 2.0), np.full(9, -1.0), np.ones(9, bool), (2.0, -1.0), [0.0, 1.0], fr)
    assert list(c1) == [9, 9] and (r1 == 0.0).all()


def test_psf_restatement_full_coverage_and_centroid():
    rng = np.random.default_rng(4)
    M, p = 32, 1e-3
    psf = rng.random((M, M))
    big = p * M * 2
    ee = ER.psf_ee(psf, p, None, [0.0, big])
    assert ee[-1] == pytest.approx(1.0, abs=1e-15)
    c = ER.psf_centroid(psf, p)
    assert np.allclose(c, LO.psf_centroid(psf, p), rtol=0, atol=1e-15)
    assert np.isnan(ER.psf_ee(np.zeros((M, M)), p, None, [big])).all()
    # a single lit pixel: all of it within radius 0 of itself
    one = np.zeros((M, M))
    one[5, 20] = 2.0
    c = ER.psf_centroid(one, p)
    assert np.allclose(c, [-p * (5 - M // 2), -p * (20 - M // 2)], rtol=0, atol=1e-18)
    assert ER.psf_ee(one, p, None, [0.0])[0] == 1.0


def test_airy_encircled_energy():
    """the restatement on calc_psf of a perfect circular pupil (64 samples across, maxdim 512):
    EE(r) = 1 - J0(pi r)^2 - J1(pi r)^2 with r in lambda / D units, the pixel pitch being
    ndim / maxdim of them, within the sampling error of pixel-centre binning (largest on the
    steep core, 0.125 lambda / D pixels)"""
    special = pytest.importorskip('scipy.special')
    ndim, M = 64, 512
    u = (np.arange(ndim) - (ndim - 1) / 2) / (ndim / 2)
    # a constant piston (calc_psf zeroes the samples whose phase is exactly 1, its padding)
    opd = np.where(u[:, None] ** 2 + u[None, :] ** 2 <= 1.0, 0.25, np.nan)
    psf = LO.numpy_calc_psf(opd, ndim, M)
    p = ndim / M
    # calc_psf's grid puts the pupil centre half a sample off the array centre: about the centroid
    r = np.array([0.5, 1.0, 1.22, 1.7, 2.23, 3.0, 5.0, 10.0])
    got = ER.psf_ee(psf, p, None, r)
    v = np.pi * r
    airy = 1 - special.j0(v) ** 2 - special.j1(v) ** 2
    assert abs(got[0] - airy[0]) < 0.02 and np.max(np.abs(got[1:] - airy[1:])) < 0.005, (got, airy)
    assert ER.psf_ee(psf, p, None, [p * M])[0] == 1.0


def test_poly_merges_on_synthetic_input():
    from rayoptics_amd import analyses
    rng = np.random.default_rng(5)
    F, W, K, N = 2, 3, 4, 6
    counts = rng.integers(0, 100, size=(F, W, K, N)).cumsum(axis=-1)
    n_ok = counts[..., -1] + rng.integers(0, 10, size=(F, W, K))
    n_ok[0, 1, 2] = 0
    counts[0, 1, 2] = 0
    s = np.array([0.5, 1.0, 2.0])
    got = analyses._poly_counts(counts, n_ok, s)
    for f in range(F):
        exp = ER.poly_counts_ee(counts[f], n_ok[f], s)
        assert np.allclose(got[f], exp, rtol=1e-15, atol=0)
    assert got[0, 2, 0] == (s * counts[0, :, 2, 0]).sum() / (s * n_ok[0, :, 2]).sum()
    # one wavelength: its own fraction
    one = analyses._poly_counts(counts[:, :1], n_ok[:, :1], s[:1])
    assert np.allclose(one, counts[:, 0] / n_ok[:, 0, :, None], rtol=1e-15)
    # diffraction: weighted mean of unit-energy curves, NaN curves skipped
    ee = rng.random((F, W, K, N))
    ee[1, 2, 3] = np.nan
    got = analyses._poly_psf(ee, s)
    assert np.allclose(got[0], ER.poly_psf_ee(ee[0], s), rtol=1e-15)
    assert np.allclose(got[1, 3], (s[:2, None] * ee[1, :2, 3]).sum(axis=0) / s[:2].sum(), rtol=1e-15)
    assert np.isnan(analyses._poly_psf(np.full((1, 2, 1, 3), np.nan), s[:2])).all()
    # polychromatic centroid: sum_w s_w (image_pt_w + c_w) / sum_w s_w
    ip = rng.normal(size=(W, K, 2))
    c = rng.normal(size=(W, K, 2))
    ok = np.ones((W, K), bool)
    ok[1, 0] = False
    C = analyses.poly_centroid(c, ip, s, ok)
    w = np.where(ok, s[:, None], 0.0)
    assert np.allclose(C, (w[..., None] * (ip + c)).sum(axis=0) / w.sum(axis=0)[:, None], rtol=1e-15)
    # the curve's radius
    r = np.linspace(0, 1, 5)
    e = np.array([0.0, 0.3, 0.6, 0.9, 1.0])
    assert analyses.curve_radius(r, e, 0.45) == pytest.approx(0.375)
    assert analyses.curve_radius(r, e, 1.0) == 1.0 and analyses.curve_radius(r, e, 0.0) == 0.0
    assert np.isnan(analyses.curve_radius(r, e * 0.5, 0.8)) and ER.curve_radius(r, e, 0.45) == pytest.approx(0.375)


def test_best_focus_is_the_smallest_radius():
    from rayoptics_amd import analyses
    K, F, n = 9, 2, 64
    focs = np.linspace(-0.02, 0.02, K)
    peaks = np.array([0.004, -0.006])
    curve_radii = np.broadcast_to(np.linspace(0, 1, n), (F, K, n)).copy()
    poly = np.empty((F, K, n))
    for f in range(F):
        for k in range(K):
            scale = 0.1 + ((focs[k] - peaks[f]) / 0.02) ** 2            # EE radius ~ scale
            poly[f, k] = np.clip(curve_radii[f, k] / scale, 0, 1)
    r = analyses.ThroughFocusEE(focs, [0.5, 1.0], None, [500.0], [1.0, 3.0], [1.0], 500.0, 'geometric',
                                np.zeros((F, 1, K, 2)), np.zeros((F, 1, K, 2)), np.zeros((F, 1, K, 2)), None,
                                curve_radii, poly, None, n_ok=np.ones((F, 1, K)))
    assert r.poly_ee_radius.shape == (F, K, 2) and (r.best_focus_kind == 'vertex').all()
    assert np.all(np.abs(r.best_focus - peaks[:, None]) < 2e-3)
    for q in range(2):
        assert (r.best_focus_all[q], r.best_focus_all_kind[q]) == analyses.overall_best_focus(
            focs, r.poly_ee_radius[:, :, q], [1.0, 3.0])


def test_python_argument_errors_before_any_launch():
    from rayoptics_amd import analyses
    model = object()
    for bad in ([0.0], [1.5], [np.nan], [], np.full(abi.MAX_EE_FRACTIONS + 1, 0.5)):
        with pytest.raises(ValueError, match='fraction'):
            analyses.through_focus_ee(model, [0.0], fractions=bad)
    for bad in ([-1.0], [0.2, 0.1], [np.inf], np.ones(abi.MAX_EE_RADII + 1)):
        with pytest.raises(ValueError, match='radii'):
            analyses.through_focus_ee(model, [0.0], radii=bad)
    with pytest.raises(ValueError, match='kind'):
        analyses.through_focus_ee(model, [0.0], kind='wave')
    with pytest.raises(ValueError, match='even'):
        analyses.through_focus_ee(model, [0.0], kind='diffraction', num_rays=31)
    with pytest.raises(ValueError, match='2 num_rays'):
        analyses.through_focus_ee(model, [0.0], kind='diffraction', num_rays=32, maxdim=48)
    with pytest.raises(ValueError, match='n_curve'):
        analyses.through_focus_ee(model, [0.0], n_curve=1)
    with pytest.raises(ValueError, match='focus values'):
        analyses.through_focus_ee(model, [])


def test_c_argument_errors_without_a_device(lib):
    """every check of rox_focus_ee and rox_focus_psf_ee comes before it touches a device: each
    returns ROX_E_ARG and names its parameter"""
    rows = np.zeros(2 * 3 * 8)
    status = np.zeros(8, dtype=np.uint8)
    radii = np.tile([0.0, 0.5, 1.0], 2)
    fr = np.array([0.5, 0.8])
    counts = np.zeros(2 * 3, dtype=np.int64)
    eer = np.zeros(2 * 2)
    nok = np.zeros(2, dtype=np.int64)
    cen = np.zeros(4)
    RW, ST, RA, FR, CO, ER_, NO, CE = (rows.ctypes.data, status.ctypes.data, radii.ctypes.data, fr.ctypes.data,
                                       counts.ctypes.data, eer.ctypes.data, nok.ctypes.data, cen.ctypes.data)
    dec = np.array([0.0, 0.5, 0.4, 0.0, 0.5, 1.0])
    neg = np.array([0.0, 0.5, 1.0, -1.0, 0.5, 1.0])
    nan_r = np.array([0.0, 0.5, 1.0, 0.0, np.nan, 1.0])
    bad_f0 = np.array([0.0, 0.8])
    bad_f1 = np.array([0.5, 1.5])
    bad_c = np.array([0.0, np.inf, 0.0, 0.0])
    ok = (1, 2, RW, 8, ST, 8, CE, 3, RA, CO, 2, FR, ER_, NO)

    def w(**kw):
        names = ('n_items', 'n_planes', 'rows', 'ld', 'status', 'n_rays', 'centers', 'n_radii', 'radii', 'counts',
                 'n_frac', 'fractions', 'ee_radius', 'n_ok')
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return tuple(a)
    cases = [(w(n_items=0), b'n_items'), (w(n_items=abi.MAX_FOCUS_ITEMS + 1), b'n_items'),
             (w(n_planes=0), b'n_planes'), (w(n_planes=abi.MAX_FOCUS_PLANES + 1), b'n_planes'),
             (w(rows=None), b'rows'), (w(status=None), b'status'),
             (w(n_rays=0), b'n_rays'), (w(n_rays=9), b'n_rays'),
             (w(n_radii=-1), b'n_radii'), (w(n_radii=abi.MAX_EE_RADII + 1), b'n_radii'),
             (w(n_frac=-1), b'n_frac'), (w(n_frac=abi.MAX_EE_FRACTIONS + 1), b'n_frac'),
             (w(counts=None, ee_radius=None), b'counts and ee_radius'),
             (w(n_radii=0), b'n_radii'), (w(radii=None), b'radii'),
             (w(n_frac=0), b'n_frac'), (w(fractions=None), b'fractions'),
             (w(radii=dec.ctypes.data), b'radii[2]'), (w(radii=neg.ctypes.data), b'radii[3]'),
             (w(radii=nan_r.ctypes.data), b'radii[4]'),
             (w(fractions=bad_f0.ctypes.data), b'fractions[0]'), (w(fractions=bad_f1.ctypes.data), b'fractions[1]'),
             (w(centers=bad_c.ctypes.data), b'centers[1]')]
    for args, name in cases:
        assert lib.rox_focus_ee(*args, None) == -1, args
        msg = lib.rox_last_error()
        assert msg.startswith(b'rox_focus_ee') and name in msg, (args, msg)

    psf = np.zeros(2 * 16 * 16)
    pitch = np.full(2, 1e-3)
    ee = np.zeros(2 * 3)
    P, PI, E = psf.ctypes.data, pitch.ctypes.data, ee.ctypes.data
    bad_p = np.array([1e-3, 0.0])
    nan_p = np.array([np.nan, 1e-3])
    pcases = [((0, 2, P, 16, PI, None, 3, RA, E, None), b'n_items'),
              ((abi.MAX_FOCUS_ITEMS + 1, 2, P, 16, PI, None, 3, RA, E, None), b'n_items'),
              ((1, 0, P, 16, PI, None, 3, RA, E, None), b'n_planes'),
              ((1, abi.MAX_FOCUS_PLANES + 1, P, 16, PI, None, 3, RA, E, None), b'n_planes'),
              ((1, 2, P, 1, PI, None, 3, RA, E, None), b'maxdim'),
              ((1, 2, P, 32769, PI, None, 3, RA, E, None), b'maxdim'),
              ((1, 2, P, 16, PI, None, 0, RA, E, None), b'n_radii'),
              ((1, 2, P, 16, PI, None, abi.MAX_EE_RADII + 1, RA, E, None), b'n_radii'),
              ((1, 2, None, 16, PI, None, 3, RA, E, None), b'psf'),
              ((1, 2, P, 16, None, None, 3, RA, E, None), b'pitch'),
              ((1, 2, P, 16, PI, None, 3, None, E, None), b'radii'),
              ((1, 2, P, 16, PI, None, 3, RA, None, None), b'ee'),
              ((1, 2, P, 16, bad_p.ctypes.data, None, 3, RA, E, None), b'pitch[1]'),
              ((1, 2, P, 16, nan_p.ctypes.data, None, 3, RA, E, None), b'pitch[0]'),
              ((1, 2, P, 16, PI, None, 3, dec.ctypes.data, E, None), b'radii[2]'),
              ((1, 2, P, 16, PI, None, 3, nan_r.ctypes.data, E, None), b'radii[4]'),
              ((1, 2, P, 16, PI, bad_c.ctypes.data, 3, RA, E, None), b'centers[1]')]
    for args, name in pcases:
        assert lib.rox_focus_psf_ee(*args, None) == -1, args
        msg = lib.rox_last_error()
        assert msg.startswith(b'rox_focus_psf_ee') and name in msg, (args, msg)
    assert {'rox_focus_ee', 'rox_focus_psf_ee'} <= set(abi.EXPORTS)
    assert abi.MAX_EE_RADII == 1024 and abi.MAX_EE_FRACTIONS == 64


# ---- the analysis over an engine double --------------------------------------------------
class _Rows:
    def __init__(self, rows, status):
        self.rows, self.status = rows, status


def focus_stats(rows, ok):
    """FOCUS_STATS_DTYPE [n_items, K] of host rows (n, centroid, rms spot; OPD fields 0)"""
    from rayoptics_amd.engine import FOCUS_STATS_DTYPE
    n_items, K = rows.shape[:2]
    st = np.zeros((n_items, K), dtype=FOCUS_STATS_DTYPE)
    for i in range(n_items):
        for k in range(K):
            x, y = rows[i, k, 0, ok[i]], rows[i, k, 1, ok[i]]
            st['n'][i, k] = x.size
            st['cx'][i, k], st['cy'][i, k] = (x.mean(), y.mean()) if x.size else (np.nan, np.nan)
            st['rms_spot'][i, k] = np.sqrt(((x - x.mean()) ** 2 + (y - y.mean()) ** 2).mean()) if x.size else np.nan
    return st


class _NumpyEeEngine:
    """the device entries through_focus_ee uses, served on the host: the rows carry the
    reference's transverse aberrations of tests/golden/through_focus_ee.npz (geometric) or its OPD
    grids of through_focus_mtf.npz (diffraction); focus_ee / focus_psf_ee are the restatement"""

    def __init__(self, model, opd=False):
        import torch
        self.torch = torch
        self.model = model
        z = model.z
        if opd:
            g = z['opd']                                       # [F, W, K, n, n] waves
            F, W, K, n, _n = g.shape
            units = z['units_per_nm'] * z['wvls']
            rows = np.full((F * W, K, 3, n * n), np.nan)
            rows[:, :, 2] = (g * units[None, :, None, None, None]).reshape(F * W, K, n * n)
            bad = np.isnan(g[:, :, 0]).reshape(F * W, n * n)
        else:
            a = z['abr']                                       # [F, W, K, n, n, 2]
            F, W, K, n, _n, _two = a.shape
            rows = np.zeros((F * W, K, 3, n * n))
            rows[:, :, :2] = np.moveaxis(a.reshape(F * W, K, n * n, 2), -1, 2)
            bad = np.isnan(a[:, :, 0, ..., 0]).reshape(F * W, n * n)
            rows[:, :, :2][np.broadcast_to(bad[:, None, None], rows[:, :, :2].shape)] = 0.0
        self.rows = rows
        self.status = np.where(bad, abi.BLOCKED, abi.OK).astype(np.uint8)
        self.calls = []

    def trace_pupil_grids_focus(self, flds, wvls, grids, opts_list, planes, want_rows=False, want_stats=True):
        """(the double's _launch_setup hands out the field and wavelength as they came)"""
        self.calls.append(('trace', len(flds), len(planes[0]), want_rows, want_stats))
        W = len(self.model.wvls)
        items = [self.model.fields.index(f) * W + self.model.wvls.index(float(w)) for f, w in zip(flds, wvls)]
        rows, status = np.ascontiguousarray(self.rows[items]), np.ascontiguousarray(self.status[items])
        fr = _Rows(self.torch.from_numpy(rows), self.torch.from_numpy(status))
        return (focus_stats(rows, status == abi.OK) if want_stats else None), fr

    def focus_ee(self, focus_rows, n_rays, centers, radii, fractions, on_device=False):
        self.calls.append(('ee', None if radii is None else np.shape(radii)[-1],
                           None if fractions is None else len(fractions)))
        rows, status = focus_rows.rows.numpy(), focus_rows.status.numpy()
        n_items, K = rows.shape[:2]
        c = np.broadcast_to(centers, (n_items, K, 2))
        counts, rad, n = ER.focus_ee(rows, status, n_rays, c, [0.0] if radii is None else radii,
                                     [1.0] if fractions is None else fractions)
        return (None if radii is None else counts), (None if fractions is None else rad), n

    def focus_psf(self, focus_rows, ndim, maxdim, wave_scale, want_psf=True):
        from rayoptics_amd.engine import FOCUS_PSF_STATS_DTYPE
        rows, status = focus_rows.rows.numpy(), focus_rows.status.numpy()
        n_items, K = rows.shape[:2]
        self.calls.append(('psf', n_items))
        psf = np.empty((n_items, K, maxdim, maxdim))
        stats = np.zeros((n_items, K), dtype=FOCUS_PSF_STATS_DTYPE)
        for i in range(n_items):
            for k in range(K):
                w = np.where(status[i] == abi.OK, wave_scale[i] * rows[i, k, 2], np.nan).reshape(ndim, ndim)
                psf[i, k] = LO.numpy_calc_psf(w, ndim, maxdim)
                stats['strehl'][i, k] = 0.5 + 0.01 * k
        return self.torch.from_numpy(psf), stats

    def focus_psf_ee(self, psf, pitch, centers, radii, want_centroid=True):
        self.calls.append(('psf_ee', int(psf.shape[0]), centers is None))
        ee, cen = ER.focus_psf_ee(psf.numpy(), pitch, centers, radii)
        return ee, (cen if want_centroid else None)


def _fixture(monkeypatch, name='through_focus_ee.npz', opd=False):
    pytest.importorskip('torch')
    import focus_map_fixture as FM
    from rayoptics_amd import analyses
    m = FM.FocusMapFixtureModel(np.load(os.path.join(GOLDEN, name)), 'dblgauss')
    eng = _NumpyEeEngine(m, opd=opd)
    monkeypatch.setattr(analyses, '_launch_setup', lambda _m, fld, wvl, _kw, _mode: (eng, fld, wvl, None))
    return m, eng


def test_geometric_result_assembled_from_an_engine_double(monkeypatch):
    """through_focus_ee over the reference's own rays: one trace; each item's radii are the exact
    order statistics about its spot centroid; the polychromatic curve is the spectrally weighted
    count fraction about the poly_merge centroid, reaching 1 at its last radius"""
    from rayoptics_amd import analyses
    m, eng = _fixture(monkeypatch)
    z = m.z
    F, W, K = z['abr'].shape[:3]
    n = int(z['ndim'])
    fr = [0.5, 0.8, 1.0]
    radii = np.linspace(0.0, 0.05, 11)
    res = analyses.through_focus_ee(m, m.focs, fractions=fr, radii=radii, num_rays=n, n_curve=64,
                                    **m.map_kwargs())
    assert eng.calls[0] == ('trace', F * W, K, True, True)
    assert res.kind == 'geometric' and res.ee_radius.shape == (F, W, K, 3) and res.ee.shape == (F, W, K, 11)
    assert res.poly_ee.shape == (F, K, 64) and res.poly_ee_radius.shape == (F, K, 3)
    assert res.best_focus.shape == (F, 3) and res.best_focus_all.shape == (3,)
    assert np.array_equal(res.image_pts, z['image_pt'])
    ok = eng.status == abi.OK
    for f in range(F):
        for w in range(W):
            i = f * W + w
            for k in range(K):
                x, y = eng.rows[i, k, 0], eng.rows[i, k, 1]
                c = (x[ok[i]].mean(), y[ok[i]].mean())
                counts, rad, nn = ER.plane_ee(x, y, ok[i], c, radii, fr)
                assert np.array_equal(res.ee_radius[f, w, k], rad) and res.n_ok[f, w, k] == nn
                assert np.array_equal(res.ee[f, w, k], counts / nn)
                assert res.ee_radius[f, w, k, 2] == np.sqrt(((x[ok[i]] - c[0]) ** 2 + (y[ok[i]] - c[1]) ** 2).max())
    assert (res.poly_ee[..., -1] == 1.0).all() and (res.poly_ee[..., 0] < 0.01).all()
    assert np.allclose(res.curve_radii[..., 1] * 63, res.curve_radii[..., -1], rtol=1e-12)
    # one wavelength alone: the curve is its own count fraction, its EE80 within a curve step
    one = analyses.through_focus_ee(m, m.focs, fractions=fr, num_rays=n, n_curve=256, flds=[m.fields[1]],
                                    wvls=[m.wvls[1]], field_wts=[1.0], spectral_wts=[1.0], ref_wvl=m.wvls[1])
    step = one.curve_radii[0, :, 1]
    assert np.all(np.abs(one.poly_ee_radius[0, :, 1] - one.ee_radius[0, 0, :, 1]) <= step * (1 + 1e-9))
    assert np.all(np.abs(one.poly_ee_radius[0, :, 2] - one.ee_radius[0, 0, :, 2]) <= step * (1 + 1e-9))


def test_diffraction_result_assembled_from_an_engine_double(monkeypatch):
    """through_focus_ee(kind='diffraction') over the reference's OPD grids: the PSFs are calc_psf's,
    each item's curve is the restatement about its centroid, the polychromatic curve the weighted
    mean about the weighted centroid; a PSF bound of one field changes nothing"""
    from rayoptics_amd import analyses
    m, eng = _fixture(monkeypatch, 'through_focus_mtf.npz', opd=True)
    z = m.z
    F, W, K = z['opd'].shape[:3]
    n, M = int(z['ndim']), int(z['maxdims'][0])
    pitch = z['psf_scaling'][:, :, :, 0, 1]
    radii = np.linspace(0, 0.01, 5)
    res = analyses.through_focus_ee(m, m.focs, kind='diffraction', radii=radii, num_rays=n, maxdim=M, pitch=pitch,
                                    n_curve=32, **m.map_kwargs())
    assert res.ee_radius.shape == (F, W, K, 2) and res.ee.shape == (F, W, K, 5)
    assert res.strehl.shape == (F, W, K) and np.array_equal(res.pitch, pitch)
    k = K // 2
    for f in range(F):
        for w in range(W):
            exp, cen = ER.focus_psf_ee(z['psf'][f, w][None, None], pitch[f, w, k], None, radii)
            assert np.max(np.abs(res.ee[f, w, k] - exp[0, 0])) <= 1e-12
            assert np.max(np.abs(res.centroid[f, w, k] - cen[0, 0])) <= 1e-12 * pitch[f, w, k] * M
    s = np.asarray(m.spectral_wts)
    C = (s[:, None, None] * (z['image_pt'][0] + res.centroid[0])).sum(axis=0) / s.sum()
    psf = np.stack([LO.numpy_calc_psf(z['opd'][0, w, k], n, M) for w in range(W)])
    per_w = [ER.psf_ee(psf[w], pitch[0, w, k], C[k] - z['image_pt'][0, w, k], res.curve_radii[0, k])
             for w in range(W)]
    assert np.max(np.abs(res.poly_ee[0, k] - ER.poly_psf_ee(per_w, s))) <= 1e-12
    monkeypatch.setattr(analyses, 'MTF_PSF_CHUNK_BYTES', 1)
    eng.calls.clear()
    small = analyses.through_focus_ee(m, m.focs, kind='diffraction', radii=radii, num_rays=n, maxdim=M, pitch=pitch,
                                      n_curve=32, **m.map_kwargs())
    assert sum(c[0] == 'psf' for c in eng.calls) == F
    assert small.poly_ee.tobytes() == res.poly_ee.tobytes() and small.ee.tobytes() == res.ee.tobytes()
