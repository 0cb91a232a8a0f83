"""CPU-side checks of the MTF through focus (rox_focus_mtf, analyses.through_focus_mtf): the line
OTF's NumPy restatement (tests/line_otf.py) against the FFT-free pupil autocorrelation on the
reference's own PSFs, the polychromatic merge on synthetic OTFs, the best-focus rules, argument
errors (C and Python) without a device, and the result assembled from an engine double over
tests/golden/through_focus_mtf.npz."""
import ctypes as C
import os

import numpy as np
import pytest

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


@pytest.mark.parametrize('field', ['f0', 'f1'])
def test_line_otf_is_the_pupil_autocorrelation_at_lattice_frequencies(field):
    """on the reference's calc_psf of tests/golden/through_focus_psf.npz (ndim 32; f0 at maxdim
    64, f1 at 48, where the circular autocorrelation wraps and the identity still holds), the
    line OTF at nu = m / (M p) equals the normalised circular autocorrelation of calc_psf's padded
    pupil array, for every m up to Nyquist, within 1e-12"""
    z = np.load(os.path.join(GOLDEN, 'through_focus_psf.npz'))
    d = {k.split('/', 1)[1]: z[k] for k in z.files if k.startswith(field + '/')}
    ndim, M = int(d['ndim']), int(d['psf_maxdim'])
    j = list(d['maxdims']).index(M)
    m = np.arange(M // 2 + 1)
    for i, k in enumerate(d['psf_focs']):
        p = d['psf_scaling'][k, j, 1]
        got = LO.line_otf(d['psf'][i], p, m / (M * p))
        exp = LO.autocorrelation_otf(d['opd'][k], ndim, M, m)
        assert np.max(np.abs(got - exp)) <= 1e-12, k
        assert np.max(np.abs(got[:, 0] - 1.0)) <= 1e-15
    # over Nyquist: NaN; an empty plane: NaN
    p = d['psf_scaling'][0, j, 1]
    assert np.isnan(LO.line_otf(d['psf'][0], p, [0.51 / p])).all()
    assert np.isnan(LO.line_otf(np.zeros((M, M)), p, [0.0])).all()


def test_poly_merge_of_synthetic_otfs():
    from rayoptics_amd import analyses
    K, Q = 3, 7
    nu = np.linspace(0.0, 60.0, Q)
    delta = 0.004
    ip = np.zeros((2, K, 2))
    ip[1, :, 0] = delta                                 # lateral colour along x
    otf = np.ones((2, K, 2, Q), dtype=np.complex128)
    got = analyses.poly_otf_merge(otf, ip, [1.0, 1.0], 0, nu)
    assert np.allclose(np.abs(got[:, 0]), np.abs(np.cos(np.pi * nu * delta)), rtol=0, atol=1e-15)
    assert np.array_equal(got[:, 1], np.ones((K, Q)))    # y: no shift
    # one wavelength gives itself exactly
    rng = np.random.default_rng(1)
    one = rng.normal(size=(1, K, 2, Q)) + 1j * rng.normal(size=(1, K, 2, Q))
    assert np.array_equal(analyses.poly_otf_merge(one, rng.normal(size=(1, K, 2)), [0.3], 0, nu), one[0])
    # NaN items are skipped and the remaining weights renormalised; none left -> NaN
    two = np.concatenate([one, np.full((1, K, 2, Q), np.nan + 0j)])
    two[1, 0, 0, 0] = 5.0
    ip2 = np.zeros((2, K, 2))
    got = analyses.poly_otf_merge(two, ip2, [0.3, 0.7], 0, nu)
    assert np.array_equal(got[1:], one[0, 1:])
    assert np.array_equal(got[0, 1], one[0, 0, 1]) and np.array_equal(got[0, 0, 1:], one[0, 0, 0, 1:])
    assert abs(got[0, 0, 0] - (0.3 * one[0, 0, 0, 0] + 0.7 * 5.0)) <= 1e-15
    none = analyses.poly_otf_merge(np.full((2, K, 2, Q), np.nan + 0j), ip2, [1.0, 1.0], 0, nu)
    assert np.isnan(none).all()


def _result(otf, image_pts=None, focs=None, field_wts=None):
    from rayoptics_amd import analyses
    F, W, K, _two, Q = otf.shape
    focs = np.linspace(-0.02, 0.02, K) if focs is None else focs
    ip = np.zeros((F, W, K, 2)) if image_pts is None else image_pts
    return analyses.ThroughFocusMTF(focs, np.linspace(0, 50, Q), [500.0 + w for w in range(W)],
                                    field_wts if field_wts is not None else [1.0] * F, [1.0] * W, 500.0, otf,
                                    np.full((F, W, K), 1e-3), ip, np.ones((F, W, K)))


def test_best_focus_is_the_mtf_maximum():
    K, Q = 9, 3
    focs = np.linspace(-0.02, 0.02, K)
    peaks = np.array([[0.004, -0.006], [0.008, 0.0]])          # [F, direction]
    otf = np.empty((2, 1, K, 2, Q), dtype=np.complex128)
    for f in range(2):
        for d in range(2):
            curve = np.exp(-((focs - peaks[f, d]) / 0.01) ** 2)
            otf[f, 0, :, d, :] = curve[:, None] * np.array([1.0, 0.8, 0.5])
    r = _result(otf, focs=focs, field_wts=[1.0, 3.0])
    assert r.best_focus.shape == (2, 2, Q) and (r.best_focus_kind == 'vertex').all()
    assert np.all(np.abs(r.best_focus - peaks[:, :, None]) < 1e-3)
    mean = (1.0 * r.poly_mtf[0].mean(axis=1) + 3.0 * r.poly_mtf[1].mean(axis=1)) / 4.0
    from rayoptics_amd import analyses
    for q in range(Q):
        assert (r.best_focus_all[q], r.best_focus_all_kind[q]) == analyses.best_focus(focs, -mean[:, q])
    # the maximum at the end of the scan
    otf[:] = np.linspace(0.1, 0.9, K)[None, None, :, None, None]
    r = _result(otf, focs=focs)
    assert (r.best_focus == focs[-1]).all() and (r.best_focus_kind == 'end').all()


def test_tangential_and_sagittal_only_for_meridional_fields():
    K, Q = 3, 2
    otf = np.ones((2, 1, K, 2, Q), dtype=np.complex128)
    otf[:, :, :, 0] = 0.25                              # x
    ip = np.zeros((2, 1, K, 2))
    ip[0, ..., 1] = 0.5                                 # field 0 in the y-z plane
    ip[1, ..., 0] = 0.1                                 # field 1 with an x component
    r = _result(otf, image_pts=ip)
    assert list(r.meridional) == [True, False]
    assert (r.tangential[0] == 1.0).all() and (r.sagittal[0] == 0.25).all()
    assert np.isnan(r.tangential[1]).all() and np.isnan(r.sagittal[1]).all()


def test_python_argument_errors_before_any_launch():
    """odd or small num_rays, maxdim < 2 num_rays, negative or non-finite frequencies raise
    ValueError before the model is touched (the model here has nothing to trace)"""
    from rayoptics_amd import analyses
    model = object()
    with pytest.raises(ValueError, match='even'):
        analyses.through_focus_mtf(model, [0.0], [10.0], num_rays=31, maxdim=128)
    with pytest.raises(ValueError, match='even'):
        analyses.through_focus_mtf(model, [0.0], [10.0], num_rays=0, maxdim=128)
    with pytest.raises(ValueError, match='2 num_rays'):
        analyses.through_focus_mtf(model, [0.0], [10.0], num_rays=32, maxdim=63)
    for bad in ([-1.0], [np.nan], [np.inf], [10.0, -0.5], []):
        with pytest.raises(ValueError, match='frequenc'):
            analyses.through_focus_mtf(model, [0.0], bad, num_rays=32, maxdim=64)
    with pytest.raises(ValueError, match='frequenc'):
        analyses.through_focus_mtf(model, [0.0], np.ones(abi.MAX_MTF_FREQS + 1), num_rays=32, maxdim=64)
    with pytest.raises(ValueError, match='focus values'):
        analyses.through_focus_mtf(model, [], [10.0], num_rays=32, maxdim=64)


def test_c_argument_errors_without_a_device(lib):
    """every check of rox_focus_mtf comes before it touches a device: each returns ROX_E_ARG and
    names its parameter"""
    psf = np.zeros(2 * 16 * 16)
    pitch = np.full(2, 1e-3)
    freqs = np.array([0.0, 10.0, 20.0])
    out = np.zeros(2 * 2 * 3 * 2)
    P, PI, FR, O = psf.ctypes.data, pitch.ctypes.data, freqs.ctypes.data, out.ctypes.data
    bad_p = np.array([1e-3, 0.0])
    nan_p = np.array([np.nan, 1e-3])
    bad_f = np.array([0.0, -1.0, 2.0])
    inf_f = np.array([0.0, np.inf, 2.0])
    cases = [((0, 2, P, 16, PI, 3, FR, O), b'n_items'),
             ((abi.MAX_FOCUS_ITEMS + 1, 2, P, 16, PI, 3, FR, O), b'n_items'),
             ((1, 0, P, 16, PI, 3, FR, O), b'n_planes'),
             ((1, abi.MAX_FOCUS_PLANES + 1, P, 16, PI, 3, FR, O), b'n_planes'),
             ((1, 2, P, 1, PI, 3, FR, O), b'maxdim'),
             ((1, 2, P, 32769, PI, 3, FR, O), b'maxdim'),
             ((1, 2, P, 16, PI, 0, FR, O), b'n_freq'),
             ((1, 2, P, 16, PI, abi.MAX_MTF_FREQS + 1, FR, O), b'n_freq'),
             ((1, 2, None, 16, PI, 3, FR, O), b'psf'),
             ((1, 2, P, 16, None, 3, FR, O), b'pitch'),
             ((1, 2, P, 16, PI, 3, None, O), b'freqs'),
             ((1, 2, P, 16, PI, 3, FR, None), b'otf'),
             ((1, 2, P, 16, bad_p.ctypes.data, 3, FR, O), b'pitch[1]'),
             ((1, 2, P, 16, nan_p.ctypes.data, 3, FR, O), b'pitch[0]'),
             ((1, 2, P, 16, PI, 3, bad_f.ctypes.data, O), b'freqs[1]'),
             ((1, 2, P, 16, PI, 3, inf_f.ctypes.data, O), b'freqs[1]')]
    for args, name in cases:
        assert lib.rox_focus_mtf(*args, None) == -1, args
        msg = lib.rox_last_error()
        assert msg.startswith(b'rox_focus_mtf') and name in msg, (args, msg)
    assert 'rox_focus_mtf' in abi.EXPORTS and abi.MAX_MTF_FREQS == 1024


# ---- the analysis over an engine double --------------------------------------------------
class _Rows:
    def __init__(self, rows, status):
        self.rows, self.status = rows, status


class _NumpyMtfEngine:
    """the three device entries through_focus_mtf uses, served on the host: each item's rows
    carry the reference's OPD grid of tests/golden/through_focus_mtf.npz (in system units),
    focus_psf is calc_psf's arithmetic in NumPy, focus_mtf the NumPy line OTF"""

    def __init__(self, z):
        import torch
        self.torch = torch
        opd = z['opd']                                          # [F, W, K, n, n] waves
        F, W, K, n, _n = opd.shape
        units = z['units_per_nm'] * z['wvls']                   # wavelength in system units
        rows = np.full((F * W, K, 3, n * n), np.nan)
        rows[:, :, 2] = (opd * units[None, :, None, None, None]).reshape(F * W, K, n * n)
        self.rows = rows
        self.status = np.where(np.isnan(opd[:, :, 0]), abi.BLOCKED, abi.OK).astype(np.uint8).reshape(F * W, n * n)
        self.calls = []

    def trace_pupil_grids_focus(self, flds, wvl_idxs, grids, opts_list, planes, want_rows=False, want_stats=True):
        self.calls.append(('trace', len(flds), len(planes[0]), want_rows, want_stats))
        return None, _Rows(self.torch.from_numpy(self.rows), self.torch.from_numpy(self.status))

    def focus_psf(self, focus_rows, ndim, maxdim, wave_scale, want_psf=True):
        from rayoptics_amd.engine import FOCUS_PSF_STATS_DTYPE
        rows, status = focus_rows.rows.numpy(), focus_rows.status.numpy()
        n_items, K = rows.shape[:2]
        self.calls.append(('psf', n_items, ndim, maxdim))
        psf = np.empty((n_items, K, maxdim, maxdim))
        stats = np.zeros((n_items, K), dtype=FOCUS_PSF_STATS_DTYPE)
        for i in range(n_items):
            for k in range(K):
                w = np.where(status[i] == abi.OK, wave_scale[i] * rows[i, k, 2], np.nan).reshape(ndim, ndim)
                psf[i, k] = LO.numpy_calc_psf(w, ndim, maxdim)
                stats['strehl'][i, k] = 0.5 + 0.01 * k
        return self.torch.from_numpy(psf), stats

    def focus_mtf(self, psf, pitch, freqs, on_device=False):
        self.calls.append(('mtf', int(psf.shape[0])))
        return LO.line_otf(psf.numpy(), pitch, freqs)


def _fixture(monkeypatch):
    pytest.importorskip('torch')
    import focus_map_fixture as FM
    from rayoptics_amd import analyses
    z = np.load(os.path.join(GOLDEN, 'through_focus_mtf.npz'))
    m = FM.FocusMapFixtureModel(z, 'dblgauss')
    eng = _NumpyMtfEngine(m.z)
    monkeypatch.setattr(analyses, '_launch_setup', lambda *a: (eng, None, 0, None))
    return m, eng


def test_result_assembled_from_an_engine_double(monkeypatch):
    """through_focus_mtf over the stored reference OPD grids: one trace, one PSF and one MTF call
    over all F W items; the OTFs are the line OTFs of calc_psf of the reference's grids at its
    calc_psf_scaling pitch; a small PSF bound splits the items and changes nothing; a table model
    without pitch= is refused"""
    from rayoptics_amd import analyses
    m, eng = _fixture(monkeypatch)
    z = m.z
    F, W, K = z['opd'].shape[:3]
    ndim, M = int(z['ndim']), int(z['maxdims'][0])
    pitch = z['psf_scaling'][:, :, :, 0, 1]
    nu = np.array([0.0, 10.0, 25.0, 40.0, 55.0])
    with pytest.raises(ValueError, match='pitch'):
        analyses.through_focus_mtf(m, m.focs, nu, num_rays=ndim, maxdim=M, **m.map_kwargs())
    eng.calls.clear()
    res = analyses.through_focus_mtf(m, m.focs, nu, num_rays=ndim, maxdim=M, pitch=pitch, psf=True,
                                     **m.map_kwargs())
    assert eng.calls == [('trace', F * W, K, True, False), ('psf', F * W, ndim, M), ('mtf', F * W)]
    assert res.otf.shape == res.mtf.shape == (F, W, K, 2, nu.size)
    assert res.poly_otf.shape == (F, K, 2, nu.size) and res.best_focus.shape == (F, 2, nu.size)
    assert np.array_equal(res.pitch, pitch) and res.strehl.shape == (F, W, K)
    assert np.array_equal(res.image_pts, z['image_pt'])
    assert res.psf.shape == (F, W, K, M, M)
    for f in range(F):
        for w in range(W):
            assert np.max(np.abs(res.psf[f, w, K // 2] - z['psf'][f, w])) <= 1e-12
            exp = LO.line_otf(z['psf'][f, w], pitch[f, w, K // 2], nu)
            assert np.nanmax(np.abs(res.otf[f, w, K // 2] - exp)) <= 1e-12
    assert np.max(np.abs(res.otf[..., 0] - 1.0)) <= 1e-15
    assert list(res.meridional) == [True, False]
    # a PSF bound of one item: F W calls of each, the same numbers bit for bit
    monkeypatch.setattr(analyses, 'MTF_PSF_CHUNK_BYTES', K * M * M * 8)
    eng.calls.clear()
    small = analyses.through_focus_mtf(m, m.focs, nu, num_rays=ndim, maxdim=M, pitch=pitch, **m.map_kwargs())
    assert sum(c[0] == 'psf' for c in eng.calls) == F * W
    assert small.otf.tobytes() == res.otf.tobytes() and small.poly_otf.tobytes() == res.poly_otf.tobytes()
    assert small.psf is None


def test_the_golden_orientation_data_is_consistent():
    """the fixture's own PSFs (the reference's calc_psf) and spot centroids: on axis the centroid
    is zero; off axis the fine-grid centroid sits several pitches from the image point along x
    and y, where the orientation tests need it"""
    z = np.load(os.path.join(GOLDEN, 'through_focus_mtf.npz'))
    d = {k.split('/', 1)[1]: z[k] for k in z.files}
    cf = d['centroid_fine']
    p = d['psf_scaling_fine'][..., 1]
    assert np.all(np.abs(cf[0]) < 1e-3 * p[0][:, None])
    assert np.all(np.abs(cf[1]) > 3 * p[1][:, None])
    assert d['field_xy'][0, 0] == 0.0 and d['field_xy'][1, 0] != 0.0
