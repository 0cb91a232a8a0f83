"""CPU-side checks of the geometric MTF through focus (rox_focus_gmtf,
analyses.through_focus_gmtf): the NumPy restatement (tests/gmtf_ref.py) against closed forms, the
polychromatic merge along given directions, the tangential / sagittal vectors, the host logic of
ThroughFocusGMTF on synthetic arrays, and the argument errors of the Python function and of the C
entry, which answers them before it touches a device.

Closed forms are compared within gmtf_ref.tol() (derived in test_gpu_through_focus_gmtf.py) plus
1e-14 for the rounding of the closed form's own evaluation (a few ulp of sin and cos at arguments
below 2 pi, divided by sines no smaller than 0.03)."""
import ctypes as C
import os

import numpy as np
import pytest

import gmtf_ref as GR
from rayoptics_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FREQS = np.array([0.0, 1.0, 5.0, 10.0, 37.5, 100.0, 400.0])


@pytest.fixture(scope='module')
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        'rox_build', os.path.join(ROOT, 'ray-optics_amd', 'build.py'))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return abi.declare(C.CDLL(b.build()))


# ---- the restatement against closed forms ---------------------------------------------------
def test_restatement_uniform_lattice_is_the_dirichlet_kernel():
    n, h = 101, 2.0 ** -10                               # u_j exact in binary64
    u = (np.arange(n) - (n - 1) / 2) * h
    nu = FREQS[1:]
    got = GR.otf_of(u, nu)
    exp = np.sin(n * np.pi * nu * h) / (n * np.sin(np.pi * nu * h))
    t = GR.tol(n, nu, np.abs(u).max()) + 1e-14
    assert (np.abs(got.real - exp) <= t).all() and (np.abs(got.imag) <= t).all()
    zero = GR.otf_of(u, [0.0])
    assert zero[0].real == 1.0 and zero[0].imag == 0.0


def test_restatement_two_rays_and_shift():
    a, c = 0.0123, -0.0071
    got = GR.otf_of([-a, a], FREQS)
    t = GR.tol(2, FREQS, a) + 1e-14
    assert (np.abs(got.real - np.cos(2 * np.pi * FREQS * a)) <= t).all() and (np.abs(got.imag) <= t).all()
    # a shift by c multiplies by exp(-2 pi i nu c)
    rng = np.random.default_rng(1)
    u = rng.normal(scale=0.01, size=500)
    base, moved = GR.otf_of(u, FREQS), GR.otf_of(u + c, FREQS)
    exp = base * np.exp(-2j * np.pi * FREQS * c)
    t = 2 * GR.tol(500, FREQS, np.abs(u).max() + abs(c)) + 1e-14
    assert (np.abs(moved.real - exp.real) <= t).all() and (np.abs(moved.imag - exp.imag) <= t).all()


def test_restatement_projection_histogram_and_empty_plane():
    rng = np.random.default_rng(2)
    x, y = rng.normal(size=50), rng.normal(size=50)
    ok = rng.random(50) < 0.7
    dirs = [(1.0, 0.0), (0.0, 1.0), (0.6, 0.8)]
    edges = np.broadcast_to(np.linspace(-2, 2, 9), (3, 9))
    otf, lsf, n, umax = GR.plane_gmtf(x, y, ok, dirs, FREQS, edges)
    assert n == ok.sum() and otf.shape == (3, 7) and lsf.shape == (3, 8)
    assert np.array_equal(lsf[0], np.histogram(x[ok], edges[0])[0])
    assert np.array_equal(otf[1], GR.otf_of(y[ok], FREQS)) and umax[0] == np.abs(x[ok]).max()
    otf, lsf, n, _u = GR.plane_gmtf(x, y, np.zeros(50, bool), dirs, FREQS, edges)
    assert n == 0 and np.isnan(otf.real).all() and (lsf == 0).all()


# ---- poly_otf_merge along directions ----------------------------------------------------------
def test_poly_otf_merge_with_dirs():
    from rayoptics_amd import analyses
    rng = np.random.default_rng(3)
    W, K, Q = 3, 4, 7
    otf = rng.normal(size=(W, K, 2, Q)) + 1j * rng.normal(size=(W, K, 2, Q))
    otf[1, 2] = np.nan                                   # a plane no ray reached
    ip = rng.normal(size=(W, K, 2)) * 0.01
    s = [1.0, 2.0, 1.0]
    now = analyses.poly_otf_merge(otf, ip, s, 1, FREQS)
    xy = analyses.poly_otf_merge(otf, ip, s, 1, FREQS, dirs=[(1.0, 0.0), (0.0, 1.0)])
    assert now.tobytes() == xy.tobytes()
    # one wavelength returns its own OTF
    one = analyses.poly_otf_merge(otf[:1], ip[:1], [0.7], 0, FREQS, dirs=[(0.6, 0.8), (0.8, -0.6)])
    assert one.tobytes() == otf[0].tobytes()
    # the lateral-colour phase is the projection of the image-point difference
    e = np.array([(0.6, 0.8), (0.8, -0.6), (0.0, 1.0)])
    o3 = np.ones((2, K, 3, Q), dtype=np.complex128)
    got = analyses.poly_otf_merge(o3, ip[:2], [1.0, 1.0], 0, FREQS, dirs=e)
    dl = (ip[1] - ip[0]) @ e.T                                             # [K, D]
    exp = 0.5 * (1.0 + np.exp(-2j * np.pi * dl[..., None] * FREQS))
    assert np.max(np.abs(got - exp)) <= 1e-13
    with pytest.raises(ValueError):
        analyses.poly_otf_merge(o3, ip[:2], [1.0, 1.0], 0, FREQS, dirs=e[:2])


# ---- directions -----------------------------------------------------------------------------
def test_tangential_and_sagittal_vectors():
    from rayoptics_amd import analyses
    ip = [(0.0, 0.0), (0.0, 7.5), (0.0, -7.5), (3.0, 4.0), (-3.0, 4.0)]
    dirs, labels = analyses.gmtf_directions(('x', 'y', 't', 's', (0.6, 0.8)), ip)
    assert labels == ['x', 'y', 't', 's', (0.6, 0.8)] and dirs.shape == (5, 5, 2)
    assert (dirs[:, 0] == (1.0, 0.0)).all() and (dirs[:, 1] == (0.0, 1.0)).all() and (dirs[:, 4] == (0.6, 0.8)).all()
    t, s = dirs[:, 2], dirs[:, 3]
    assert np.array_equal(t[0], (0.0, 1.0)) and np.array_equal(s[0], (1.0, 0.0))      # on axis
    assert np.array_equal(t[1], (0.0, 1.0)) and np.array_equal(s[1], (1.0, 0.0))      # +y
    assert np.array_equal(t[2], (0.0, -1.0)) and np.array_equal(s[2], (-1.0, 0.0))    # -y
    assert not np.signbit(s[1]).any() and not np.signbit(t[2][0])
    assert np.array_equal(t[3], (0.6, 0.8)) and np.array_equal(s[3], (0.8, -0.6))     # oblique
    assert np.array_equal(t[4], (-0.6, 0.8)) and np.array_equal(s[4], (0.8, 0.6))
    assert np.max(np.abs((t * s).sum(axis=-1))) == 0.0


# ---- ThroughFocusGMTF on synthetic arrays -----------------------------------------------------
def synthetic_result(lsf=True):
    from rayoptics_amd import analyses
    F, W, K, D, Q, B = 2, 3, 5, 4, 3, 6
    focs = np.linspace(-0.2, 0.2, K)
    nu = np.array([0.0, 10.0, 30.0])
    # a Gaussian blur whose width is smallest at focus 0.05 (field 0) / -0.05 (field 1)
    best = np.array([0.05, -0.05])
    sig = 0.002 + 0.05 * np.abs(focs[None, :] - best[:, None])                       # [F, K]
    mtf = np.exp(-2 * (np.pi * sig[:, None, :, None, None] * nu) ** 2) * np.ones((F, W, K, D, Q))
    otf = mtf.astype(np.complex128)
    image_pts = np.zeros((F, W, K, 2))
    image_pts[1, :, :, 0], image_pts[1, :, :, 1] = 3.0, 4.0
    dirs, labels = analyses.gmtf_directions(('x', 'y', 't', 's'), image_pts[:, 1, 2])
    n_ok = np.full((F, W, K), 100, dtype=np.int64)
    n_ok[0, 2, :] = 50
    n_ok[1, 0, 1] = 0
    otf[1, 0, 1] = np.nan
    counts = edges = None
    if lsf:
        rng = np.random.default_rng(5)
        counts = rng.integers(0, 9, size=(F, W, K, D, B))
        counts[1, 0, 1] = 0
        edges = analyses.lsf_edges(np.zeros((F, K, D)), np.full((F, 1, 1), 0.03), B)
    res = analyses.ThroughFocusGMTF(focs, nu, [656.3, 587.6, 486.1], [1.0, 1.0], [1.0, 2.0, 1.0], 587.6, labels,
                                    dirs, otf, n_ok, image_pts, lsf=counts, lsf_edges=edges)
    return res, counts, n_ok, best


def test_result_host_logic():
    res, counts, n_ok, best = synthetic_result()
    F, W, K, D, Q = res.otf.shape
    assert res.poly_otf.shape == (F, K, D, Q) and res.best_focus.shape == (F, D, Q)
    assert res.tangential.shape == (F, K, Q) and res.sagittal.shape == (F, K, Q)
    assert res.tangential.tobytes() == np.ascontiguousarray(res.poly_mtf[:, :, 2]).tobytes()
    assert res.sagittal.tobytes() == np.ascontiguousarray(res.poly_mtf[:, :, 3]).tobytes()
    assert np.isfinite(res.poly_mtf).all()               # the NaN wavelength is skipped
    assert np.max(np.abs(res.poly_otf[..., 0] - 1.0)) <= 1e-15
    # the MTF peaks where the blur is smallest
    assert np.max(np.abs(res.best_focus[0, :, 1:] - best[0])) < 0.02
    assert np.max(np.abs(res.best_focus[1, :, 1:] - best[1])) < 0.02
    assert res.best_focus_all.shape == (Q,) and np.max(np.abs(res.best_focus_all[1:])) < 0.03
    # poly_lsf: each wavelength's unit-energy line spread, spectrally weighted
    s = np.array([1.0, 2.0, 1.0])
    exp = (s[:, None, None, None] * counts[0] / n_ok[0][..., None, None]).sum(axis=0) / s.sum()
    assert np.max(np.abs(res.poly_lsf[0] - exp)) <= 1e-15
    sk = np.array([0.0, 2.0, 1.0])                       # field 1, focus 1: wavelength 0 has no ray
    exp = (sk[:, None, None] * counts[1, :, 1] / np.maximum(n_ok[1, :, 1], 1)[:, None, None]).sum(axis=0) / sk.sum()
    assert np.max(np.abs(res.poly_lsf[1, 1] - exp)) <= 1e-15
    assert np.array_equal(res.esf, np.cumsum(res.poly_lsf, axis=-1))
    assert np.array_equal(res.lsf_inside, res.poly_lsf.sum(axis=-1)) and res.lsf_edges.shape == (F, K, D, 7)
    assert np.max(np.abs(res.esf[..., -1] - res.lsf_inside)) <= 1e-15
    plain, _c, _n, _b = synthetic_result(lsf=False)
    assert plain.lsf is None and plain.poly_lsf is None and plain.esf is None and plain.lsf_inside is None


def test_poly_lsf_merge_without_any_ray():
    from rayoptics_amd import analyses
    out = analyses.poly_lsf_merge(np.zeros((2, 3, 1, 4)), np.array([[5, 0, 2], [5, 0, 0]]), [1.0, 3.0])
    assert np.isnan(out[1]).all() and (out[[0, 2]] == 0.0).all()
    e = analyses.lsf_edges([0.5, -1.0], 0.25, 4)
    assert np.array_equal(e, [[0.25, 0.375, 0.5, 0.625, 0.75], [-1.25, -1.125, -1.0, -0.875, -0.75]])


# ---- argument errors ------------------------------------------------------------------------
@pytest.mark.parametrize('kw,word', [
    (dict(freqs=[]), 'frequencies'),
    (dict(freqs=[1.0, -2.0]), 'frequencies'),
    (dict(freqs=[float('nan')]), 'frequencies'),
    (dict(freqs=np.zeros(abi.MAX_MTF_FREQS + 1)), 'frequencies'),
    (dict(directions=()), 'directions'),
    (dict(directions=['x'] * (abi.MAX_GMTF_DIRS + 1)), 'directions'),
    (dict(directions=('x', 'r')), 'direction'),
    (dict(directions=((0.0, 0.0),)), 'direction'),
    (dict(directions=((1.0, float('inf')),)), 'direction'),
    (dict(directions=((1.0, 0.0, 0.0),)), 'direction'),
    (dict(lsf_bins=-1), 'lsf_bins'),
    (dict(lsf_bins=abi.MAX_LSF_BINS + 1), 'lsf_bins'),
    (dict(lsf_bins=8, lsf_half_width=0.0), 'lsf_half_width'),
    (dict(lsf_bins=8, lsf_half_width=float('nan')), 'lsf_half_width'),
    (dict(lsf_bins=8, lsf_half_width=[[0.1]]), 'lsf_half_width'),
    (dict(num_rays=0), 'num_rays'),
    (dict(focs=[]), 'through_focus_gmtf'),
])
def test_python_argument_errors(kw, word):
    """each is raised before the model is looked at (None stands in for it)"""
    from rayoptics_amd import analyses
    args = dict(focs=[-0.1, 0.0, 0.1], freqs=[10.0])
    args.update(kw)
    with pytest.raises(ValueError, match=word):
        analyses.through_focus_gmtf(None, **args)


def test_abi_declares_the_prototype(lib):
    assert 'rox_focus_gmtf' in abi.EXPORTS and abi.MAX_GMTF_DIRS == 8 and abi.MAX_LSF_BINS == 4096
    assert lib.rox_focus_gmtf.restype is C.c_int and len(lib.rox_focus_gmtf.argtypes) == 16
    with open(os.path.join(ROOT, 'include', 'roxtrace.h')) as f:
        src = f.read()
    assert '#define ROX_MAX_GMTF_DIRS   8' in src and '#define ROX_MAX_LSF_BINS 4096' in src


def c_error_cases():
    """(name, overrides, the word rox_last_error() must hold)"""
    nan, inf = float('nan'), float('inf')
    return [
        ('n_items 0', dict(n_items=0), 'n_items'),
        ('n_items over', dict(n_items=abi.MAX_FOCUS_ITEMS + 1), 'n_items'),
        ('n_planes 0', dict(n_planes=0), 'n_planes'),
        ('n_planes over', dict(n_planes=abi.MAX_FOCUS_PLANES + 1), 'n_planes'),
        ('null rows', dict(rows=None), 'rows'),
        ('null status', dict(status=None), 'status'),
        ('n_rays 0', dict(n_rays=0), 'n_rays'),
        ('n_rays over ld', dict(n_rays=321), 'n_rays'),
        ('n_rays beyond a launch', dict(ld=2 ** 63 - 1, n_rays=2 ** 63 - 1), 'n_rays'),
        ('n_dir 0', dict(n_dir=0), 'n_dir'),
        ('n_dir over', dict(n_dir=abi.MAX_GMTF_DIRS + 1), 'n_dir'),
        ('null dirs', dict(dirs=None), 'dirs'),
        ('zero direction', dict(dirs=[(1.0, 0.0), (0.0, 0.0)] * 2), 'dirs[1]'),
        ('nan direction', dict(dirs=[(1.0, 0.0), (0.0, 1.0), (1.0, 0.0), (nan, 1.0)]), 'dirs[3]'),
        ('n_freq -1', dict(n_freq=-1), 'n_freq'),
        ('n_freq over', dict(n_freq=abi.MAX_MTF_FREQS + 1), 'n_freq'),
        ('otf without freqs', dict(n_freq=0), 'n_freq'),
        ('otf with null freqs', dict(freqs=None), 'freqs'),
        ('negative freq', dict(freqs=[0.0, 1.0, -1.0]), 'freqs[2]'),
        ('inf freq', dict(freqs=[0.0, inf, 1.0]), 'freqs[1]'),
        ('n_bins -1', dict(n_bins=-1), 'n_bins'),
        ('n_bins over', dict(n_bins=abi.MAX_LSF_BINS + 1), 'n_bins'),
        ('lsf without bins', dict(n_bins=0), 'n_bins'),
        ('lsf with null edges', dict(edges=None), 'edges'),
        ('edges not increasing', dict(bad_edge=(7, 2, 'same')), 'edges[37]'),
        ('edges nan', dict(bad_edge=(0, 4, 'nan')), 'edges[4]'),
        ('null otf and lsf', dict(otf=None, lsf=None), 'otf and lsf'),
    ]


def call_gmtf(lib, over, rows=None, status=None, outs=None, stream=None):
    """one rox_focus_gmtf call on 2 items x 3 planes x 300 rays (ld 320), 2 directions, 3
    frequencies, 4 bins, with ``over`` replacing arguments; rows / status / outs: pointers (the
    default ones are host memory the entry never reads: every case fails its checks first)"""
    n_items, K, D, Q, B = 2, 3, 2, 3, 4
    a = dict(n_items=n_items, n_planes=K, rows=rows if rows is not None else 8, ld=320,
             status=status if status is not None else 8, n_rays=300, n_dir=D,
             dirs=[(1.0, 0.0), (0.0, 1.0)] * n_items, n_freq=Q, freqs=[0.0, 1.0, 5.0], n_bins=B,
             otf=outs[0] if outs else 8, lsf=outs[1] if outs else 8, n_ok=outs[2] if outs else None)
    edges = np.ascontiguousarray(np.broadcast_to(np.linspace(-1.0, 1.0, B + 1), (n_items, K, D, B + 1)))
    a['edges'] = edges
    bad = over.pop('bad_edge', None)
    a.update(over)
    if bad is not None:
        row, j, kind = bad
        flat = edges.reshape(-1, B + 1)
        flat[row, j] = flat[row, j - 1] if kind == 'same' else float('nan')
    keep = []

    def arr(v):
        if v is None or isinstance(v, int):
            return v
        v = np.ascontiguousarray(np.asarray(v, dtype=np.float64))
        keep.append(v)
        return v.ctypes.data

    return lib.rox_focus_gmtf(a['n_items'], a['n_planes'], a['rows'], a['ld'], a['status'], a['n_rays'], a['n_dir'],
                              arr(a['dirs']), a['n_freq'], arr(a['freqs']), a['otf'], a['n_bins'], arr(a['edges']),
                              a['lsf'], a['n_ok'], stream)


@pytest.mark.parametrize('name,over,word', c_error_cases(), ids=[c[0] for c in c_error_cases()])
def test_c_argument_errors_need_no_device(lib, name, over, word):
    assert call_gmtf(lib, dict(over)) == -1
    msg = lib.rox_last_error().decode()
    assert msg.startswith('rox_focus_gmtf: ') and word in msg, msg
