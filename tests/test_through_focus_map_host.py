"""CPU-side checks of the field-and-wavelength through-focus map (rox_trace_through_focus_grids,
analyses.through_focus_map): every argument error of the batched entry before a device is
touched, the polychromatic merge against a direct computation on pooled rows, and the
field-curvature / overall best-focus rules on synthetic curves."""
import ctypes as C
import os

import numpy as np
import pytest

from rayoptics_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        'rox_build', os.path.join(ROOT, 'ray-optics_amd', 'build.py'))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return abi.declare(C.CDLL(b.build()))


def _args(n_items=3, n_planes=2, ld=64, rows=True, stats=True, null=None):
    """valid arguments of 3 items x 2 planes over an 8 x 8 grid, no system; ``null`` names an
    array to pass as NULL"""
    from rayoptics_amd.engine import make_grid, make_opts
    from rayoptics_amd.table import field_struct
    n, K = max(n_items, 1), max(n_planes, 1)
    flds = (abi.Field * n)(*[field_struct([0.0, 0.1 * i, 0.0], (0., 0.), 1.0, 10.0) for i in range(n)])
    wvl = (C.c_int32 * n)(*([0] * n))
    grids = (abi.Grid * n)(*[make_grid((-1. + 0.1 * i, -1.), (1., 1.), 8) for i in range(n)])
    opts = (abi.Opts * n)(*[make_opts(out_mode=abi.OUT_FAN, first_surf=1, last_surf=2) for _ in range(n)])
    p = (abi.FocusPlane * (n * K))()
    for q in p:
        q.wf.ref_radius = 100.0
    buf = np.zeros(n * K * 3 * 64)
    st = (abi.FocusStats * (n * K))()
    a = dict(sys=None, n_items=n_items, flds=flds, wvl=wvl, grids=grids, opts=opts, n_planes=n_planes,
             planes=p, rows=buf.ctypes.data if rows else None, ld=ld, status=None,
             stats=st if stats else None, stream=None)
    if null:
        a[null] = None
    return a, buf


def _call(lib, a):
    return lib.rox_trace_through_focus_grids(a['sys'], a['n_items'], a['flds'], a['wvl'], a['grids'],
                                             a['opts'], a['n_planes'], a['planes'], a['rows'], a['ld'],
                                             a['status'], a['stats'], a['stream'])


def _err(lib, a, msg):
    assert _call(lib, a) == -1
    got = lib.rox_last_error()
    assert msg in got, got
    return got


def test_constant_and_export(lib):
    assert abi.MAX_FOCUS_ITEMS == 1024
    assert 'rox_trace_through_focus_grids' in abi.EXPORTS
    assert hasattr(lib, 'rox_trace_through_focus_grids')


@pytest.mark.parametrize('kw,msg', [
    (dict(n_items=0), b'n_items 0 outside [1, 1024]'),
    (dict(n_items=abi.MAX_FOCUS_ITEMS + 1), b'n_items 1025 outside'),
    (dict(n_planes=0), b'n_planes 0 outside'),
    (dict(n_planes=abi.MAX_FOCUS_PLANES + 1), b'n_planes 257 outside'),
    (dict(null='flds'), b'null array'),
    (dict(null='wvl'), b'null array'),
    (dict(null='grids'), b'null array'),
    (dict(null='opts'), b'null array'),
    (dict(null='planes'), b'null array'),
    (dict(rows=False, stats=False), b'both null'),
    (dict(ld=63), b'ld (63) < rays (64)'),
])
def test_argument_errors_without_a_device(lib, kw, msg):
    """ROX_E_ARG before anything is enqueued (no system exists here: the checks come first)"""
    a, _buf = _args(**kw)
    _err(lib, a, msg)


def test_item_errors_name_the_item(lib):
    a, _ = _args()
    a['grids'][2].num = 9                                   # grid mismatch
    _err(lib, a, b'item 2: grid kind, num and row block')
    a, _ = _args()
    a['grids'][1].kind = abi.GRID_FAN
    _err(lib, a, b'item 1: grid')
    a, _ = _args()
    a['grids'][1].row_count = 4
    _err(lib, a, b'item 1: grid')
    a, _ = _args()
    a['opts'][1].out_mode = abi.OUT_OPD
    _err(lib, a, b'item 1: out_mode must be ROX_OUT_FAN')
    for flag in (abi.HOST_POINTERS, abi.HITS_APPEND):
        a, _ = _args()
        a['opts'][2].flags |= flag
        _err(lib, a, b'item 2: device pointers only')
    for flag in (abi.FILTER_PHANTOMS, abi.FAST_FP64):
        a, _ = _args()
        a['opts'][1].flags |= flag
        _err(lib, a, b'item 1: ROX_FILTER_PHANTOMS, ROX_FAST_FP64, first_surf and last_surf')
    a, _ = _args()
    a['opts'][2].last_surf = 1
    _err(lib, a, b'item 2: ROX_FILTER_PHANTOMS')
    a, _ = _args()
    a['opts'][0].first_surf = 0                             # item 0 differs from the others
    _err(lib, a, b'item 1: ROX_FILTER_PHANTOMS')


def test_a_bad_plane_names_item_and_plane(lib):
    a, _ = _args()
    a['planes'][2 * 2 + 1].wf.ref_radius = 0.0              # item 2, plane 1
    _err(lib, a, b'item 2 plane 1: bad wf')
    a, _ = _args()
    a['planes'][1 * 2 + 0].wf.kind = 7                      # item 1, plane 0
    _err(lib, a, b'item 1 plane 0: bad wf')
    a, _ = _args()                                          # valid arguments, no system: still no device
    _err(lib, a, b'null system')


def _stats_of(x, y, w):
    """one wavelength's record (FOCUS_STATS_DTYPE fields) of rays relative to its image point"""
    n = len(x)
    if not n:
        return dict(n=0, cx=np.nan, cy=np.nan, rms_spot=np.nan, rms_spot_image_pt=np.nan,
                    opd_mean=np.nan, opd_rms=np.nan, opd_min=np.nan, opd_max=np.nan)
    cx, cy = x.mean(), y.mean()
    return dict(n=n, cx=cx, cy=cy, rms_spot=np.sqrt(np.mean((x - cx) ** 2 + (y - cy) ** 2)),
                rms_spot_image_pt=np.sqrt(np.mean(x ** 2 + y ** 2)), opd_mean=w.mean(),
                opd_rms=np.sqrt(np.mean((w - w.mean()) ** 2)), opd_min=w.min(), opd_max=w.max())


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_poly_merge_equals_pooled_rows(seed):
    """the merge of per-wavelength records == the weighted statistics of the pooled rays in
    absolute image coordinates (lateral colour included), within 1e-12 relative"""
    from rayoptics_amd.analyses import POLY_STATS_DTYPE, poly_merge
    from rayoptics_amd.engine import FOCUS_STATS_DTYPE
    rng = np.random.default_rng(seed)
    W, K = 3, 5
    s = rng.uniform(0.2, 2.0, W)
    ref = 1
    stats = np.zeros((W, K), dtype=FOCUS_STATS_DTYPE)
    ip = rng.normal(0, 0.3, (W, K, 2)) + np.array([0.0, 12.0])
    pooled = [[] for _ in range(K)]
    for w in range(W):
        for k in range(K):
            n = 0 if (w == 2 and k == 3) else int(rng.integers(5, 400))
            x = rng.normal(0.01 * w, 0.02 * (k + 1), n)
            y = rng.normal(-0.03 * w, 0.015 * (k + 1), n)
            op = rng.normal(-300.0 + 50 * w, 0.05 * (k + 1), n)     # a large piston per wavelength
            for key, v in _stats_of(x, y, op).items():
                stats[key][w, k] = v
            pooled[k].append((s[w], x + ip[w, k, 0], y + ip[w, k, 1], op - (op.mean() if n else 0)))
    got = poly_merge(stats, ip, s, ref)
    assert got.dtype == POLY_STATS_DTYPE and got.shape == (K,)
    for k in range(K):
        wt = np.concatenate([np.full(len(p[1]), p[0]) for p in pooled[k]])
        X = np.concatenate([p[1] for p in pooled[k]])
        Y = np.concatenate([p[2] for p in pooled[k]])
        D = np.concatenate([p[3] for p in pooled[k]])
        N = wt.sum()
        cx, cy = (wt * X).sum() / N, (wt * Y).sum() / N
        exp = dict(n=N, cx=cx, cy=cy,
                   rms_spot=np.sqrt((wt * ((X - cx) ** 2 + (Y - cy) ** 2)).sum() / N),
                   rms_spot_ref_pt=np.sqrt((wt * ((X - ip[ref, k, 0]) ** 2 + (Y - ip[ref, k, 1]) ** 2)).sum() / N),
                   rms_wavefront=np.sqrt((wt * D ** 2).sum() / N))
        for key, v in exp.items():
            assert abs(got[key][k] - v) <= 1e-12 * abs(v), (seed, k, key, got[key][k], v)


def test_poly_merge_without_rays_is_nan():
    from rayoptics_amd.analyses import poly_merge
    from rayoptics_amd.engine import FOCUS_STATS_DTYPE
    stats = np.zeros((2, 3), dtype=FOCUS_STATS_DTYPE)
    for name in FOCUS_STATS_DTYPE.names[1:]:
        stats[name] = np.nan
    stats['n'][0, 1] = 4
    stats['cx'][0, 1] = stats['cy'][0, 1] = stats['rms_spot'][0, 1] = stats['opd_rms'][0, 1] = 0.5
    got = poly_merge(stats, np.zeros((2, 3, 2)), [1.0, 1.0], 0)
    assert np.isnan(got['rms_spot'][[0, 2]]).all() and np.isnan(got['rms_wavefront'][[0, 2]]).all()
    assert got['n'][1] == 4 and got['rms_spot'][1] == 0.5 and got['rms_wavefront'][1] == 0.5


def test_field_and_overall_best_focus():
    """the best focus of each field's curve (field curvature) and of the weighted mean curve"""
    from rayoptics_amd.analyses import field_best_focus, overall_best_focus
    x = np.linspace(-0.5, 0.5, 21)
    z = np.array([0.0, -0.12, -0.3])                        # a curved best-focus surface
    a = np.array([1.0, 2.0, 0.5])
    curves = a[:, None] * (x[None, :] - z[:, None]) ** 2 + 0.1
    f, kind = field_best_focus(x, curves)
    assert list(kind) == ['vertex'] * 3
    np.testing.assert_allclose(f, z, atol=1e-12)
    wt = np.array([1.0, 1.0, 0.5])
    best, kind = overall_best_focus(x, curves, wt)
    exp = (wt * a * z).sum() / (wt * a).sum()               # vertex of the weighted sum of parabolas
    assert kind == 'vertex' and abs(best - exp) < 1e-12
    curves[2, 20] = np.nan                                  # a plane no ray of field 2 reached
    f, kind = field_best_focus(x, curves)
    assert kind[2] == 'vertex' and abs(f[2] - z[2]) < 1e-12
    assert overall_best_focus(x, curves, wt)[1] == 'vertex'
    f, kind = field_best_focus(x, np.full((1, 21), np.nan))
    assert kind[0] == 'none' and np.isnan(f[0])
