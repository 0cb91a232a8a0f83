"""Weighted maps without a GPU: the NumPy restatement of rox_weighted_maps (tests/wmaps_ref.py)
against numpy.histogram2d and against a longdouble weighted sum, its order independence, the corner
cases of the scale exponent, and the map arithmetic of analyses.Ghosts on synthetic integer maps.

The bound of the converted map.  A ray's q = rint(v * 2^e) differs from v * 2^e by at most 1/2, so
a bin of ``count`` rays holds its exact sum to count * 2^-(e + 1); the conversion int64 -> float64
rounds once more, by at most |ref| * 2^-53."""
import os

import numpy as np
import pytest

import wmaps_ref as WR
from rayoptics_amd import abi, analyses
from test_ghost_host import synthetic_records


def test_the_export_and_the_record():
    from rayoptics_amd.engine import WMAP_ITEM_DTYPE, load_library
    lib = load_library()
    assert hasattr(lib, 'rox_weighted_maps') and 'rox_weighted_maps' in abi.EXPORTS
    assert WMAP_ITEM_DTYPE.itemsize == 40 and WMAP_ITEM_DTYPE == WR.DTYPE
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, 'include', 'roxtrace.h')).read()
    assert 'int rox_weighted_maps(rox_system *sys, uint32_t trace_flags, int32_t n_items, const rox_out *outs,' in src
    assert '} rox_wmap_item;             /* 40 bytes */' in src


def points(R, seed, window, nbx, nby):
    """R points about the window, among them both outer edges, an interior edge, a value one ulp
    outside and a NaN"""
    cx, cy, hx, hy = window
    rng = np.random.default_rng(seed)
    x, y = rng.normal(cx, 0.6 * hx, R), rng.normal(cy, 0.6 * hy, R)
    ex, ey = WR.edges(cx, hx, nbx), WR.edges(cy, hy, nby)
    x[:6] = [ex[0], ex[-1], ex[nbx // 2], np.nextafter(ex[-1], np.inf), np.nextafter(ex[0], -np.inf), np.nan]
    y[:6] = cy
    y[6:11] = [ey[0], ey[-1], ey[nby // 2], np.nextafter(ey[-1], np.inf), np.nan]
    x[6:11] = cx
    return x, y


@pytest.mark.parametrize('window,nbx,nby', [((0.5, -0.25, 4.0, 3.0), 8, 4), ((0.1, 0.7, 0.3, 1.1), 7, 5),
                                            ((0.0, 0.0, 2.0, 2.0), 1, 1)])
def test_counts_are_numpy_histogram2d(window, nbx, nby):
    R = 1089
    x, y = points(R, 5, window, nbx, nby)
    status = np.zeros(R, np.uint8)
    _wm, counts, _e, item = WR.weighted_maps([x], [y], [status], None, None, None, 1, window, nbx, nby)
    cx, cy, hx, hy = window
    rng2 = [[cx - hx, cx + hx], [cy - hy, cy + hy]]
    keep = ~(np.isnan(x) | np.isnan(y))
    ref, xe, ye = np.histogram2d(x[keep], y[keep], bins=(nbx, nby), range=rng2)
    assert np.array_equal(xe, WR.edges(cx, hx, nbx)) and np.array_equal(ye, WR.edges(cy, hy, nby))
    assert np.array_equal(counts[0], ref.astype(np.uint32))
    assert item['n_in'][0] == ref.sum() and item['n_in'][0] + item['n_out'][0] == R and item['n_bad'][0] == 0
    assert item['n_out'][0] >= 4                            # the NaN and the values one ulp outside


def test_map_against_a_longdouble_sum_and_permutation():
    R, nbx, nby = 1089, 8, 4
    window = (0.5, -0.25, 4.0, 3.0)
    x, y = points(R, 9, window, nbx, nby)
    rng = np.random.default_rng(10)
    w = rng.uniform(0.0, 1.0, R) * 10.0 ** rng.uniform(-6, 0, R)
    status = np.zeros(R, np.uint8)
    wm, counts, e, item = WR.weighted_maps([x], [y], [status], [w], [0.37], None, 1, window, nbx, nby)
    v = w * 0.37
    bx, by = WR.bin_of(WR.edges(0.5, 4.0, nbx), x), WR.bin_of(WR.edges(-0.25, 3.0, nby), y)
    ref = np.zeros((nbx, nby), np.longdouble)
    inside = (bx >= 0) & (by >= 0)
    np.add.at(ref, (bx[inside], by[inside]), v[inside].astype(np.longdouble))
    got = np.ldexp(wm[0].astype(np.float64), -int(e[0]))
    bound = counts[0] * 2.0 ** -(int(e[0]) + 1) + np.abs(ref).astype(np.float64) * 2.0 ** -53
    err = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
    print(f'scale_exp {e[0]}: largest error / bound {np.max(err[bound > 0] / bound[bound > 0]):.3g}')
    assert (err <= bound).all()
    assert wm[0].sum() == item['q_in'][0] and wm[0].max() < 2 ** 62
    # the largest q is below 2^(61 - ceil(log2 N)): no sum of N of them reaches 2^62
    assert np.rint(np.ldexp(v.max(), int(e[0]))) <= 2.0 ** (61 - (R - 1).bit_length())
    perm = rng.permutation(R)
    again = WR.weighted_maps([x[perm]], [y[perm]], [status], [w[perm]], [0.37], None, 1, window, nbx, nby)
    for a, b in zip((wm, counts, e, item), again):
        assert a.tobytes() == b.tobytes()


def test_scale_exp_corner_cases():
    assert WR.scale_exp(None, 1024) == 0 and WR.scale_exp(0.0, 1024) == 0
    # one ray of weight 1 = 0.5 * 2^1: 61 - 0 - 1
    assert WR.scale_exp(1.0, 1) == 60
    # N an exact power of two takes its own logarithm, one more ray the next
    assert WR.scale_exp(1.0, 1024) == 50 and WR.scale_exp(1.0, 1025) == 49 and WR.scale_exp(1.0, 1023) == 50
    assert WR.scale_exp(0.75, 2) == 61 - 1 - 0 and WR.scale_exp(2.0 ** -30, 2) == 61 - 1 + 29
    assert WR.scale_exp(5e-324, 4) == 1000 and WR.scale_exp(1.7e308, 2 ** 38) == -1000
    x = y = np.zeros(1)
    st = np.zeros(1, np.uint8)
    for w, q in ((0.0, 0), (1.0, 2 ** 60), (3.0, 3 * 2 ** 59)):
        wm, c, e, item = WR.weighted_maps([x], [y], [st], [np.array([w])], None, None, 1, (0, 0, 1, 1), 1, 1)
        assert wm[0, 0, 0] == q == item['q_in'][0] and c[0, 0, 0] == 1 and e[0] == (0 if w == 0 else 61 - int(np.frexp(w)[1]))
    # all weights 0, and weights that are left out
    w = np.array([0.0, -1.0, np.inf, np.nan, 0.0])
    wm, c, e, item = WR.weighted_maps([np.zeros(5)], [np.zeros(5)], [np.zeros(5, np.uint8)], [w], None, None, 1,
                                      (0, 0, 1, 1), 2, 2)
    assert e[0] == 0 and not wm.any() and c.sum() == 2 and tuple(item[0]) == (2, 0, 3, 0, 0)


def ghosts_with_maps(P=3, F=2, W=3, nbx=4, nby=2, seed=1):
    rng = np.random.default_rng(seed)
    recs = synthetic_records(P, F, W, 5)
    slots = [dict(source=np.arange(5), pass_=np.array([0, 0, 1, 2, 2]), gap=np.arange(5))] * P
    signal = rng.uniform(0.8, 0.9, (F, W))
    s = np.array([1.0, 2.0, 1.0])
    maps = dict(window=(2.0, 1.5), wmaps=rng.integers(0, 2 ** 40, (P, F, nbx, nby)),
                scale_exp=rng.integers(45, 55, (P, F)), counts=rng.integers(0, 50, (P, F, nbx, nby)),
                signal_wmaps=rng.integers(2 ** 50, 2 ** 52, (F, nbx, nby)), signal_scale_exp=np.array([40, 41]))
    pairs = [(2, 1), (3, 1), (3, 2)][:P]
    return analyses.Ghosts(pairs, [], recs, slots, signal, s, maps=maps), maps, signal, s


def test_ghosts_map_arithmetic():
    g, maps, signal, s = ghosts_with_maps()
    P, F, nbx, nby = maps['wmaps'].shape
    area = (4.0 / nbx) * (3.0 / nby)
    assert np.array_equal(g.map_edges[0], np.linspace(-2.0, 2.0, nbx + 1))
    assert np.array_equal(g.map_edges[1], np.linspace(-1.5, 1.5, nby + 1))
    poly_signal = (signal * s).sum(axis=1) / s.sum()
    for p in range(P):
        for f in range(F):
            flux = np.ldexp(maps['wmaps'][p, f].astype(np.float64), -int(maps['scale_exp'][p, f]))
            assert np.allclose(g.irradiance[p, f], flux / area / poly_signal[f], rtol=4e-16, atol=0)
            # its sum times the bin area: the flux on the detector over the signal flux
            assert np.isclose(g.irradiance[p, f].sum() * area, flux.sum() / poly_signal[f], rtol=1e-14)
    total = np.zeros((F, nbx, nby))
    for p in range(P):
        total = total + g.irradiance[p]
    assert g.irradiance_total.tobytes() == total.tobytes()
    sflux = np.ldexp(maps['signal_wmaps'].astype(np.float64), -maps['signal_scale_exp'][:, None, None])
    assert np.allclose(g.signal_irradiance, sflux / area / poly_signal[:, None, None], rtol=4e-16, atol=0)
    assert np.array_equal(g.peak, g.irradiance.max(axis=(2, 3)))
    assert np.array_equal(g.peak_over_signal, g.peak / g.signal_irradiance.max(axis=(1, 2))[None])
    maps['signal_wmaps'][1] = 0                             # a field whose image point is off the detector
    dark = analyses.Ghosts(g.pairs, [], g.records, g.slots, signal, s, maps=maps)
    assert np.isnan(dark.peak_over_signal[:, 1]).all() and np.array_equal(dark.peak_over_signal[:, 0], g.peak_over_signal[:, 0])
    assert [p for p, _f in dark.ranking(by='peak')] == sorted(range(P), key=lambda p: (-g.peak_over_signal[p, 0], p))
    assert np.array_equal(g.ray_counts, maps['counts']) and g.ray_counts.shape == (P, F, nbx, nby)
    best = g.peak_over_signal.max(axis=1)
    order = sorted(range(P), key=lambda p: (-best[p], p))
    assert g.ranking(by='peak') == [(p, float(best[p])) for p in order]
    assert g.ranking() == g.ranking(by='area') and 'peak/signal peak' in g.table()
    with pytest.raises(ValueError):
        g.ranking(by='flux')


def test_without_maps_nothing_changes():
    P, F, W = 2, 2, 3
    recs = synthetic_records(P, F, W, 5)
    slots = [dict(source=np.arange(5), pass_=np.array([0, 0, 1, 2, 2]), gap=np.arange(5))] * P
    g = analyses.Ghosts([(2, 1), (3, 1)], [], recs, slots, np.full((F, W), 0.9), np.ones(W))
    for name in ('map_edges', 'irradiance', 'irradiance_total', 'signal_irradiance', 'peak', 'peak_over_signal',
                 'ray_counts'):
        assert getattr(g, name) is None, name
    assert 'peak' not in g.table()
    with pytest.raises(ValueError):
        g.ranking(by='peak')
    empty = analyses.Ghosts([], [], [], [], np.full((F, W), 0.9), np.ones(W),
                            maps=dict(window=(1.0, 1.0), wmaps=[], scale_exp=[], counts=[],
                                      signal_wmaps=np.ones((F, 3, 2), np.int64), signal_scale_exp=np.zeros(F, np.int32)))
    assert empty.irradiance.shape == (0, F, 3, 2) and not empty.irradiance_total.any() and empty.ranking(by='peak') == []


def test_maps_without_a_detector_raises():
    """checked before anything else: no model, no device is touched"""
    with pytest.raises(ValueError, match='detector'):
        analyses.ghost_analysis(None, maps=16)
    with pytest.raises(ValueError, match='maps'):
        analyses.ghost_analysis(None, detector=(1.0, 1.0), maps=(16, 0))
