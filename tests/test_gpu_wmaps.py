"""rox_weighted_maps on the device against its NumPy restatement (tests/wmaps_ref.py), every output
bit for bit and under both forced scatter paths and the default (ROX_WMAPS_PATH): the sums are
integers, so there is no tolerance anywhere but where a float64 sum of rox_segment_foci is the
other side.  Contention, the invariances the header promises, the count maps against
rox_surface_footprints on traced packets, the maps of analyses.ghost_analysis on a plane-parallel
plate, and every argument error."""
import contextlib
import os

import numpy as np
import pytest

import wmaps_ref as WR
from packets_fixture import torch, trace_packets, upload  # noqa: F401 (torch: the fixture)
from rayoptics_amd import abi, workloads
from test_gpu_ghost import plain_table, plate_model

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
PATHS = ['', 'lds', 'global']
N_RAYS = [1, 63, 64, 65, 1023, 1024, 1025, 1089]
BINS = [(1, 1), (8, 4), (128, 128), (1024, 3)]
N_SEG = 3
# dyadic, so that -3.5, 0.5 and 4.5 are edges in x at 8, 128 and 1024 bins, -3.25, -0.25 and 2.75 in y at 4 and 128
WINDOW = (0.5, -0.25, 4.0, 3.0)
WINDOWS3 = [(0.5, -0.25, 4.0, 3.0), (100.0, 100.0, 1.0, 1.0), (-0.75, 0.5, 2.0, 5.0)]     # no ray reaches map 1


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


def synthetic(R, seed):
    """packets [N_SEG, 10, R] with failed rays interleaved (NaN in their rows and weights); among
    the OK rays' weights zeros, one negative, one +inf and one NaN, and positions exactly on the
    outer and on interior edges of WINDOW and one ulp outside it (where there are rays enough)
    -> (seg, status, fail_surf, weight)"""
    rng = np.random.default_rng(seed)
    seg = rng.normal(size=(N_SEG, 10, R)) * 3.0
    status = np.where(rng.random(R) < 0.3, rng.integers(1, 5, R), 0).astype(np.uint8)
    status[0] = abi.OK
    weight = rng.uniform(0.0, 1.0, R) * 10.0 ** rng.uniform(-5, 0, R)
    ok = np.flatnonzero(status == abi.OK)
    weight[ok[::7]] = 0.0
    if len(ok) >= 24:
        weight[ok[3]], weight[ok[5]], weight[ok[6]] = -0.25, np.inf, np.nan
        on_x = [-3.5, 4.5, 0.5, np.nextafter(4.5, np.inf), np.nextafter(-3.5, -np.inf), 0.5]
        on_y = [0.0, 0.0, 0.0, 0.0, 0.0, -0.25]
        for k in (1, N_SEG - 1):
            seg[k, 0, ok[10:16]], seg[k, 1, ok[10:16]] = on_x, on_y
            seg[k, 1, ok[16:20]], seg[k, 0, ok[16:20]] = [-3.25, 2.75, -0.25, np.nextafter(2.75, np.inf)], 1.0
            seg[k, 0, ok[20]] = np.nan                      # an OK ray without a position: outside
    seg[:, :, status != abi.OK] = np.nan
    weight[status != abi.OK] = np.nan
    return seg, status, np.zeros(R, np.int16), weight


@pytest.fixture(scope='module')
def world(torch):
    """one engine, and per ray count three items' packets in HBM with their weights (row 1 of a
    [3, 2, R] tensor whose row 0 is NaN) -- made once, read by every test, never changed"""
    from rayoptics_amd.engine import TraceEngine
    eng = TraceEngine(plain_table(N_SEG))
    assert eng.num_segments(abi.INTERSECT_OBJ) == N_SEG
    packs = {}

    def get(R):
        if R not in packs:
            cases = [synthetic(R, 1000 + 10 * R + i) for i in range(3)]
            res = [upload(eng, s, st, fs) for s, st, fs, _w in cases]
            assert all(r.out_struct().ld > R for r in res)          # ld > n_rays: the rows are padded
            wt = torch.full((3, 2, R), float('nan'), dtype=torch.float64, device=eng.device)
            wt[:, 1] = torch.from_numpy(np.stack([c[3] for c in cases])).to(eng.device)
            packs[R] = (cases, res, wt)
        return packs[R]

    yield eng, get
    eng.close()


# (items, slot, weights, factors, item_map, n_maps, windows)
VARIANTS = [(1, -1, True, [0.37], None, 1, [WINDOW]),
            (3, 1, True, [0.5, 2.0, 0.125], None, 3, WINDOWS3),
            (3, -1, False, [0.2, 0.5, 0.3], [0, 0, 0], 1, [WINDOW]),
            (3, -1, True, None, [0, 2, 0], 3, WINDOWS3),
            (1, 1, False, None, None, 1, [WINDOW])]
_REFS = {}


def reference(cases, R, v, bins):
    key = (R, v, bins)
    if key not in _REFS:
        items, slot, use_w, fac, imap, n_maps, wins = VARIANTS[v]
        k = N_SEG - 1 if slot < 0 else slot
        _REFS[key] = WR.weighted_maps([c[0][k, 0] for c in cases[:items]], [c[0][k, 1] for c in cases[:items]],
                                      [c[1] for c in cases[:items]],
                                      [c[3] for c in cases[:items]] if use_w else None, fac, imap, n_maps,
                                      np.array(wins), bins[0], bins[1])
    return _REFS[key]


def call(eng, res, wt, v, bins, **kw):
    items, slot, use_w, fac, imap, n_maps, wins = VARIANTS[v]
    return eng.weighted_maps(res[:items], abi.INTERSECT_OBJ, slot=slot, weight=wt[:items] if use_w else None,
                             weight_row=1, item_factor=fac, item_map=imap, n_maps=n_maps, window=np.array(wins),
                             bins=bins, want_counts=True, raw=True, **kw)


def same(got, ref, what):
    for name, a, b in zip(('wmaps', 'counts', 'scale_exp', 'item'), got, ref):
        assert a.dtype == b.dtype and a.shape == b.shape, f'{what}: {name} {a.dtype} {a.shape}'
        assert a.tobytes() == b.tobytes(), f'{what}: {name} differs\n{a}\n{b}'


@pytest.mark.parametrize('path', PATHS)
def test_against_the_restatement(world, path):
    eng, get = world
    with forced(path):
        for R in N_RAYS:
            cases, res, wt = get(R)
            for bins in BINS:
                for v in range(len(VARIANTS)):
                    ref = reference(cases, R, v, bins)
                    same(call(eng, res, wt, v, bins), ref, f'path {path!r} R {R} bins {bins} variant {v}')
    # what the cases are there to exercise
    wm, cnt, e, item = reference(get(1089)[0], 1089, 1, (8, 4))
    assert item['n_bad'].min() >= 3 and (item['n_in'][[0, 2]] > 0).all() and (item['n_out'] > 0).all()
    assert not cnt[1].any() and e[1] != 0 and item['n_in'][1] == 0       # the map no ray reaches
    wm, cnt, e, item = reference(get(1089)[0], 1089, 3, (8, 4))
    assert not cnt[1].any() and e[1] == 0                                # the map without an item
    assert wm[0].sum() == item['q_in'][[0, 2]].sum() and wm[2].sum() == item['q_in'][1]


@pytest.mark.parametrize('path', PATHS)
def test_contention(world, path):
    """all 1089 rays in one bin, and all rays on one bin row"""
    eng, _get = world
    R = 1089
    rng = np.random.default_rng(4)
    st = np.zeros(R, np.uint8)
    w = rng.uniform(0.0, 1.0, (1, 1, R))
    wt = eng.torch.from_numpy(w).to(eng.device)
    for xs, ys in ((np.full(R, 0.1), np.full(R, 0.1)), (np.full(R, 0.1), rng.uniform(-3.0, 2.5, R))):
        seg = np.zeros((N_SEG, 10, R))
        seg[-1, 0], seg[-1, 1] = xs, ys
        res = upload(eng, seg, st, np.zeros(R, np.int16))
        ref = WR.weighted_maps([xs], [ys], [st], [w[0, 0]], None, None, 1, WINDOW, 128, 128)
        with forced(path):
            got = eng.weighted_maps(res, abi.INTERSECT_OBJ, weight=wt, window=WINDOW, bins=128, want_counts=True,
                                    raw=True)
        same(got, ref, f'path {path!r}')
        assert got[1].sum() == R and np.count_nonzero(got[1][0].sum(axis=1)) == 1
        assert got[1].max() == R or ys[0] != ys[1]


@pytest.mark.parametrize('path', PATHS)
def test_invariance(world, path):
    from rayoptics_amd.engine import WMAP_ITEM_DTYPE, records_view
    eng, get = world
    R, bins = 1089, (128, 128)
    cases, res, wt = get(R)
    with forced(path):
        first = call(eng, res, wt, 1, bins)
        same(call(eng, res, wt, 1, bins), first, 'two identical calls')
        dev = call(eng, res, wt, 1, bins, on_device=True)
        host = (dev[0].cpu().numpy(), dev[1].cpu().numpy().view(np.uint32), dev[2].cpu().numpy(),
                records_view(dev[3], WMAP_ITEM_DTYPE))
        same(host, first, 'device destinations')
        # one call over 3 items into 3 maps against 3 calls
        _items, slot, _w, fac, _imap, _n, wins = VARIANTS[1]
        for i in range(3):
            one = eng.weighted_maps(res[i], abi.INTERSECT_OBJ, slot=slot, weight=wt[i:i + 1].contiguous(), weight_row=1,
                                    item_factor=fac[i:i + 1], window=wins[i], bins=bins, want_counts=True, raw=True)
            same(one, tuple(a[i:i + 1] for a in first), f'item {i} on its own')
        for m in range(3):
            assert first[0][m].sum() == first[3]['q_in'][m]
        # the ray columns permuted, seg, status and weight together
        perm = np.random.default_rng(8).permutation(R)
        pres = [upload(eng, s[:, :, perm], st[perm], fs) for s, st, fs, _w in cases]
        got = call(eng, pres, wt[:, :, eng.torch.from_numpy(perm).to(eng.device)].contiguous(), 1, bins)
        same(got[:3], first[:3], 'permuted rays')
        assert got[3].tobytes() == first[3].tobytes()
    # the converted maps: ldexp on the host and on the device
    _items, slot, _w, fac, _imap, _n, wins = VARIANTS[1]
    kw = dict(slot=slot, weight=wt, weight_row=1, item_factor=fac, window=np.array(wins), bins=bins)
    m_host = eng.weighted_maps(res, abi.INTERSECT_OBJ, **kw)[0]
    m_dev = eng.weighted_maps(res, abi.INTERSECT_OBJ, on_device=True, **kw)[0]
    assert m_host.tobytes() == np.ldexp(first[0].astype(np.float64), -first[2][:, None, None]).tobytes()
    assert m_dev.cpu().numpy().tobytes() == m_host.tobytes()


def test_host_maps_in_several_launches(world):
    """three maps of 1024 x 1024 bins bound for host memory are 36 MiB of scratch, over the 32 MiB of
    one launch: the second launch takes the third map.  Same bits as the restatement and as the
    single launch into device memory."""
    eng, get = world
    R, bins = 1089, (1024, 1024)
    cases, res, wt = get(R)
    ref = reference(cases, R, 1, bins)
    host = call(eng, res, wt, 1, bins)
    same(host, ref, 'host destinations')
    dev = call(eng, res, wt, 1, bins, on_device=True)
    assert dev[0].cpu().numpy().tobytes() == ref[0].tobytes()
    assert dev[1].cpu().numpy().view(np.uint32).tobytes() == ref[1].tobytes()
    assert ref[1][2].any() and ref[1][0].any()


def test_counts_are_the_footprint_maps(world):
    """traced double Gauss packets, 33^2 rays: with a centred square window and no weight the
    counts are the image-slot map of rox_surface_footprints(ROX_FP_OK_ONLY)"""
    from rayoptics_amd.engine import TraceEngine
    wl = workloads.load('dblgauss_c2')
    eng = TraceEngine(wl.table)
    flags = abi.INTERSECT_OBJ | abi.CHECK_APERTURES | abi.APPLY_VIGNETTING
    flds = [wl.fields[0], wl.fields[-1]]
    res = trace_packets(eng, flags, flds, [0, 1], 33)
    n_seg = eng.num_segments(flags)
    rec, _m = eng.surface_footprints(res, flags, ok_only=True)
    hw = np.sqrt(rec['r2_max'].max(axis=0)) * 0.5           # some rays outside the box
    nb = 32
    _rec, fmaps = eng.surface_footprints(res, flags, ok_only=True, half_width=hw, n_bins=nb)
    for path in PATHS:
        for k in (n_seg - 1, 3):
            with forced(path):
                _wm, cnt, _e, item = eng.weighted_maps(res, flags, slot=-1 if k == n_seg - 1 else k,
                                                       window=(0.0, 0.0, hw[k], hw[k]), bins=nb, want_counts=True, raw=True)
            assert np.array_equal(cnt, fmaps[:, k]), f'path {path!r} slot {k}'
            assert (item['n_in'] == fmaps[:, k].sum(axis=(1, 2))).all() and (item['n_out'] > 0).any()
    eng.close()


def test_maps_through_ghost_analysis(torch):
    """The plate ghost of test_gpu_ghost with a detector that cuts its patch.  irradiance.sum() *
    bin area = (the map's sum) / area / signal summed and times area, against poly_ratio *
    in_detector = w_in / signal (one field, one wavelength).  The map's sum differs from the exact
    sum of the binned weights by at most n_in * 2^-(e + 1) (the quantisation; no weight exceeds
    their sum, the flux, so e >= 61 - ceil(log2 n) - E(flux)) and w_in by at most n_in * u * w_in
    (the bound rox_segment_foci's sums are held to); the conversion and the two quotients per bin,
    the sum over the bins, the product with the area and the six operations of the other side
    add (n_bins + 12) u."""
    from rayoptics_amd import analyses, session
    model = plate_model(4.0)
    kw = dict(flds=model.fields, wvls=[550.0], num_rays=9)
    free = analyses.ghost_analysis(model, **kw)
    rms = float(free.rms_patch[0, 0, 0])
    det = (1.2 * rms, 0.8 * rms)
    a = analyses.ghost_analysis(model, detector=det, **kw)
    g = analyses.ghost_analysis(model, detector=det, maps=(16, 8), **kw)
    n_in, n = int(g.records[0]['n_in'][0, 0, -1]), int(g.rays[0, 0, 0])
    assert 0 < n_in < n
    for name in ('pairs', 'skipped', 'slots', 'internal_foci', 'trace_flags'):
        assert repr(getattr(a, name)) == repr(getattr(g, name)), name
    for name in ('signal', 'spectral_wts', 'rays', 'flux', 'ratio', 'in_detector', 'centroid', 'rms_patch',
                 'focus_distance', 'poly_flux', 'poly_ratio', 'poly_rms_patch'):
        assert getattr(a, name).tobytes() == getattr(g, name).tobytes(), name
    assert a.records[0].tobytes() == g.records[0].tobytes() and a.irradiance is None
    assert g.irradiance.shape == (1, 1, 16, 8) and g.ray_counts.shape == (1, 1, 16, 8)
    assert g.ray_counts.sum() == n_in
    area = (2 * det[0] / 16) * (2 * det[1] / 8)
    lhs = g.irradiance.sum() * area
    rhs = g.poly_ratio[0, 0] * g.in_detector[0, 0, 0]
    e = 61 - (n - 1).bit_length() - int(np.frexp(g.flux[0, 0, 0])[1])           # at most the scale exponent
    signal = float(g.signal[0, 0])
    bound = n_in * 2.0 ** -(e + 1) / signal + (n_in + 128 + 12) * U * rhs
    print(f'sum(irradiance) * area {lhs!r} poly_ratio * in_detector {rhs!r}: error {abs(lhs - rhs):.3g} bound {bound:.3g}')
    assert abs(lhs - rhs) <= bound
    assert g.signal_irradiance.shape == (1, 16, 8) and g.irradiance_total.tobytes() == g.irradiance[0].tobytes()
    assert g.peak[0, 0] == g.irradiance.max() and g.peak_over_signal[0, 0] == g.peak[0, 0] / g.signal_irradiance.max()
    assert g.ranking(by='peak') == [(0, float(g.peak_over_signal[0, 0]))] and 'peak' in g.table()
    with pytest.raises(ValueError, match='detector'):
        analyses.ghost_analysis(model, maps=8, **kw)
    session.clear()


def test_argument_errors(world):
    from rayoptics_amd.engine import WMAP_ITEM_DTYPE, load_library
    lib = load_library()
    eng, get = world
    R = 63
    cases, res, wt = get(R)
    good = res[0].out_struct()
    nbx = nby = 4
    wm = np.full((2, nbx, nby), -7, np.int64)
    cnt = np.full((2, nbx, nby), 7, np.uint32)
    exp = np.full(2, -7, np.int32)
    item = np.zeros(2, WMAP_ITEM_DTYPE)
    win = np.array([[0.0, 0.0, 1.0, 1.0], [0.0, 0.0, 1.0, 1.0]])
    w_ptr = wt.data_ptr() + 8 * R                           # row 1 of item 0

    def call_c(n_items=2, n_rays=R, slot=-1, weight=w_ptr, stride=2 * R, factor=None, imap=None, n_maps=2, window=win,
               nbx=nbx, nby=nby, p_wm=wm.ctypes.data, p_cnt=cnt.ctypes.data, p_exp=exp.ctypes.data,
               p_item=item.ctypes.data, outs=None):
        arr = (abi.Out * 2)(*(outs or [good, res[1].out_struct()]))
        wm[:], cnt[:], exp[:], item['n_in'] = -7, 7, -7, -7
        fac = None if factor is None else np.asarray(factor, np.float64)
        im = None if imap is None else np.asarray(imap, np.int32)
        rc = lib.rox_weighted_maps(eng._handle, abi.INTERSECT_OBJ, n_items, arr, n_rays, slot, weight, stride,
                                   None if fac is None else fac.ctypes.data, None if im is None else im.ctypes.data,
                                   n_maps, window.ctypes.data, nbx, nby, p_wm, p_cnt, p_exp, p_item, None)
        return rc, lib.rox_last_error().decode()

    def window_with(c, value):
        w = win.copy()
        w[1, c] = value
        return w

    o = abi.Out.from_buffer_copy(bytes(good))
    o.ld = R - 1
    bad = [(dict(slot=N_SEG), 'slot'), (dict(slot=-2), 'slot'), (dict(nbx=0), 'nbx'), (dict(nbx=1025), 'nbx'),
           (dict(nby=0), 'nby'), (dict(nby=1025), 'nby'), (dict(n_maps=1), 'n_maps'),
           (dict(imap=[0, 2]), 'item 1: item_map'), (dict(imap=[-1, 0]), 'item 0: item_map'),
           (dict(window=window_with(0, np.nan)), 'window[1][0]'), (dict(window=window_with(1, np.inf)), 'window[1][1]'),
           (dict(window=window_with(2, 0.0)), 'window[1][2]'), (dict(window=window_with(3, -1.0)), 'window[1][3]'),
           (dict(factor=[1.0, -0.5]), 'item 1: item_factor'), (dict(factor=[np.nan, 1.0]), 'item 0: item_factor'),
           (dict(p_exp=None), 'scale_exp'), (dict(p_wm=None, p_cnt=None, p_item=None), 'null wmaps, counts and item'),
           (dict(stride=R - 1), 'weight_stride'), (dict(n_items=0), 'n_items'), (dict(n_rays=0), 'n_rays'),
           (dict(n_maps=0, imap=[0, 0]), 'n_maps'), (dict(outs=[good, o]), 'item 1: ld')]
    for kw, word in bad:
        rc, msg = call_c(**kw)
        assert rc == -1 and 'rox_weighted_maps' in msg and word in msg, (kw, rc, msg)
        assert (wm == -7).all() and (cnt == 7).all() and (exp == -7).all() and (item['n_in'] == -7).all(), \
            f'{kw}: outputs touched'
    rc, msg = call_c()
    assert rc == 0, msg
    ref = WR.weighted_maps([c[0][-1, 0] for c in cases[:2]], [c[0][-1, 1] for c in cases[:2]], [c[1] for c in cases[:2]],
                           [c[3] for c in cases[:2]], None, None, 2, win, nbx, nby)
    same((wm, cnt, exp, item), ref, 'the C entry, every output on the host')
    # counts alone, and the item records alone
    rc, msg = call_c(p_wm=None, p_exp=None, p_item=None)
    assert rc == 0 and np.array_equal(cnt, ref[1]) and (wm == -7).all(), msg
    rc, msg = call_c(p_wm=None, p_exp=None, p_cnt=None)
    assert rc == 0 and item.tobytes() == ref[3].tobytes() and (cnt == 7).all(), msg
