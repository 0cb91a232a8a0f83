"""Two-reflection ghosts on the device: the packets of unfolded tables against the oracle bit for
bit; rox_segment_foci against its NumPy restatement (tests/segfoci_ref.py) on uploaded packets;
its determinism; the focus of a homocentric bundle; the physics of a plane-parallel plate through
analyses.ghost_analysis; every argument error.

Bounds.  u = 2^-53.  Counts, minima, maxima and the in-window counts are exact.  A sum of n terms
(w_sum, w_in) lies within the any-order summation bound n * u * sum|terms| of its longdouble
value.  The means and moments are not plain sums; each is held to the same bound over the terms of
the sum it stands for -- w*a for a mean (over w_sum), w*|a|^2, w*|a.b|, w*|b|^2 about the frame's
origin for a moment, the terms a one-pass evaluation adds -- plus the roundings of FORMING a
term and finishing the quantity, which no summation bound covers: 2 (the product w*a, the
quotient by W) for a mean, 8 for a moment (difference, two squares, their sum, W_P*W_Q/W in three
and the product: the n = 2 case of the pairwise update).  So: |mean - exact| <= (n + 2) u
sum|w a| / W and |m - exact| <= (n + 8) u sum|terms|."""
import math

import numpy as np
import pytest

import fresnel_ref as FR
import segfoci_ref as SR
from helpers import bit_equal
from packets_fixture import torch, trace_packets, upload  # noqa: F401 (torch: the fixture)
from rayoptics_amd import SurfaceTable, abi, ghost, workloads
from rayoptics_amd.table import field_struct
from thinfilm_ref import ROW_BOUND

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
N_RAYS = [1, 63, 64, 65, 129, 513, 1089]
EXACT = ('n', 'n_flat', 'n_bad', 'n_in', 'z_in_min', 'z_in_max', 'z_out_min', 'z_out_max')


def plain_table(n_ifcs):
    surfs = [dict(cv=0, thi=10.0)] + [dict(cv=0.01 * k, thi=3.0, n=1.5 if k % 2 else 1.0) for k in range(1, n_ifcs - 1)]
    return SurfaceTable.from_prescription(surfs + [dict(cv=0, thi=0)])


def synthetic(n_seg, R, seed):
    """packets [n_seg, 10, R] with failed rays interleaved (NaN in their rows and weights), some
    weights zero, one negative and one infinite (where there are rays enough) and one ray with
    N == 0 at slot 1 -> (seg, status, fail_surf, weight)"""
    rng = np.random.default_rng(seed)
    seg = rng.normal(size=(n_seg, 10, R)) * 3.0
    d = rng.normal(size=(n_seg, 3, R)) * 0.2
    d[:, 2] = 1.0
    d[1::2, 2] = -1.0                                      # some segments run backwards
    seg[:, 3:6] = d / np.linalg.norm(d, axis=1, keepdims=True)
    seg[:, 6] = rng.uniform(1.0, 9.0, (n_seg, R))
    status = np.where(rng.random(R) < 0.3, rng.integers(1, 5, R), 0).astype(np.uint8)
    status[0] = abi.OK
    weight = rng.uniform(0.0, 1.0, R)
    ok = np.flatnonzero(status == abi.OK)
    weight[ok[::7]] = 0.0
    if len(ok) >= 12:
        weight[ok[3]], weight[ok[5]] = -0.25, np.inf
        seg[1, 5, ok[8]] = 0.0
        weight[ok[8]] = 0.5
    seg[:, :, status != abi.OK] = np.nan
    weight[status != abi.OK] = np.nan
    return seg, status, np.zeros(R, np.int16), weight


def check(rec, seg, status, weight, window, what, worst):
    """one item's records [n_seg] against the restatement and the bounds of the module docstring"""
    ref, ab, ex = SR.segment_foci(seg, status, weight, window)
    for name in EXACT:
        assert np.array_equal(rec[name], ref[name]), f'{what}: {name}\n{rec[name]}\n{ref[name]}'
    same = sum(rec[name].tobytes() == ref[name].tobytes() for name in rec.dtype.names)
    print(f'{what}: {same} of {len(rec.dtype.names)} fields bit-identical to the restatement')

    def hold(err, bound, name, k):
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else math.inf)
        worst[name] = max(worst.get(name, 0.0), ratio)
        assert err <= bound, f'{what} slot {k}: {name} error {err:.3g} > bound {bound:.3g}'

    for k in range(rec.shape[0]):
        n = int(ref['n'][k])
        for name in ('w_sum', 'w_in'):
            hold(abs(float(np.longdouble(rec[name][k]) - ex[name][k])), n * U * ab[name][k], name, k)
        counted = n > 0 and ref['w_sum'][k] > 0
        for name in ('a_mean', 'b_mean', 'm_aa', 'm_ab', 'm_bb'):
            assert np.isnan(rec[name][k]).all() == (not counted), f'{what} slot {k}: {name} NaN-ness'
        if not counted:
            continue
        W = float(ex['w_sum'][k])
        for name, s in (('a_mean', 'sa'), ('b_mean', 'sb')):
            for c in range(2):
                hold(abs(float(np.longdouble(rec[name][k, c]) - ex[name][k, c])), (n + 2) * U * ab[s][k, c] / W, name, k)
        for name in ('m_aa', 'm_ab', 'm_bb'):
            hold(abs(float(np.longdouble(rec[name][k]) - ex[name][k])), (n + 8) * U * ab[name][k], name, k)
    return ref


@pytest.mark.parametrize('n_ifcs', [3, 6])
def test_against_the_restatement(torch, n_ifcs):
    from rayoptics_amd.engine import TraceEngine
    eng = TraceEngine(plain_table(n_ifcs))
    assert eng.num_segments(abi.INTERSECT_OBJ) == n_ifcs
    worst = {}
    for R in N_RAYS:
        cases = [synthetic(n_ifcs, R, 100 * n_ifcs + R + i) for i in range(3)]
        res = [upload(eng, s, st, fs) for s, st, fs, _w in cases]
        wt = torch.full((3, 2, R), float('nan'), dtype=torch.float64, device=eng.device)
        wt[:, 1] = torch.from_numpy(np.stack([c[3] for c in cases])).to(eng.device)
        window = (2.5, 4.0)
        for items in (1, 3):
            for use_w in (False, True):
                for win in (None, window):
                    rec = eng.segment_foci(res[:items], abi.INTERSECT_OBJ, weight=wt[:items] if use_w else None,
                                           weight_row=1, window=win)
                    assert rec.shape == (items, n_ifcs)
                    for i in range(items):
                        seg, st, _fs, w = cases[i]
                        ref = check(rec[i], seg, st, w if use_w else None, win,
                                    f'n_seg {n_ifcs} R {R} item {i}/{items} weight {use_w} window {win}', worst)
                        if R >= 63 and use_w:
                            assert ref['n_bad'][0] == 2 and ref['n_flat'][1] == 1 and ref['n_flat'][0] == 0
                        if win is not None and R >= 63:
                            assert 0 < ref['n_in'][0] < ref['n'][0]
    print('largest error / bound:', {k: f'{v:.3g}' for k, v in worst.items()})
    eng.close()


def test_determinism(torch):
    from rayoptics_amd.engine import TraceEngine, SEG_FOCUS_DTYPE, records_view
    n_ifcs, R = 6, 1089
    eng = TraceEngine(plain_table(n_ifcs))
    cases = [synthetic(n_ifcs, R, 7 + i) for i in range(3)]
    res = [upload(eng, s, st, fs) for s, st, fs, _w in cases]
    wt = torch.from_numpy(np.stack([c[3] for c in cases])[:, None, :].copy()).to(eng.device)
    kw = dict(weight=wt, window=(3.0, 3.0))
    rec = eng.segment_foci(res, abi.INTERSECT_OBJ, **kw)
    again = eng.segment_foci(res, abi.INTERSECT_OBJ, **kw)
    assert rec.tobytes() == again.tobytes()
    raw = eng.segment_foci(res, abi.INTERSECT_OBJ, on_device=True, **kw)
    assert records_view(raw, SEG_FOCUS_DTYPE).tobytes() == rec.tobytes()
    for i in range(3):
        one = eng.segment_foci(res[i], abi.INTERSECT_OBJ, weight=wt[i:i + 1].contiguous(), window=(3.0, 3.0))
        assert one.tobytes() == rec[i:i + 1].tobytes(), f'item {i}: one call of three != its own call'
    # a single counted ray: zero moments, its own a and b as the means
    seg, st, fs, w = cases[0]
    st1 = np.full(R, abi.BLOCKED, np.uint8)
    r = int(np.flatnonzero((st == abi.OK) & (w > 0) & np.isfinite(w))[10])
    st1[r] = abi.OK
    for weight in (None, wt[:1].contiguous()):
        rec1 = eng.segment_foci(upload(eng, seg, st1, fs), abi.INTERSECT_OBJ, weight=weight)[0]
        assert (rec1['n'] == 1).all() and (rec1['n_in'] == 1).all()
        for name in ('m_aa', 'm_ab', 'm_bb'):
            assert (rec1[name] == 0.0).all(), name
        b = seg[:, 3:5, r] / seg[:, 5:6, r]
        assert np.array_equal(rec1['b_mean'], b) or weight is not None
        assert np.allclose(rec1['b_mean'], b, rtol=4 * U, atol=0)
    eng.close()


def test_focus_of_a_homocentric_bundle(torch):
    """Rays through one point P = (px, py, pz) of the slot's frame: a = P.xy - pz*b exactly, so the
    bundle's moments are m_aa = pz^2 m_bb and m_ab = -pz m_bb: zeta* = pz and the smallest
    mean-square radius 0.  The device's a carries the rounding of x - z*(L/N) (3 u |P.xy| + 3 u
    |pz b|, written ea) per ray and its moments the bound of the module docstring; with S = sum
    w|a|^2 etc. the moments' errors are e_aa <= (n + 8) u S_aa + 2 sqrt(m_aa W) ea and likewise
    e_ab, e_bb.  zeta* = -m_ab/m_bb then errs by at most (e_ab + |pz| e_bb) / m_bb and the smallest
    mean square radius (m_aa - m_ab^2/m_bb)/W by at most (e_aa + 2 |pz| e_ab + pz^2 e_bb)/W (first
    order; a factor 2 covers the second)."""
    from rayoptics_amd.engine import TraceEngine, seg_focus_derive
    eng = TraceEngine(plain_table(3))
    R = 513
    rng = np.random.default_rng(11)
    P = np.array([0.7, -1.3, 42.0])
    b = rng.uniform(-0.3, 0.3, (2, R))
    d = np.stack([b[0], b[1], np.ones(R)])
    d /= np.linalg.norm(d, axis=0)
    z = rng.uniform(-2.0, 2.0, R)                           # the sag of the surface the rays leave
    seg = np.zeros((3, 10, R))
    for k in range(3):
        t = (z - P[2]) / d[2]
        seg[k, 0:3] = P[:, None] + t * d
        seg[k, 3:6] = d
        seg[k, 6] = 50.0
    st = np.zeros(R, np.uint8)
    res = upload(eng, seg, st, np.zeros(R, np.int16))
    w = rng.uniform(0.1, 1.0, R)
    wt = torch.from_numpy(w[None, None, :].copy()).to(eng.device)
    for weight, wh in ((None, np.ones(R)), (wt, w)):
        rec = eng.segment_foci(res, abi.INTERSECT_OBJ, weight=weight)[0]
        zeta, ms_min, _ms0, inside = seg_focus_derive(rec)
        bh = seg[1, 3:5] / seg[1, 5:6]
        ah = seg[1, 0:2] - seg[1, 2:3] * bh
        W = wh.sum()
        S_aa, S_ab, S_bb = (wh * (ah * ah).sum(0)).sum(), (wh * np.abs(ah * bh).sum(0)).sum(), (wh * (bh * bh).sum(0)).sum()
        ea = 3 * U * np.abs(P[:2]).max() + 3 * U * abs(P[2]) * np.abs(bh).max() + 3 * U * np.abs(seg[1, 0:2]).max()
        n = R
        e_aa = (n + 8) * U * S_aa + 2 * math.sqrt(rec['m_aa'][1] * W) * ea
        e_ab = (n + 8) * U * S_ab + math.sqrt(rec['m_bb'][1] * W) * ea
        e_bb = (n + 8) * U * S_bb
        bz = 2 * (e_ab + abs(P[2]) * e_bb) / rec['m_bb'][1]
        bm = 2 * (e_aa + 2 * abs(P[2]) * e_ab + P[2] ** 2 * e_bb) / W
        print(f'weighted {weight is not None}: zeta* {zeta[1]!r} (P.z {P[2]}, bound {bz:.3g}) smallest mean square '
              f'radius {ms_min[1]:.3g} (bound {bm:.3g})')
        assert (np.abs(zeta - P[2]) <= bz).all(), zeta
        assert (ms_min <= bm).all(), ms_min
        assert inside.all() and (rec['z_out_max'] > P[2]).all() and (rec['z_in_max'] < P[2]).all()
    eng.close()


def test_unfolded_tables_against_the_oracle(torch):
    """device packets of unfolded tables against the oracle, bit for bit, as every other table"""
    from oracle import oracle
    from oracle.oracle import make_opts as mk
    from rayoptics_amd.engine import TraceEngine, make_grid
    wl = workloads.load('dblgauss_c2')
    flags = abi.INTERSECT_OBJ | abi.CHECK_APERTURES | abi.APPLY_VIGNETTING
    for j, i in ((2, 1), (7, 3), (11, 10), (11, 1)):
        unf = ghost.unfold(wl.table, j, i)
        eng = TraceEngine(unf.table)
        grid = make_grid((-1., -1.), (1., 1.), 17)
        last = unf.table.n_ifcs - 2
        for f, wi in ((wl.fields[0], 0), (wl.fields[-1], len(wl.table.wvls) - 1)):
            opts = mk(flags=flags, out_mode=abi.OUT_FULL, first_surf=1, last_surf=last)
            dev = eng.trace_pupil_grid(f, grid, wi, opts, nan_fill=True).to_host()
            orc = oracle.trace_pupil_grid(unf.table, f, grid, wi, opts)
            assert np.array_equal(dev.status, orc.status) and np.array_equal(dev.fail_surf, orc.fail_surf)
            assert (dev.status == abi.OK).any(), (j, i)
            bit_equal(dev.seg, orc.seg, f'ghost ({j}, {i})')
        eng.close()


N_PLATE, T_PLATE, D_IMG = 1.5, 4.0, 20.0


def plate_model(thickness):
    """a plane-parallel plate in a converging beam: the rays head for a virtual object point 50
    behind the front surface (the object gap is negative), the pupil on the front surface"""
    from rayoptics_amd.workloads import SimpleWorkload, TableModel
    tbl = SurfaceTable.from_prescription([dict(cv=0, thi=-50.0), dict(cv=0, thi=thickness, n=N_PLATE, max_aperture=20.0),
                                          dict(cv=0, thi=D_IMG, max_aperture=20.0), dict(cv=0, thi=0)], wvls=(550.0,))
    fld = field_struct((0., 0., 0.), (0., 0.), 5.0, -50.0)
    return TableModel(SimpleWorkload(tbl, [fld], [(0., 0.)]))


def test_plate_ghost_through_ghost_analysis(torch):
    from rayoptics_amd import analyses
    num = 9
    model, thick = plate_model(T_PLATE), plate_model(3 * T_PLATE)
    g = analyses.ghost_analysis(model, flds=model.fields, wvls=[550.0], num_rays=num, keep_packets=True)
    assert g.pairs == [(2, 1)] and g.skipped == []
    gh = g.results[0][0].to_host(want=('seg', 'status'))
    bf = analyses.beam_footprints(thick, flds=thick.fields, wvls=[550.0], num_rays=num, check_apertures=True,
                                  keep_packets=True)
    th = bf.results[0].to_host(want=('seg', 'status'))
    assert (gh.status == abi.OK).all() and (th.status == abi.OK).all()
    a, b = np.asarray(gh.seg)[-1], np.asarray(th.seg)[-1]
    assert np.asarray(gh.seg).shape[0] == 6 and np.asarray(th.seg).shape[0] == 4
    err = np.abs(a - b) / np.maximum(1.0, np.abs(b))
    print(f'plate ghost (2, 1) against a plate three times as thick: largest image-slot deviation {err.max():.3g}')
    assert err.max() <= 1e-10
    assert a[5].min() > 0.9 and np.ptp(a[0]) > 0.1          # a converging beam that has not yet focused
    # the axial ray's weight: two transmissions and two reflections at normal incidence
    R = ((N_PLATE - 1.0) / (N_PLATE + 1.0)) ** 2
    want = (1.0 - R) ** 2 * R ** 2
    centre = (num // 2) * num + num // 2
    assert a[0, centre] == 0.0 and a[1, centre] == 0.0
    unf = ghost.unfold(model.workload.table, 2, 1)
    from rayoptics_amd import session
    geng = session.engine_for_table(unf.table)
    rows, _s, _i = geng.surface_thinfilm(g.results[0], g.trace_flags, [0], [550.0],
                                         **ghost.coating_tables(model.workload.table, unf, None))
    tol = ROW_BOUND + FR.CLOSED * 4
    print(f'axial ghost ray: weight {rows[0, 0, centre]!r} closed form {want!r} (bound {tol:.3g})')
    assert abs(rows[0, 0, centre] - want) <= tol
    assert abs(g.flux[0, 0, 0] - np.nansum(rows[0, 0])) <= num * num * U * np.nansum(rows[0, 0])
    assert 0 < g.ratio[0, 0, 0] < 2 * R * R and g.rays[0, 0, 0] == num * num
    ideal = analyses.ghost_analysis(model, flds=model.fields, wvls=[550.0], num_rays=num, coatings='ideal')
    assert ideal.pairs == [(2, 1)] and (ideal.flux == 0.0).all() and (ideal.rays == num * num).all()
    session.clear()


def catadioptric_model():
    """a window, two mirrors and a field lens: pairs across a mirror cannot be unfolded"""
    from rayoptics_amd.workloads import SimpleWorkload, TableModel
    tbl = SurfaceTable.from_prescription(
        [dict(cv=0, thi=200.0), dict(cv=0, thi=2.0, n=1.5, max_aperture=12.0), dict(cv=0, thi=40.0, max_aperture=12.0),
         dict(cv=-0.008, thi=-30.0, mode='reflect', max_aperture=12.0),
         dict(cv=-0.004, thi=35.0, mode='reflect', max_aperture=6.0),
         dict(cv=0.01, thi=2.0, n=1.6, max_aperture=8.0), dict(cv=0, thi=15.0, max_aperture=8.0), dict(cv=0, thi=0)],
        wvls=(550.0,))
    fld = field_struct((0., 0., 0.), (0., 0.), 4.0, 200.0)
    return TableModel(SimpleWorkload(tbl, [fld], [(0., 0.)]))


def test_rc_telescope_and_skipped_pairs(torch):
    """the RC telescope's surfaces are mirrors in air: it has no pair, nothing is skipped and
    nothing raises; with a window before and a lens behind two mirrors the pairs across a mirror
    are skipped and reported, the others analysed"""
    from rayoptics_amd import analyses, session
    model = workloads.TableModel('rc_telescope_c4')
    g = analyses.ghost_analysis(model, flds=model.fields, wvls=list(model.workload.table.wvls), num_rays=9)
    assert g.pairs == [] and g.skipped == [] and g.ranking() == [] and 'pair' in g.table()
    cat = catadioptric_model()
    g = analyses.ghost_analysis(cat, flds=cat.fields, wvls=[550.0], num_rays=9)
    assert g.pairs == [(2, 1), (6, 5)]
    assert [p for p, _why in g.skipped] == [(5, 1), (5, 2), (6, 1), (6, 2)]
    assert all('interface 3 between them is a mirror' == why for _p, why in g.skipped)
    assert g.flux.shape == (2, 1, 1) and 'skipped' in g.table()
    session.clear()


def test_argument_errors(torch):
    from rayoptics_amd.engine import TraceEngine, load_library, SEG_FOCUS_DTYPE
    lib = load_library()
    n_ifcs, R = 3, 65
    eng = TraceEngine(plain_table(n_ifcs))
    seg, st, fs, w = synthetic(n_ifcs, R, 3)
    res = upload(eng, seg, st, fs)
    good = res.out_struct()
    wt = torch.from_numpy(w.copy()).to(eng.device)
    rec = np.zeros((2, n_ifcs), SEG_FOCUS_DTYPE)
    win = np.array([1.0, 1.0])

    def call(sys=eng._handle, outs=None, n_items=1, n_rays=R, weight=wt.data_ptr(), stride=R, window=win,
             rec_p=rec.ctypes.data):
        arr = (abi.Out * 2)(*(outs or [good, good]))
        rec['n'] = -7
        rc = lib.rox_segment_foci(sys, abi.INTERSECT_OBJ, n_items, arr, n_rays, weight, stride,
                                  window.ctypes.data if window is not None else None, rec_p, None)
        return rc, lib.rox_last_error().decode()

    def bad(field, value):
        o = abi.Out.from_buffer_copy(bytes(good))
        setattr(o, field, value)
        return [good, o]

    cases = [(dict(sys=None), 'sys'), (dict(rec_p=None), 'rec'), (dict(outs=bad('ld', R - 1), n_items=2), 'item 1: ld'),
             (dict(outs=bad('seg', None), n_items=2), 'item 1'), (dict(stride=R - 1), 'weight_stride'),
             (dict(window=np.array([1.0, 0.0])), 'window[1]'), (dict(window=np.array([-1.0, 1.0])), 'window[0]'),
             (dict(window=np.array([np.nan, 1.0])), 'window[0]'), (dict(n_items=0), 'n_items'),
             (dict(n_rays=0), 'n_rays'), (dict(n_rays=(1 << 28) + 1), 'n_rays')]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == -1 and 'rox_segment_foci' in msg and word in msg, (kw, rc, msg)
        assert (rec['n'] == -7).all(), f'{kw}: outputs touched'
    rc, msg = call()
    assert rc == 0, msg
    assert rec['n'][0, 0] > 0 and (rec['n'][1] == -7).all()
    eng.close()
