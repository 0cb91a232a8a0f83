"""rox_wave_differentials on the device: the columns against the NumPy restatement
(tests/wavediff_ref.py) bit for bit on uploaded synthetic and on traced packets, the records and
the pivot exactly, sums and gram within the any-order summation bound of their longdouble values,
determinism, the telescoping identity of the shift columns, and analyses.tolerance_sensitivity
against re-traced perturbed models.

Bounds.  u = 2^-53.  n, n_bad, pivot_ray and pivot are exact; cols are the restatement's bits.  A
sum of n terms lies within n * u * sum|terms| of its exact value whatever the order; the terms of
sums are float64 differences (exact inputs) and those of gram their products, which the matrix
cores form and add in an order of their own: (n + 4) * u * sum|terms|, the 4 covering the products'
roundings and those of adding the chunks' records (tests/test_gpu_ghost.py holds its sums so)."""
import numpy as np
import pytest

import wavediff_ref as WR
from packets_fixture import host_of, torch, trace_packets, upload  # noqa: F401 (torch: the fixture)
from rayoptics_amd import SurfaceTable, abi, workloads

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SPOT = abi.INTERSECT_OBJ | abi.CHECK_APERTURES | abi.APPLY_VIGNETTING
N_RAYS = [1, 63, 64, 65, 1024, 1025, 1089]


def rot(ax, ang):
    c, s = np.cos(ang), np.sin(ang)
    m = {0: [[1, 0, 0], [0, c, -s], [0, s, c]], 1: [[c, 0, s], [0, 1, 0], [-s, 0, c]],
         2: [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[ax]
    return np.array(m, dtype=np.float64)


def varied_table(n_ifcs):
    """n_ifcs interfaces with three wavelengths: a mirror, a conic whose radicand turns negative
    inside the packets' range, a toroid (6 slots), tilted frames in both rt_orders"""
    mid = []
    for k in range(1, n_ifcs - 1):
        s = dict(cv=0.013 * k, thi=3.0, n=[1.5 + 0.01 * k, 1.6, 1.7 - 0.02 * k] if k % 2 else [1.0, 1.0, 1.0])
        if k == 1:
            s.update(profile='Conic', cc=3.0, cv=0.2)
        if k == 2:
            s.update(mode='reflect', n=[-1.0, -1.0, -1.0])
        if k == 3:
            s.update(profile='YToroid')
        if k == 4:
            s.update(profile='EvenPolynomial', cc=-1.5, coefs=[0.0, 1e-4])
        mid.append(s)
    t = SurfaceTable.from_prescription([dict(cv=0, thi=10.0, n=[1.0] * 3)] + mid + [dict(cv=0, thi=0, n=[1.0] * 3)],
                                       wvls=(486.1, 587.6, 656.3))
    for i in range(n_ifcs - 1):
        m = rot(i % 3, 0.05 * (i + 1)) @ rot((i + 1) % 3, -0.03 * (i + 2))
        for e in range(9):
            t.rows[i].rt[e] = float(m.reshape(-1)[e])
        t.rows[i].rt_order = abi.RT_F_ORDER if i % 2 else abi.RT_C_ORDER
    return t


def synthetic(n_seg, R, seed, n_aux):
    """packets [n_seg, 10, R] with failed rays interleaved (NaN in their rows and aux values) and,
    where there are rays enough, OK rays with a NaN, a +inf and a -inf aux value and one with an
    infinite row -> (seg, status, fail_surf, aux [n_aux, R])"""
    rng = np.random.default_rng(seed)
    seg = rng.normal(size=(n_seg, 10, R)) * 3.0
    d = rng.normal(size=(n_seg, 3, R)) * 0.2
    d[:, 2] = 1.0
    d[1::2, 2] = -1.0
    seg[:, 3:6] = d / np.linalg.norm(d, axis=1, keepdims=True)
    seg[:, 6] = rng.uniform(1.0, 9.0, (n_seg, R))
    status = np.where(rng.random(R) < 0.3, rng.integers(1, 5, R), 0).astype(np.uint8)
    if R > 2:
        status[0] = abi.BLOCKED                             # the pivot is not ray 0
    aux = rng.normal(size=(n_aux, R))
    ok = np.flatnonzero(status == abi.OK)
    if len(ok) >= 12:
        if n_aux:
            aux[0, ok[0]] = np.nan                          # the lowest OK ray is not the pivot either
            aux[n_aux - 1, ok[5]] = np.inf
            aux[0, ok[9]] = -np.inf
        seg[:, 3, ok[7]] = np.inf                           # d.x: every slot's g is not finite
    seg[:, :, status != abi.OK] = np.nan
    aux[:, status != abi.OK] = np.nan
    return seg, status, np.zeros(R, np.int16), aux


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    nan = np.isnan(a)
    assert np.array_equal(nan, np.isnan(b)), f'{what}: NaN where the restatement has none, or the reverse'
    ua, ub = a.view(np.uint64)[~nan], b.view(np.uint64)[~nan]
    assert np.array_equal(ua, ub), f'{what}: {np.count_nonzero(ua != ub)} of {ua.size} values differ in bits'


def check_item(out, i, table, flags, seg, status, wvl, slots, aux, what, worst):
    item, pivot, sums, gram, cols = out
    ref_cols, counted, n_bad = WR.columns(table, flags, seg, status, wvl, slots, aux if aux.shape[0] else None)
    ref = WR.reduce(ref_cols, counted)
    if cols is not None:
        same_bits(cols[i], ref_cols, f'{what}: cols')
    n = ref['n']
    assert (int(item['n'][i]), int(item['n_bad'][i]), int(item['pivot_ray'][i])) == (n, n_bad, ref['pivot_ray']), \
        (what, item[i], n, n_bad, ref['pivot_ray'])
    same_bits(pivot[i], ref['pivot'], f'{what}: pivot')
    if gram is None:
        return ref
    assert np.array_equal(gram[i], gram[i].T), f'{what}: gram is not symmetric'
    for name, got, ex, ab in (('sums', sums[i], ref['sums'], ref['abs_sums']),
                              ('gram', gram[i], ref['gram'], ref['abs_gram'])):
        err = np.abs(got.astype(np.longdouble) - ex).astype(np.float64)
        bound = ((n + 4) * U * ab).astype(np.float64)
        assert (err <= bound).all(), f'{what}: {name} error {err.max():.3g} beyond its bound (worst ' \
                                     f'{(err / np.where(bound > 0, bound, 1)).max():.3g} of it)'
        worst[name] = max(worst.get(name, 0.0), float((err / np.where(bound > 0, bound, np.inf)).max()))
    return ref


CONFIGS = {3: [([1], 0), (None, 2)], 6: [([2], 0), ([0, 3, 5], 2), (None, 5)]}


@pytest.mark.parametrize('n_ifcs', [3, 6])
def test_against_the_restatement(torch, n_ifcs):
    from rayoptics_amd.engine import TraceEngine
    table = varied_table(n_ifcs)
    eng = TraceEngine(table)
    assert eng.num_segments(abi.INTERSECT_OBJ) == n_ifcs
    worst = {}
    for R in N_RAYS:
        for slots, n_aux in CONFIGS[n_ifcs]:
            cases = [synthetic(n_ifcs, R, 1000 * n_ifcs + 10 * R + i, n_aux) for i in range(3)]
            res = [upload(eng, s, st, fs) for s, st, fs, _a in cases]
            aux = torch.from_numpy(np.stack([c[3] for c in cases])).to(eng.device) if n_aux else None
            n_cols = n_aux + 11 * (n_ifcs if slots is None else len(slots))
            assert n_cols in (11, 35, 71)
            for items in (1, 3):
                wis = [2, 0, 1][:items]
                out = eng.wave_differentials(res[:items], abi.INTERSECT_OBJ, wis, slots=slots,
                                             aux=aux[:items].contiguous() if n_aux else None, want_cols=True)
                cols = out[4].cpu().numpy()
                assert cols.shape == (items, n_cols, R)
                for i in range(items):
                    seg, st, _fs, a = cases[i]
                    ref = check_item((*out[:4], cols), i, table, abi.INTERSECT_OBJ, seg, st, wis[i], slots, a,
                                     f'n_seg {n_ifcs} R {R} cols {n_cols} item {i}/{items}', worst)
                    if R >= 63:
                        assert ref['n'] > 0 and ref['pivot_ray'] > 0
                        assert int(out[0]['n_bad'][i]) == (4 if n_aux else 1)
                # without the columns: the same records
                lean = eng.wave_differentials(res[:items], abi.INTERSECT_OBJ, wis, slots=slots,
                                              aux=aux[:items].contiguous() if n_aux else None)
                assert lean[4] is None
                for a, b in zip(out[:4], lean[:4]):
                    assert a.tobytes() == b.tobytes()
    print('largest error / bound:', {k: f'{v:.3g}' for k, v in worst.items()})
    eng.close()


def test_no_ray_counted(torch):
    from rayoptics_amd.engine import TraceEngine
    table = varied_table(3)
    eng = TraceEngine(table)
    seg, st, fs, aux = synthetic(3, 65, 5, 0)
    st[:] = abi.BLOCKED
    item, pivot, sums, gram, cols = eng.wave_differentials(upload(eng, seg, st, fs), abi.INTERSECT_OBJ, [0],
                                                           want_cols=True)
    assert (int(item['n'][0]), int(item['n_bad'][0]), int(item['pivot_ray'][0])) == (0, 0, -1)
    assert np.isnan(pivot).all() and np.isnan(cols.cpu().numpy()).all()
    assert (sums == 0).all() and (gram == 0).all()
    eng.close()


def test_determinism(torch):
    from rayoptics_amd.engine import TraceEngine, WD_ITEM_DTYPE, records_view
    n_ifcs, R, n_aux = 6, 1089, 5
    table = varied_table(n_ifcs)
    eng = TraceEngine(table)
    cases = [synthetic(n_ifcs, R, 70 + i, n_aux) for i in range(3)]
    res = [upload(eng, s, st, fs) for s, st, fs, _a in cases]
    aux = torch.from_numpy(np.stack([c[3] for c in cases])).to(eng.device)
    wis = [0, 1, 2]
    out = eng.wave_differentials(res, abi.INTERSECT_OBJ, wis, aux=aux, want_cols=True)
    again = eng.wave_differentials(res, abi.INTERSECT_OBJ, wis, aux=aux, want_cols=True)
    raw = eng.wave_differentials(res, abi.INTERSECT_OBJ, wis, aux=aux, on_device=True)
    host = [out[0], *out[1:4]]
    for a, b in zip(host, again[:4]):
        assert a.tobytes() == b.tobytes(), 'two identical calls differ'
    same_bits(out[4].cpu().numpy(), again[4].cpu().numpy(), 'cols of two calls')
    assert records_view(raw[0], WD_ITEM_DTYPE).tobytes() == out[0].tobytes()
    for a, b in zip(host[1:], raw[1:4]):
        assert a.tobytes() == b.cpu().numpy().tobytes(), 'host and device destinations differ'
    for i in range(3):
        one = eng.wave_differentials(res[i], abi.INTERSECT_OBJ, wis[i:i + 1], aux=aux[i:i + 1].contiguous())
        for a, b in zip(host, one[:4]):
            assert a[i:i + 1].tobytes() == b.tobytes(), f'item {i}: one call of three != its own call'
    eng.close()


def test_the_cap_and_the_scratch_bound(torch):
    """the 44-interface workload with 28 aux rows: 512 columns, 65 rays.  Six items need more than
    the 32 MiB of one launch's scratch (6.6 MB each: a chunk record and the running record of 528^2
    doubles, the 512^2 of gram): the job runs as two launches of five and one items and gives
    each item the bits of its own call"""
    from rayoptics_amd.engine import TraceEngine
    wl = workloads.load('litho_c5')
    table = wl.table
    eng = TraceEngine(table)
    n_seg = eng.num_segments(abi.INTERSECT_OBJ)
    n_aux, R, items = abi.MAX_WD_COLS - 11 * n_seg, 65, 6
    assert n_seg == 44 and n_aux == 28
    cases = [synthetic(n_seg, R, 900 + i, n_aux) for i in range(items)]
    res = [upload(eng, s, st, fs) for s, st, fs, _a in cases]
    aux = torch.from_numpy(np.stack([c[3] for c in cases])).to(eng.device)
    wis = [i % len(table.wvls) for i in range(items)]
    out = eng.wave_differentials(res, abi.INTERSECT_OBJ, wis, aux=aux, want_cols=True)
    cols = out[4].cpu().numpy()
    worst = {}
    for i in (0, items - 1):
        seg, st, _fs, a = cases[i]
        check_item((*out[:4], cols), i, table, abi.INTERSECT_OBJ, seg, st, wis[i], None, a, f'cap item {i}', worst)
    print('largest error / bound:', {k: f'{v:.3g}' for k, v in worst.items()})
    for i in (0, 3, items - 1):
        one = eng.wave_differentials(res[i], abi.INTERSECT_OBJ, wis[i:i + 1], aux=aux[i:i + 1].contiguous())
        for a, b in zip(out[:4], one[:4]):
            assert a[i:i + 1].tobytes() == b.tobytes(), f'item {i}: the split job differs from its own call'
    with pytest.raises(Exception, match='n_cols'):
        eng.wave_differentials(res[0], abi.INTERSECT_OBJ, wis[:1],
                               aux=torch.zeros((1, n_aux + 1, R), dtype=torch.float64, device=eng.device))
    eng.close()


def test_traced_packets_and_the_telescoping_identity(torch):
    """double Gauss packets traced on the device: the columns are the restatement's bits, and over
    all slots the shift columns sum to n0*d0 of the object slot -- a rigid shift of lens and image
    under the incoming beam is a piston.  The tolerance is the restatement's own residual on the
    same packets times 4."""
    from rayoptics_amd.engine import TraceEngine
    wl = workloads.load('dblgauss_c2')
    table = wl.table
    eng = TraceEngine(table)
    flds, wis = [wl.fields[0], wl.fields[2], wl.fields[2]], [1, 0, 2]
    results = trace_packets(eng, SPOT, flds, wis, 33)
    host = host_of(results, ('seg', 'status'))
    out = eng.wave_differentials(results, SPOT, wis, want_cols=True)
    cols = out[4].cpu().numpy()
    n_seg = eng.num_segments(SPOT)
    worst = {}
    for i, (seg, st) in enumerate(host):
        ref = check_item((*out[:4], cols), i, table, SPOT, seg, st, wis[i], None, np.zeros((0, st.shape[0])),
                         f'traced item {i}', worst)
        assert 0 < ref['n'] <= 33 * 33
        ok = st == abi.OK
        ref_cols, _c, _b = WR.columns(table, SPOT, seg, st, wis[i])
        n0 = abs(float(np.asarray(table.n_table)[wis[i]][0]))
        for c in range(3):
            want = n0 * seg[0, 3 + c][ok]

            def residual(cc):
                total = np.zeros(int(ok.sum()))
                for k in range(n_seg):
                    total = total + cc[11 * k + c][ok]
                return np.abs(total - want).max()

            tol = 4 * residual(ref_cols)
            got = residual(cols[i])
            print(f'item {i} axis {c}: telescoping residual {got:.3g} (restatement {tol / 4:.3g})')
            assert got <= tol and tol < 1e-14
    print('largest error / bound:', {k: f'{v:.3g}' for k, v in worst.items()})
    eng.close()


# ---- analyses.tolerance_sensitivity against re-traced perturbed models ----------------------
def fixture_model(perturb=None):
    """the double Gauss of tests/golden/through_focus_map.npz as a table model whose focus planes
    carry the reference's own rox_wavefront constants; ``perturb(table)`` replaces its table
    before any engine is made for it (the constants stay the nominal ones)"""
    import ctypes as C
    import focus_map_fixture as FM
    m = FM.FocusMapFixtureModel(FM.load(), 'dblgauss')
    if perturb is not None:
        tbl = m.seq_model.surface_table
        new = perturb(tbl)
        C.memmove(tbl.rows, new.rows, C.sizeof(tbl.rows))
        tbl.n_table[:] = new.n_table
    return m


def test_tolerance_sensitivity_against_retraced_models(torch):
    """the RMS wavefront predicted for an element decentre, a surface tilt and an index change, with
    and without the focus compensator, against the OPD grid of the re-traced perturbed model (its
    aux column 0: the through-focus launch of the perturbed table with the nominal constants).
    The margin is what first order leaves out, measured on the CPU oracle
    (tests/test_wavediff_host.py: at most 4.9e-3 of the largest |dW| over the pupil, which is the margin).
    Seen on the device: |predicted - re-traced| <= 3.9e-3 waves of 4.4 .. 7.3, margins 0.017 .. 0.031."""
    from rayoptics_amd import analyses, session, tolerance
    from wavediff_ref import FIRST_ORDER_MARGIN
    num = 16
    m = fixture_model()
    foc = m.focs[int(np.argmin(np.abs(m.focs)))]
    kw = dict(wvls=m.wvls, num_rays=num, foc=foc, keep_cols=True)
    cases = [('decentre', lambda p: p.element_decenter(3, 5, 'y'), 0.02, lambda t: WR.shifted_group(t, 3, 5, (0, 0.02, 0))),
             ('tilt', lambda p: p.surface_tilt(7, 'x'), 3e-4, lambda t: WR.moved(t, 7, alpha=(3e-4, 0, 0))),
             ('index', lambda p: p.index(10), 5e-4, lambda t: WR.indexed(t, 10, None, 5e-4))]

    def tols(p):
        return [tolerance.Tolerance(name, make(p), mag) for name, make, mag, _t in cases]

    ts = analyses.tolerance_sensitivity(m, tolerances=tols, compensators=('focus',), flds=m.fields, **kw)
    q = ts.quadratic
    F, W = q.F, q.W
    assert ts.rms_plus.shape == (3, F) and ts.comp_plus.shape == (3, 1) and ts.image_shift.shape == (3, F, 2)
    cols = ts.cols.cpu().numpy()                                          # [F*W, n_cols, R]
    pert = tolerance.Perturbations(session.engine_for(m).table, None, 3, [0] * (F * W))
    focus_col = pert.col(-1, 'dz')
    rms0, mc0 = ts.monte_carlo(200, seed=11)
    rms1, mc1 = ts.monte_carlo(200, seed=11)
    assert np.array_equal(rms0, rms1) and np.array_equal(mc0, mc1) and rms0.shape == (200, F)
    assert np.isfinite(rms0).all() and (ts.rss() >= ts.nominal_compensated).all()

    def poly_rms(wmaps, c=0.0):
        """[F] the polychromatic RMS of per-item maps [F*W, R] (NaN: not counted) plus c times the
        focus column, each item's piston removed"""
        out = np.zeros(F)
        for i in range(F * W):
            v = wmaps[i] + c * (-q.ws[i // W, i % W]) * cols[i, focus_col]
            v = v[np.isfinite(v)]
            out[i // W] += q.sw[i % W] * v.var()
        return np.sqrt(out)

    assert np.allclose(poly_rms(cols[:, 0]), ts.nominal_rms, rtol=1e-9)
    for k, (name, _make, mag, perturb) in enumerate(cases):
        m2 = fixture_model(perturb)
        ts2 = analyses.tolerance_sensitivity(m2, tolerances=tols, compensators=(), flds=m2.fields, **kw)
        true = ts2.cols.cpu().numpy()[:, 0]                                # the re-traced OPD, waves
        dw = np.stack([mag * (q.A[i // W, i % W, :, 1 + k] @ cols[i]) for i in range(F * W)])
        big = max(float(np.nanmax(np.abs(dw[i] - np.nanmean(dw[i])))) for i in range(F * W))
        margin = FIRST_ORDER_MARGIN * big
        e = np.zeros(3)
        e[k] = mag
        plain = q.rms(e, np.zeros(1))
        got = poly_rms(true)
        print(f'{name}: largest |dW| {big:.4g} waves, margin {margin:.3g}; RMS per field predicted {plain} '
              f're-traced {got}')
        assert np.isfinite(got).all() and (np.abs(plain - got) <= margin).all(), (name, plain, got, margin)
        # compensated: the focus motion that minimises the field-weighted mean square of the re-traced maps
        cs = np.linspace(-1.0, 1.0, 3)
        ms = np.array([(q.fw * poly_rms(true, c) ** 2).sum() for c in cs])
        a, b, _c0 = np.polyfit(cs, ms, 2)
        c_true = -b / (2 * a)
        got_c = poly_rms(true, c_true)
        print(f'{name}: compensated RMS predicted {ts.rms_plus[k]} (focus {ts.comp_plus[k, 0]:.5g}) re-traced '
              f'{got_c} (focus {c_true:.5g})')
        assert (np.abs(ts.rms_plus[k] - got_c) <= margin).all(), (name, ts.rms_plus[k], got_c, margin)
    # a pupil map of one perturbation's wavefront change, from the kept columns
    dm = ts.delta_map(1, 0)
    assert dm.shape == (num, num) and np.isfinite(dm).sum() == int(ts.item['n'][0])
    session.clear()


# ---- several chunks, ranges of rays, groups of chunks, and columns bound for host memory -----
def late(case, dead):
    """the rays before ``dead`` fail: the pivot lies in a later chunk"""
    seg, st, fs, aux = case
    st[:dead] = abi.BLOCKED
    seg[:, :, :dead] = np.nan
    aux[:, :dead] = np.nan
    return seg, st, fs, aux


def raw_call(eng, res, wis, aux, cols_ptr, ld_cols, n_cols):
    """rox_wave_differentials through ctypes with host item, pivot, sums and gram -> (item, pivot, sums, gram)"""
    from rayoptics_amd.engine import WD_ITEM_DTYPE
    n = len(res)
    outs = (abi.Out * n)(*[r.out_struct() for r in res])
    wi = np.asarray(wis, np.int32)
    item = np.zeros(n, WD_ITEM_DTYPE)
    pivot, sums, gram = np.zeros((n, n_cols)), np.zeros((n, n_cols)), np.zeros((n, n_cols, n_cols))
    n_aux, ld_aux = int(aux.shape[1]), int(aux.shape[2])
    rc = eng.lib.rox_wave_differentials(eng._handle, abi.INTERSECT_OBJ, n, outs, int(res[0].R), wi.ctypes.data,
                                        eng.num_segments(abi.INTERSECT_OBJ), None, n_aux, aux.data_ptr(),
                                        n_aux * ld_aux, ld_aux, cols_ptr, ld_cols, item.ctypes.data,
                                        pivot.ctypes.data, sums.ctypes.data, gram.ctypes.data, None)
    assert rc == 0, eng.lib.rox_last_error().decode()
    return item, pivot, sums, gram


def test_ranges_of_rays_and_host_columns(torch):
    """24577 rays, 71 columns: 49 chunks of 512 rays.  Without device ``cols`` the columns pass
    through the scratch 28 chunks (14336 rays) at a time (two ranges; the pivot, ray 15000 or
    later, lies in the second); with them the walk is one range.  ``cols`` in host memory with ld_cols > n_rays
    arrive a range at a time.  All three give the same bits, the restatement's where those are
    promised."""
    from rayoptics_amd.engine import TraceEngine
    n_ifcs, R, n_aux, items = 6, 24577, 5, 2
    table = varied_table(n_ifcs)
    eng = TraceEngine(table)
    cases = [late(synthetic(n_ifcs, R, 40 + i, n_aux), 15000 + 17 * i) for i in range(items)]
    res = [upload(eng, s, st, fs) for s, st, fs, _a in cases]
    aux = torch.from_numpy(np.stack([c[3] for c in cases])).to(eng.device)
    wis, n_cols = [1, 2], 71
    lean = eng.wave_differentials(res, abi.INTERSECT_OBJ, wis, aux=aux)
    kept = eng.wave_differentials(res, abi.INTERSECT_OBJ, wis, aux=aux, want_cols=True)
    for a, b in zip(lean[:4], kept[:4]):
        assert a.tobytes() == b.tobytes(), 'two ranges through the scratch differ from one range'
    dev_cols = kept[4].cpu().numpy()
    worst = {}
    for i in range(items):
        seg, st, _fs, a = cases[i]
        ref = check_item((*kept[:4], dev_cols), i, table, abi.INTERSECT_OBJ, seg, st, wis[i], None, a,
                         f'49 chunks item {i}', worst)
        assert ref['pivot_ray'] >= 15000 and ref['n'] > 6000
    print('largest error / bound:', {k: f'{v:.3g}' for k, v in worst.items()})
    # columns bound for host memory, rows longer than the rays: the padding stays as it was
    ld = R + 7
    host_cols = np.full((items, n_cols, ld), -7.25)
    out = raw_call(eng, res, wis, aux, host_cols.ctypes.data, ld, n_cols)
    assert (host_cols[:, :, R:] == -7.25).all()
    same_bits(host_cols[:, :, :R], dev_cols, 'host cols against device cols')
    for a, b in zip(kept[:4], out):
        assert a.tobytes() == b.tobytes(), 'host cols: the records differ'
    eng.close()


def test_groups_of_chunks(torch):
    """the 44-interface workload at the cap of 512 columns with 24577 rays in 49 chunks: a chunk record
    is 2.2 MB, so the chunks go onto the running record in groups of three -- with device ``cols``
    all 49 of one range, without them in ranges of four chunks (groups of three and one).  The same bits; the columns, the records and
    the pivot (in a later range) are the restatement's, sums and a 40-column block of gram
    within the any-order bound."""
    from rayoptics_amd.engine import TraceEngine
    wl = workloads.load('litho_c5')
    table = wl.table
    eng = TraceEngine(table)
    n_seg, R, n_aux = 44, 24577, 28
    seg, st, fs, a = late(synthetic(n_seg, R, 77, n_aux), 7000)
    res = [upload(eng, seg, st, fs)]
    aux = torch.from_numpy(a[None]).to(eng.device)
    kept = eng.wave_differentials(res, abi.INTERSECT_OBJ, [3], aux=aux, want_cols=True)
    lean = eng.wave_differentials(res, abi.INTERSECT_OBJ, [3], aux=aux)
    for x, y in zip(lean[:4], kept[:4]):
        assert x.tobytes() == y.tobytes(), 'groups of chunks differ from single chunks'
    item, pivot, sums, gram, cols = kept
    ref_cols, counted, n_bad = WR.columns(table, abi.INTERSECT_OBJ, seg, st, 3, None, a)
    same_bits(cols[0].cpu().numpy(), ref_cols, 'cols')
    idx = np.flatnonzero(counted)
    assert (int(item['n'][0]), int(item['n_bad'][0]), int(item['pivot_ray'][0])) == (idx.size, n_bad, int(idx[0]))
    assert idx[0] >= 7000
    same_bits(pivot[0], ref_cols[:, idx[0]], 'pivot')
    assert np.array_equal(gram[0], gram[0].T)
    dev = (ref_cols[:, idx] - ref_cols[:, idx[:1]]).astype(np.longdouble)
    n = idx.size
    err = np.abs(sums[0].astype(np.longdouble) - dev.sum(axis=1)).astype(np.float64)
    assert (err <= ((n + 4) * U * np.abs(dev).sum(axis=1)).astype(np.float64)).all(), 'sums beyond their bound'
    sel = np.r_[0:8, 90:106, 496:512]                       # both sides of panel edges, the last tile
    g, ab = dev[sel] @ dev[sel].T, np.abs(dev[sel]) @ np.abs(dev[sel]).T
    err = np.abs(gram[0][np.ix_(sel, sel)].astype(np.longdouble) - g).astype(np.float64)
    bound = ((n + 4) * U * ab).astype(np.float64)
    print(f'gram block: largest error / bound {(err / np.where(bound > 0, bound, np.inf)).max():.3g}')
    assert (err <= bound).all(), 'gram beyond its bound'
    eng.close()
