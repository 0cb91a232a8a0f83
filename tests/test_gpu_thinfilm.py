"""rox_surface_thinfilm on the device against the NumPy restatement (tests/thinfilm_ref.py: the
recursive Airy summation and a complex field carry, not the product's characteristic matrix) run on
the same packets copied to the host.  The device's sincos / exp / sqrt are not NumPy's, so rows are
compared within thinfilm_ref.ROW_BOUND, ten times the largest error measured over the cases below;
sums within n * 2^-53 relative of math.fsum of the restatement's values plus n times that bound;
counts, NaN patterns and n_ok exactly.  Grids are 15 x 15 rays as in tests/test_gpu_transmission.py
(a ragged last wave), one case also at 33 x 33 (three tiles of 512 rays, the last ragged)."""
import functools

import numpy as np
import pytest

import fresnel_ref as FR
import packets_fixture
import thinfilm_ref as TR
from helpers import bit_equal
from packets_fixture import torch  # noqa: F401 (the fixture)
from rayoptics_amd import abi, coatings, workloads
from rayoptics_amd.coatings import Coating
from test_gpu_transmission import CENTRE, NUM, SPOT, case
from thinfilm_ref import EPS, ROW_BOUND

pytestmark = pytest.mark.gpu

host_of = functools.partial(packets_fixture.host_of, want=('seg', 'status'))
AL = 0.96 + 6.7j


def metal(wvl):
    """an aluminium-like metal with dispersion"""
    return complex(0.4 + wvl / 1000.0, 3.0 + wvl / 150.0)


def glass_ifcs(table, air_only=True):
    """the refracting interfaces between object and image (with ``air_only`` those with air on
    exactly one side) and whether the air comes first"""
    nt = np.asarray(table.n_table)
    out = []
    for i in range(1, table.n_ifcs - 1):
        row = table.rows[i]
        a0, a1 = bool((nt[:, i - 1] == 1.0).all()), bool((nt[:, i] == 1.0).all())
        if row.mode == abi.TRANSMIT and row.profile != abi.THINLENS and row.ph.kind == abi.PH_NONE \
                and (nt[:, i - 1] != nt[:, i]).any() and (a0 != a1 or not air_only):
            out.append((i, a0))
    return out


def stacks_of(name, table):
    """{interface: Coating in crossing order} of a case"""
    if name.startswith('dblgauss'):
        one = Coating([(1.38, 99.6)])
        four = Coating([(1.38, 95.0), (2.1, 60.0), (1.62, 40.0), (lambda w: 1.46 + (550.0 - w) * 2e-4, 110.0)])
        g = glass_ifcs(table)
        assert len(g) == 8 and len(glass_ifcs(table, False)) == 10          # two cemented surfaces stay bare
        return {i: (four if k in (1, 6) else one) if air else (four if k in (1, 6) else one).reversed()
                for k, (i, air) in enumerate(g)}
    if name.startswith('rc_telescope'):
        return {i: Coating([(1.46, 100.0)], substrate=metal) for i, r in enumerate(table.rows) if r.mode == abi.REFLECT}
    if name == 'cell_phone':
        two = Coating([(1.38, 90.0), (1.7, 70.0)])
        return {i: two if air else two.reversed() for i, air in glass_ifcs(table)}
    three = Coating([(1.38, 100.0), (2.0 + 0.05j, 30.0), (1.62, 80.0)])
    return {i: three if air else three.reversed() for i, air in glass_ifcs(table)}


def film_args(table, stacks, kind=None, value=None):
    """the keyword arguments of surface_thinfilm and thinfilm_ref's description of the same stacks"""
    N = table.n_ifcs
    kind = np.zeros(N, np.int32) if kind is None else np.array(kind, np.int32)
    value = np.ones((N, 2)) if value is None else np.array(value, np.float64)
    for i in stacks:
        kind[i] = abi.COAT_STACK
    first, thick, index, sub = coatings.stack_tables(table, stacks)
    kw = dict(coat_kind=kind, coat_value=value, stack_first=first, layer_thickness=thick, layer_index=index,
              sub_index=sub)
    return kw, TR.stack_dict(first, thick, index, sub)


def check_item(table, flags, seg, status, wi, kw, stack, rows, surf, item, what, bound=ROW_BOUND):
    """one item against the restatement -> the largest row error"""
    a = TR.thinfilm(table, flags, seg, status, wi, table.wvls[wi], kw['coat_kind'], kw['coat_value'], stack,
                    fields=rows.shape[0] == 16)
    assert np.array_equal(np.isnan(rows), np.isnan(a['rows'])), f'{what}: NaN pattern'
    ok = a['ok']
    worst = float(np.abs(rows[:, ok] - a['rows'][:, ok]).max()) if ok.any() else 0.0
    print(f'{what}: largest row error {worst:.3g} ({worst / EPS:.1f} * 2^-53), bound {bound:.3g}')
    assert worst <= bound, what
    ref_s, ref_i = TR.records(a)
    n = ref_i['n_ok']
    assert int(item['n_ok']) == n and int(item['n_rays']) == status.shape[0] and np.array_equal(surf['n'], ref_s['n'])
    if n:
        for name in ('ts_min', 'tp_min', 'ci_min'):
            assert np.abs(surf[name] - ref_s[name]).max() <= bound, (what, name)
        for name in ('t_min', 't_max', 'd_max'):
            assert abs(float(item[name]) - ref_i[name]) <= bound, (what, name)
    for name in ('ts_sum', 'tp_sum', 't_sum', 'ci_sum'):
        assert (np.abs(surf[name] - ref_s[name]) <= n * EPS * ref_s[name] + n * bound).all(), (what, name)
    for name in ('t_sum', 't1_sum', 't2_sum', 'd_sum'):
        assert abs(float(item[name]) - ref_i[name]) <= n * EPS * ref_i[name] + n * bound, (what, name)
    return worst, a


@pytest.mark.parametrize('name,num', [('dblgauss_c2', NUM), ('rc_telescope_c4', NUM), ('cell_phone', NUM),
                                      ('tilted', NUM), ('tilted_filtered', NUM), ('dblgauss_c2', 33)])
def test_against_the_restatement(torch, name, num):
    from rayoptics_amd.engine import TraceEngine
    table, flags, flds, wis = case(name)
    eng = TraceEngine(table)
    results = packets_fixture.trace_packets(eng, flags, flds, wis, num)
    host = host_of(results)
    stacks = stacks_of(name, table)
    assert stacks
    kw, stack = film_args(table, stacks)
    rows, surf, item = eng.surface_thinfilm(results, flags, wis, [table.wvls[w] for w in wis], fields=True, **kw)
    n_seg = eng.num_segments(flags)
    assert rows.shape == (len(flds), 16, num * num) and surf.shape == (len(flds), n_seg)
    worst, n_ok = 0.0, 0
    for i, (seg, st) in enumerate(host):
        w, a = check_item(table, flags, seg, st, wis[i], kw, stack, rows[i], surf[i], item[i], f'{name} item {i}')
        worst, n_ok = max(worst, w), n_ok + int(a['ok'].sum())
    print(f'{name} at {num} x {num}: largest row error {worst:.3g}')
    assert n_ok >= 100
    assert np.nanmax(np.abs(rows[:, 10:16])) > 1e-3             # the stacks turn the phase: complex fields
    if name == 'rc_telescope_c4':
        assert (surf['t_sum'][:, 1:3] < 0.95 * surf['n'][:, 1:3]).all()      # metal mirrors cost light
    eng.close()


def test_no_stack_is_the_old_entry_bit_for_bit(torch):
    from rayoptics_amd.engine import TraceEngine
    for name, over in (('dblgauss_c2', {1: (abi.COAT_IDEAL, 1.0, 1.0), 2: (abi.COAT_FIXED, 0.9, 0.8),
                                        4: (abi.COAT_FIXED, 0.97, 0.97)}),
                       ('rc_telescope_c4', {1: (abi.COAT_FIXED, 0.9, 0.8), 2: (abi.COAT_IDEAL, 1.0, 1.0)}),
                       ('tilted_filtered', {})):
        table, flags, flds, wis = case(name)
        N = table.n_ifcs
        eng = TraceEngine(table)
        results = packets_fixture.trace_packets(eng, flags, flds, wis, NUM)
        kind, value = np.zeros(N, np.int32), np.ones((N, 2))
        for i, (k, ts, tp) in over.items():
            kind[i], value[i] = k, (ts, tp)
        old = eng.surface_transmission(results, flags, wis, coat_kind=kind, coat_value=value, fields=True)
        new = eng.surface_thinfilm(results, flags, wis, None, coat_kind=kind, coat_value=value, fields=True)
        bit_equal(new[0][:, :10], old[0], f'{name}: real rows')
        assert new[1].tobytes() == old[1].tobytes() and new[2].tobytes() == old[2].tobytes(), name
        ok = ~np.isnan(old[0][:, 0])
        im = new[0][:, 10:16]
        assert ok.any() and (im.transpose(0, 2, 1)[ok] == 0.0).all() and np.isnan(im.transpose(0, 2, 1)[~ok]).all()
        four = eng.surface_thinfilm(results, flags, wis, coat_kind=kind, coat_value=value)
        assert four[0].tobytes() == old[0][:, :4].tobytes()
        if not over:
            none = eng.surface_thinfilm(results, flags, wis, fields=True)
            assert none[0].tobytes() == new[0].tobytes() and none[2].tobytes() == new[2].tobytes()
            # a stack without layers on every refracting surface is the bare surface
            kw, _st = film_args(table, {i: Coating([]) for i, _air in glass_ifcs(table, False)})
            zero = eng.surface_thinfilm(results, flags, wis, [table.wvls[w] for w in wis], fields=True, **kw)
            assert np.array_equal(np.isnan(zero[0]), np.isnan(new[0]))
            err = np.nanmax(np.abs(zero[0] - new[0]))
            print(f'{name}: zero-layer stacks against bare rows: {err:.3g}')
            assert err <= ROW_BOUND and np.array_equal(zero[2]['n_ok'], new[2]['n_ok'])
        eng.close()


def test_quarter_and_half_wave_layers_on_the_axial_ray(torch):
    from rayoptics_amd.engine import TraceEngine
    wl = workloads.load('dblgauss_c2')
    table = wl.table
    eng = TraceEngine(table)
    results = packets_fixture.trace_packets(eng, SPOT, [wl.fields[0]], [1], NUM, span=0.875)
    seg, st = host_of(results)[0]
    assert st[CENTRE] == abi.OK and seg[0, 3:6, CENTRE].tolist() == [0.0, 0.0, 1.0]
    wvl, nt = table.wvls[1], table.n_table[1]
    g = [i for i, _a in glass_ifcs(table, False)]
    assert len(g) == 10
    n1 = 1.38
    want_q = want_h = 1.0
    for i in g:
        want_q *= 1.0 - ((nt[i - 1] * nt[i] - n1 * n1) / (nt[i - 1] * nt[i] + n1 * n1)) ** 2
        want_h *= 4.0 * nt[i - 1] * nt[i] / (nt[i - 1] + nt[i]) ** 2
    tol = ROW_BOUND + FR.CLOSED * len(g)                # against a product of closed forms; D and T1 - T2 have none
    for c, want in ((Coating.quarter_wave(n1, wvl), want_q), (Coating([(n1, wvl / (2.0 * n1))]), want_h)):
        kw, _stack = film_args(table, {i: c for i in g})
        rows, _s, _i = eng.surface_thinfilm(results, SPOT, [1], [wvl], **kw)
        T, T1, T2, D = rows[0, :, CENTRE]
        print(f'axial ray, {c!r}: T {T!r} closed form {want!r} error {abs(T - want):.3g} D {D:.3g} (bound {tol:.3g})')
        assert abs(T - want) <= tol and D <= ROW_BOUND and abs(T1 - T2) <= ROW_BOUND
    bare, _s, _i = eng.surface_transmission(results, SPOT, [1])
    assert abs(rows[0, 0, CENTRE] - bare[0, 0, CENTRE]) <= tol and want_q > want_h + 0.2
    eng.close()


def test_a_micrometre_of_metal_and_the_perfect_conductor(torch):
    from rayoptics_amd.engine import TraceEngine
    table, flags, flds, wis = case('rc_telescope_c4')
    eng = TraceEngine(table)
    results = packets_fixture.trace_packets(eng, flags, flds, wis, NUM)
    wv = [table.wvls[w] for w in wis]
    mirrors = [i for i, r in enumerate(table.rows) if r.mode == abi.REFLECT]
    kw, _st = film_args(table, {i: Coating([(AL, 1000.0)], substrate=1.52) for i in mirrors})
    film = eng.surface_thinfilm(results, flags, wis, wv, fields=True, **kw)
    kw, _st = film_args(table, {i: Coating([], substrate=AL) for i in mirrors})
    bulk = eng.surface_thinfilm(results, flags, wis, wv, fields=True, **kw)
    ok = ~np.isnan(bulk[0][:, 0])
    assert ok.sum() >= 100 and np.array_equal(np.isnan(film[0]), np.isnan(bulk[0]))
    assert np.isfinite(film[0].transpose(0, 2, 1)[ok]).all()
    err = np.nanmax(np.abs(film[0] - bulk[0]))
    print(f'1000 nm of metal against the bulk metal: {err:.3g}')
    assert err <= ROW_BOUND and 0.80 < np.nanmean(bulk[0][:, 0]) < 0.88      # two aluminium mirrors: 0.92^2
    # sub_index = (0, 1e8): the ideal mirror's (-1, +1), the fields of rox_surface_transmission
    kw, _st = film_args(table, {i: Coating([], substrate=1e8j) for i in mirrors})
    pec = eng.surface_thinfilm(results, flags, wis, wv, fields=True, **kw)
    ideal = eng.surface_transmission(results, flags, wis, fields=True)
    err = np.nanmax(np.abs(pec[0][:, :10] - ideal[0]))
    im = np.nanmax(np.abs(pec[0][:, 10:]))
    print(f'perfect conductor against the ideal mirror: {err:.3g}, imaginary parts {im:.3g}')
    assert err <= 1e-6 and im <= 1e-6
    eng.close()


def test_repeats_destinations_and_grouping(torch):
    from rayoptics_amd.engine import TX_ITEM_DTYPE, TX_SURFACE_DTYPE, TraceEngine, tx_view
    table, flags, flds, wis = case('dblgauss_c2')
    eng = TraceEngine(table)
    results = packets_fixture.trace_packets(eng, flags, flds, wis, NUM)
    kw, _st = film_args(table, stacks_of('dblgauss_c2', table))
    wv = [table.wvls[w] for w in wis]
    rows, surf, item = eng.surface_thinfilm(results, flags, wis, wv, fields=True, **kw)
    again = eng.surface_thinfilm(results, flags, wis, wv, fields=True, **kw)
    assert all(x.tobytes() == y.tobytes() for x, y in zip((rows, surf, item), again)), 'a repeat differs'
    drows, dsurf, ditem = eng.surface_thinfilm(results, flags, wis, wv, fields=True, on_device=True, **kw)
    assert drows.cpu().numpy().tobytes() == rows.tobytes(), 'device rows differ from host rows'
    assert tx_view(dsurf, TX_SURFACE_DTYPE).tobytes() == surf.tobytes()
    assert tx_view(ditem, TX_ITEM_DTYPE).tobytes() == item.tobytes()
    for i, r in enumerate(results):
        r1, s1, i1 = eng.surface_thinfilm(r, flags, wis[i:i + 1], wv[i:i + 1], fields=True, **kw)
        assert r1.tobytes() == rows[i:i + 1].tobytes() and s1.tobytes() == surf[i:i + 1].tobytes(), f'item {i}'
        assert i1.tobytes() == item[i:i + 1].tobytes(), f'item {i}'
    none, s0, i0 = eng.surface_thinfilm(results, flags, wis, wv, want_rows=False, **kw)
    assert none is None and s0.tobytes() == surf.tobytes() and i0.tobytes() == item.tobytes()
    r4, s4, i4 = eng.surface_thinfilm(results, flags, wis, wv, **kw)
    assert r4.tobytes() == rows[:, :4].tobytes() and s4.tobytes() == surf.tobytes() and i4.tobytes() == item.tobytes()
    eng.close()


def test_split_launches_equal_one_launch(torch):
    """3 items x 600^2 rays with rows bound for host memory: the rows pass through the scratch a
    range of rays at a time and the items run as two launches; the same bits as device destinations
    (one launch) and as an item's own call"""
    from rayoptics_amd.engine import TX_ITEM_DTYPE, TX_SURFACE_DTYPE, TraceEngine, tx_view
    table, flags, flds, wis = case('dblgauss_c2')
    flds, wis = flds[:3], wis[:3]
    eng = TraceEngine(table)
    results = packets_fixture.trace_packets(eng, flags, flds, wis, 600)
    kw, _st = film_args(table, stacks_of('dblgauss_c2', table))
    wv = [table.wvls[w] for w in wis]
    rows, surf, item = eng.surface_thinfilm(results, flags, wis, wv, **kw)
    drows, dsurf, ditem = eng.surface_thinfilm(results, flags, wis, wv, on_device=True, **kw)
    assert drows.cpu().numpy().tobytes() == rows.tobytes()
    assert tx_view(dsurf, TX_SURFACE_DTYPE).tobytes() == surf.tobytes()
    assert tx_view(ditem, TX_ITEM_DTYPE).tobytes() == item.tobytes()
    r1, s1, i1 = eng.surface_thinfilm(results[2], flags, wis[2:], wv[2:], **kw)
    assert r1.tobytes() == rows[2:].tobytes() and s1.tobytes() == surf[2:].tobytes() and i1.tobytes() == item[2:].tobytes()
    assert int(item[2]['n_rays']) == 600 * 600 and 0 < int(item[2]['n_ok']) < 600 * 600
    eng.close()


def test_argument_errors_leave_the_outputs_untouched(torch):
    from helpers import phase_table
    from rayoptics_amd.table import field_struct
    from rayoptics_amd.engine import EngineError, TX_ITEM_DTYPE, TX_SURFACE_DTYPE, TraceEngine, load_library
    lib = load_library()
    table, flags, flds, wis = case('rc_telescope_c4')
    eng = TraceEngine(table)
    results = packets_fixture.trace_packets(eng, flags, flds, wis, NUM)
    R, N, n_seg = NUM * NUM, table.n_ifcs, eng.num_segments(flags)
    kw, _st = film_args(table, {1: Coating([(1.46, 100.0)], substrate=AL)})
    with pytest.raises(EngineError, match='wvls_nm'):
        eng.surface_thinfilm(results, flags, wis, [550.0], **kw)
    with pytest.raises(EngineError, match='layers need wvls_nm'):
        eng.surface_thinfilm(results, flags, wis, None, **kw)
    with pytest.raises(EngineError, match='layer_thickness'):
        eng.surface_thinfilm(results, flags, wis, [550.0, 550.0], **dict(kw, layer_thickness=[1.0, 2.0]))
    with pytest.raises(EngineError, match='sub_index'):
        eng.surface_thinfilm(results, flags, wis, [550.0, 550.0], **dict(kw, sub_index=np.ones((1, 3, 2))))
    with pytest.raises(EngineError, match='stack_first'):
        eng.surface_thinfilm(results, flags, wis, [550.0, 550.0], **dict(kw, stack_first=[0, 1]))

    good = [r.out_struct() for r in results]
    rows = np.zeros((2, 4, R))
    surf = np.zeros((2, n_seg), TX_SURFACE_DTYPE)
    item = np.zeros(2, TX_ITEM_DTYPE)

    def call(handle=None, n=N, outs=None, n_rays=R, trace_flags=flags, surf=surf, **over):
        a = dict(wvl=[550.0, 550.0], kind=kw['coat_kind'], value=np.ones((n, 2)), first=kw['stack_first'],
                 thick=kw['layer_thickness'], index=kw['layer_index'], sub=kw['sub_index'])
        a.update(over)
        rows[:] = 7.0
        surf['n'] = -7
        item['n_ok'] = -7
        keep = [None if v is None else np.ascontiguousarray(v, dtype=t) for v, t in (
            (a['wvl'], np.float64), (a['kind'], np.int32), (a['value'], np.float64), (a['first'], np.int32),
            (a['thick'], np.float64), (a['index'], np.float64), (a['sub'], np.float64))]
        p = [None if v is None else v.ctypes.data for v in keep]
        w = np.zeros(2, np.int32)
        rc = lib.rox_surface_thinfilm(handle or eng._handle, trace_flags, 0, 2, outs or (abi.Out * 2)(*good), n_rays,
                                      w.ctypes.data, p[0], n, p[1], p[2], p[3], p[4], p[5], p[6], rows.ctypes.data,
                                      R, surf.ctypes.data, item.ctypes.data, None)
        return rc, lib.rox_last_error().decode()

    def kinds(*stacked):
        k = np.zeros(N, np.int32)
        k[list(stacked)] = abi.COAT_STACK
        return k

    no_layers = dict(first=np.zeros(N + 1, np.int32), thick=None, index=None)
    bad_sub = kw['sub_index'].copy()
    bad_sub[0, 1] = (0.0, 0.0)
    bad_index = kw['layer_index'].copy()
    bad_index[0, 0, 1] = -0.1
    cases = [(dict(kind=kinds(0), **no_layers), 'coat_kind[0]'),                  # the object: a dummy interface
             (dict(kind=kinds(3), **no_layers), 'coat_kind[3]'),                  # a dummy interface behind the mirrors
             (dict(sub=None), 'coat_kind[1]: a stack on a ROX_REFLECT interface needs sub_index'),
             (dict(sub=bad_sub), 'sub_index[0][1]'), (dict(index=bad_index), 'layer_index[0][0]'),
             (dict(thick=[-1.0]), 'layer_thickness[0]'), (dict(wvl=[550.0, 0.0]), 'item 1: wvl'),
             (dict(first=[0, 0, 65, 65, 65, 65]), 'stack_first[1]'), (dict(n_rays=0), 'n_rays')]
    for over, word in cases:
        rc, msg = call(**over)
        assert rc == -1 and msg.startswith('rox_surface_thinfilm: ') and word in msg, (over, rc, msg)
        assert (rows == 7.0).all() and (surf['n'] == -7).all() and (item['n_ok'] == -7).all(), f'{over}: outputs touched'
    rc, msg = call()
    assert rc == 0, msg
    want = eng.surface_thinfilm(results, flags, [0, 0], [550.0, 550.0], **kw)
    assert rows.tobytes() == want[0].tobytes() and surf.tobytes() == want[1].tobytes() and item.tobytes() == want[2].tobytes()
    eng.close()

    # a stack on a thin lens and on a phase element: systems of their own, with packets of their own
    # traced on them (a check that got lost would show as rc == 0 and overwritten sentinels)
    fld = field_struct([0.0, 0.0, 0.0], (0., 0.), 2.0, 40.0)
    for what in ('thinlens', 'grating'):
        tbl, k = phase_table(np.random.default_rng(3), what)
        assert tbl.rows[k].mode == abi.TRANSMIT
        assert tbl.rows[k].profile == abi.THINLENS if what == 'thinlens' else tbl.rows[k].ph.kind == abi.PH_GRATING
        e2 = TraceEngine(tbl)
        res = packets_fixture.trace_packets(e2, abi.CHECK_APERTURES, [fld, fld], [0, 0], NUM)
        n = tbl.n_ifcs
        kk = np.zeros(n, np.int32)
        kk[k] = abi.COAT_STACK
        surf2 = np.zeros((2, e2.num_segments(abi.CHECK_APERTURES)), TX_SURFACE_DTYPE)
        rc, msg = call(handle=e2._handle, n=n, outs=(abi.Out * 2)(*(r.out_struct() for r in res)),
                       trace_flags=abi.CHECK_APERTURES, surf=surf2, kind=kk, first=np.zeros(n + 1, np.int32),
                       thick=None, index=None, sub=None)
        assert rc == -1 and f'coat_kind[{k}]: a stack belongs on' in msg, (what, rc, msg)
        assert (rows == 7.0).all() and (surf2['n'] == -7).all() and (item['n_ok'] == -7).all(), what
        e2.close()


def test_analysis_with_a_quarter_wave_coating(torch):
    from rayoptics_amd import analyses
    model = workloads.TableModel('dblgauss_c2')
    wvls = list(model.workload.table.wvls)
    kw = dict(flds=model.fields, wvls=wvls, num_rays=NUM)
    bare = analyses.transmission(model, fields=True, **kw)
    c = Coating.quarter_wave(1.38, 550.0)
    tx = analyses.transmission(model, coatings=c, fields=True, **kw)
    assert (tx.poly_T > bare.poly_T).all() and (tx.poly_T > 0.85).all() and (tx.T < 1.0).all()
    assert tx.E1.dtype == np.complex128 and bare.E1.dtype == np.float64 and tx.E1.shape == bare.E1.shape
    assert np.array_equal(np.isnan(tx.T_map), np.isnan(bare.T_map)) and np.nanmax(np.abs(tx.E1.imag)) > 1e-3
    # the coated surfaces no longer lead the losses: the bare cemented ones do not change, the rest drop
    assert [k for k, _i, _l in tx.surface_loss] != [k for k, _i, _l in bare.surface_loss]
    loss, was = {i: l for _k, i, l in tx.surface_loss}, {i: l for _k, i, l in bare.surface_loss}
    coated = [i for i, _air in glass_ifcs(model.workload.table)]
    assert all(loss[i] < 0.5 * was[i] for i in coated) and all(loss[i] == was[i] for i in (4, 8))
    bf = analyses.beam_footprints(model, check_apertures=True, keep_packets=True, **kw)
    shared = analyses.transmission(model, coatings=c, packets=bf, fields=True, **kw)
    assert shared.items.tobytes() == tx.items.tobytes() and shared.surfaces.tobytes() == tx.surfaces.tobytes()
    assert shared.T_map.tobytes() == tx.T_map.tobytes() and shared.E1.tobytes() == tx.E1.tobytes()
    # on a mirror the substrate is the metal: the telescope no longer reports T = 1
    rc = workloads.TableModel('rc_telescope_c4')
    al = Coating([], substrate=AL)
    t = analyses.transmission(rc, flds=rc.fields[:1], wvls=list(rc.workload.table.wvls), num_rays=NUM,
                              coatings={1: al, 2: al})
    assert 0.80 < float(t.T[0, 0]) < 0.88 and float(t.diattenuation_max[0, 0]) > 0.0
