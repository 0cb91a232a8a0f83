"""rox_projected_solid_angle on the device against the NumPy restatement (tests/solidangle_ref.py)
run on the same rows copied to the host: the cells bit for bit, counts, minima and maxima exact,
each sum within n * 2^-53 * sum|terms| of math.fsum of the restatement's terms (a bound that holds
for any order of summation; the largest error over its bound is printed).

Grid sizes: 2 (one cell), 15 (a ragged wave), 64 (exactly one 63-cell strip with its spare lane),
65 (a second strip one cell wide), 127 (exactly two strips), 128 (two strips and one column); each
of them has a last chunk of rows shorter than the others.  1025 takes the longer row chunks and,
with cells bound for host memory, consecutive launches."""
import math

import numpy as np
import pytest

import packets_fixture
import solidangle_ref as SR
from helpers import bit_equal, field_from_arr, fixture
from packets_fixture import torch  # noqa: F401 (the fixture)
from rayoptics_amd import abi, workloads

pytestmark = pytest.mark.gpu

SPOT = abi.INTERSECT_OBJ | abi.CHECK_APERTURES | abi.APPLY_VIGNETTING
SIZES = [2, 15, 64, 65, 127, 128]


def case(name):
    """-> (table, trace flags, fields [n_items], wavelength indices [n_items]); the systems of
    test_gpu_transmission.py"""
    if name == 'tilted':                                # decentred and tilted: rt is not the identity
        fx = fixture('tilted_singlet')
        c = fx['grid_f1']
        return fx.table, int(c['flags']), [field_from_arr(c['field'])] * 2, [0, 1]
    wl = workloads.load(name)
    picks = {'dblgauss_c2': ([0, 0, 2, 2], [0, 2, 0, 2]), 'rc_telescope_c4': ([0, 4], [0, 0]),
             'cell_phone': ([0, 1, 2], [1, 1, 1])}[name]     # (no ray of field 2 passes the apertures)
    return wl.table, SPOT, [wl.fields[f] for f in picks[0]], picks[1]


def trace(eng, flags, flds, wis, num, out_mode=abi.OUT_LAST):
    from rayoptics_amd.engine import make_grid, make_opts
    opts = [make_opts(flags=flags, out_mode=out_mode) for _ in flds]
    return eng.trace_pupil_grids(flds, wis, make_grid((-1., -1.), (1., 1.), num), opts, want_pupil=False)


def host_of(results):
    return packets_fixture.host_of(results, want=('seg', 'status'))


def check(results, num, items, cells, what, weight=None):
    """every item's record and cells against the restatement of its rows -> the records of the
    restatement"""
    worst, recs = 0.0, []
    for i, (seg, st) in enumerate(host_of(results)):
        rec, ref_cells, bounds = SR.of_packet(seg, st, num, None if weight is None else weight[i])
        if cells is not None:
            bit_equal(cells[i], ref_cells, f'{what} item {i}: cells')
        worst = max(worst, SR.check_record(items[i], rec, bounds, f'{what} item {i}', log=lambda s: None))
        recs.append(rec)
    print(f'{what}: largest sum error over its bound {worst:.3g}')
    return np.array(recs)


@pytest.mark.parametrize('num', SIZES)
def test_exact_against_the_restatement(torch, num):
    from rayoptics_amd.engine import TraceEngine
    table, flags, flds, wis = case('dblgauss_c2')
    eng = TraceEngine(table)
    results = trace(eng, flags, flds, wis, num)
    items, cells = eng.projected_solid_angle(results, num, want_cells=True)
    assert items.shape == (4,) and cells.shape == (4, num - 1, num - 1)
    recs = check(results, num, items, cells, f'dblgauss_c2 {num}^2')
    assert (items['n_cells'].sum(axis=1) == (num - 1) ** 2).all()
    assert items['aw_full'].tobytes() == items['a_full'].tobytes() and items['aw_tri'].tobytes() == items['a_tri'].tobytes()
    if num >= 15:                                       # apertures checked: the rim fails, triangles appear
        assert (recs['n_ok'] < num * num).all() and (recs['n_ok'] > 0.4 * num * num).all()
        assert (recs['n_cells'][:, 3] > 0).all() and (items['a_tri'] != 0.0).all()
    eng.close()


@pytest.mark.parametrize('name', ['rc_telescope_c4', 'cell_phone', 'tilted'])
def test_other_systems(torch, name):
    from rayoptics_amd.engine import TraceEngine
    table, flags, flds, wis = case(name)
    eng = TraceEngine(table)
    num = 65
    results = trace(eng, flags, flds, wis, num)
    items, cells = eng.projected_solid_angle(results, num, want_cells=True)
    check(results, num, items, cells, f'{name} {num}^2')
    if name == 'rc_telescope_c4':                       # the obscuration: cells with one and two rays inside
        assert [r.mode for r in table.rows].count(abi.REFLECT) == 2 and (items['n_cells'][:, 1:3] > 0).all()
    if name == 'cell_phone':
        none = items[2]
        assert none['n_ok'] == 0 and none['n_cells'].tolist() == [(num - 1) ** 2, 0, 0, 0, 0] and not cells[2].any()
        assert all(float(none[n]) == 0.0 for n in SR.SUMS)
        assert all(math.isnan(float(none[n])) for n in ('l_min', 'l_max', 'm_min', 'm_max', 'r2_max'))
        assert items[0]['n_ok'] > 100
    eng.close()


def test_last_and_full_packets_give_the_same_records(torch):
    from rayoptics_amd.engine import EngineError, TraceEngine, make_grid, make_opts
    table, flags, flds, wis = case('dblgauss_c2')
    eng = TraceEngine(table)
    num = 65
    last = trace(eng, flags, flds, wis, num)
    full = trace(eng, flags, flds, wis, num, abi.OUT_FULL)
    a, ca = eng.projected_solid_angle(last, num, want_cells=True)
    b, cb = eng.projected_solid_angle(full, num, want_cells=True)
    assert a.tobytes() == b.tobytes() and ca.tobytes() == cb.tobytes()
    one, _c = eng.projected_solid_angle(full[1], num)   # a single result gains the item axis
    assert one.tobytes() == a[1:2].tobytes()
    with pytest.raises(EngineError, match='item 1'):
        eng.projected_solid_angle([last[0], full[1]], num)
    with pytest.raises(EngineError, match='item 0'):
        eng.projected_solid_angle(last, num - 1)
    hits = eng.trace_pupil_grid(flds[0], make_grid((-1., -1.), (1., 1.), num), 0,
                                make_opts(flags=flags, out_mode=abi.OUT_HITS))
    with pytest.raises(EngineError, match='OUT_LAST or OUT_FULL'):
        eng.projected_solid_angle(hits, num)
    with pytest.raises(EngineError, match='weight'):
        eng.projected_solid_angle(last, num, weight=np.ones((4, 4, num * num)))
    eng.close()


def film_rows(eng, results, flags, wis, coating):
    """surface_thinfilm's rows, left on the device, with ``coating`` on every glass-air surface"""
    from rayoptics_amd import analyses
    from rayoptics_amd.coatings import stack_tables
    kind, value, stacks = analyses._coating_tables(eng.table, coating)
    first, thick, index, sub = stack_tables(eng.table, stacks, 'test')
    rows, _s, _i = eng.surface_thinfilm(results, flags, wis, [float(eng.table.wvls[w]) for w in wis], coat_kind=kind,
                                        coat_value=value, stack_first=first, layer_thickness=thick, layer_index=index,
                                        sub_index=sub, on_device=True)
    return rows


@pytest.mark.parametrize('coat', ['bare', 'quarter_wave'])
def test_weights_from_the_transmission_rows(torch, coat):
    from rayoptics_amd.coatings import Coating
    from rayoptics_amd.engine import TraceEngine
    table, flags, flds, wis = case('dblgauss_c2')
    eng = TraceEngine(table)
    num = 65
    results = trace(eng, flags, flds, wis, num, abi.OUT_FULL)
    if coat == 'bare':
        rows, _s, _i = eng.surface_transmission(results, flags, wis, on_device=True)
    else:
        rows = film_rows(eng, results, flags, wis, Coating.quarter_wave(1.38, 550.0))
    assert rows.is_cuda and tuple(rows.shape) == (4, 4, num * num)
    items, cells = eng.projected_solid_angle(results, num, weight=rows, want_cells=True)
    T = rows[:, 0].cpu().numpy()
    assert np.isnan(T).any()                            # NaN at the rays that failed: never read
    check(results, num, items, cells, f'{coat} weights', weight=T)
    plain, plain_cells = eng.projected_solid_angle(results, num, want_cells=True)
    assert plain_cells.tobytes() == cells.tobytes() and plain['a_full'].tobytes() == items['a_full'].tobytes()
    ratio = (items['aw_full'] + items['aw_tri']) / (items['a_full'] + items['a_tri'])
    assert (ratio > np.nanmin(T)).all() and (ratio < np.nanmax(T)).all()
    d, _c = eng.projected_solid_angle(results, num, weight=rows, weight_row=3)       # another row as the weight
    check(results, num, d, None, f'{coat} row 3', weight=rows[:, 3].cpu().numpy())
    eng.close()


def test_repeats_destinations_and_grouping(torch):
    from rayoptics_amd.engine import SA_ITEM_DTYPE, TraceEngine, records_view
    table, flags, flds, wis = case('dblgauss_c2')
    eng = TraceEngine(table)
    num = 128
    results = trace(eng, flags, flds, wis, num, abi.OUT_FULL)
    rows, _s, _i = eng.surface_transmission(results, flags, wis, on_device=True)
    items, cells = eng.projected_solid_angle(results, num, weight=rows, want_cells=True)
    again = eng.projected_solid_angle(results, num, weight=rows, want_cells=True)
    assert again[0].tobytes() == items.tobytes() and again[1].tobytes() == cells.tobytes(), 'a repeat differs'
    ditems, dcells = eng.projected_solid_angle(results, num, weight=rows, want_cells=True, on_device=True)
    assert records_view(ditems, SA_ITEM_DTYPE).tobytes() == items.tobytes()
    assert dcells.cpu().numpy().tobytes() == cells.tobytes(), 'device cells differ from host cells'
    for i, r in enumerate(results):                     # four in one call against four single calls
        i1, c1 = eng.projected_solid_angle(r, num, weight=rows[i:i + 1], want_cells=True)
        assert i1.tobytes() == items[i:i + 1].tobytes() and c1.tobytes() == cells[i:i + 1].tobytes(), f'item {i}'
    only, none = eng.projected_solid_angle(results, num, weight=rows)
    assert none is None and only.tobytes() == items.tobytes()
    eng.close()


def test_split_launches_equal_one_launch(torch):
    """4 items x 1025^2 rays with cells bound for host memory (8.4 MB each of a 32 MiB scratch):
    the items run as two launches; the same bits as device destinations (one launch), as one
    item's own call, and as the restatement on that item"""
    from rayoptics_amd.engine import SA_ITEM_DTYPE, TraceEngine, records_view
    table, flags, flds, wis = case('dblgauss_c2')
    eng = TraceEngine(table)
    num = 1025
    results = trace(eng, flags, flds, wis, num)
    items, cells = eng.projected_solid_angle(results, num, want_cells=True)
    ditems, dcells = eng.projected_solid_angle(results, num, want_cells=True, on_device=True)
    assert records_view(ditems, SA_ITEM_DTYPE).tobytes() == items.tobytes()
    assert dcells.cpu().numpy().tobytes() == cells.tobytes()
    i3, c3 = eng.projected_solid_angle(results[3], num, want_cells=True)
    assert i3.tobytes() == items[3:].tobytes() and c3.tobytes() == cells[3:].tobytes()
    check(results[3:], num, items[3:], cells[3:], '1025^2')
    eng.close()


def test_nan_rows_and_poisoned_weights_at_failed_rays(torch):
    """a hand-uploaded FULL packet whose rows are NaN wherever a ray failed (and in every slot
    but the image's), with NaN weights there: the records are finite, the restatement's"""
    from rayoptics_amd.engine import TraceEngine
    table = workloads.load('dblgauss_c2').table
    eng = TraceEngine(table)
    t = eng.torch
    num, n_seg = 65, 3
    x = np.linspace(-1.0, 1.0, num)
    X, Y = (v.ravel() for v in np.meshgrid(x, x, indexing='ij'))
    status = np.where((X - 0.1) ** 2 + Y * Y <= 0.7, abi.OK, abi.BLOCKED).astype(np.uint8)
    status[(np.abs(X) < 0.2) & (np.abs(Y) < 0.2)] = abi.TIR         # a hole: cells with 1, 2 and 3 corners
    ok = status == abi.OK
    seg = np.full((n_seg, 10, num * num), np.nan)
    seg[-1, 3] = np.where(ok, 0.3 * X + 0.02 * X * Y, np.nan)
    seg[-1, 4] = np.where(ok, -0.28 * Y + 0.01 * X * X, np.nan)      # a negative determinant
    w = np.where(ok, 0.9 - 0.1 * X * X, np.nan)
    res = packets_fixture.upload(eng, seg, status, np.zeros(num * num, np.int16))
    weight = t.from_numpy(np.ascontiguousarray(w.reshape(1, 1, -1))).to(eng.device)
    items, cells = eng.projected_solid_angle(res, num, weight=weight, want_cells=True)
    rec, ref_cells, bounds = SR.solid_angle(seg[-1, 3], seg[-1, 4], status, num, w)
    bit_equal(cells[0], ref_cells, 'cells')
    SR.check_record(items[0], rec, bounds, 'uploaded')
    assert all(np.isfinite(items[0][n]).all() for n in items.dtype.names) and np.isfinite(cells).all()
    assert (items['n_cells'][0, 1:] > 0).all() and items['a_full'][0] < 0.0 and items['aw_full'][0] > items['a_full'][0]
    eng.close()


def test_argument_errors_leave_the_outputs_untouched(torch):
    from rayoptics_amd.engine import SA_ITEM_DTYPE, TraceEngine, load_library
    lib = load_library()
    table, flags, flds, wis = case('dblgauss_c2')
    eng = TraceEngine(table)
    num = 15
    R = num * num
    results = trace(eng, flags, flds[:2], wis[:2], num)
    good = [r.out_struct() for r in results]
    weight = eng.torch.ones((2, 1, R), dtype=eng.torch.float64, device=eng.device)
    item = np.zeros(2, SA_ITEM_DTYPE)
    cells = np.zeros((2, num - 1, num - 1))

    def call(outs=None, n_items=2, num_=num, dir_row=3, stride=R, item_=True, cells_=True):
        arr = (abi.Out * 2)(*(outs or good))
        item['n_ok'] = -7
        cells[:] = 7.0
        rc = lib.rox_projected_solid_angle(n_items, num_, arr, dir_row, weight.data_ptr(), stride,
                                           item.ctypes.data if item_ else None, cells.ctypes.data if cells_ else None,
                                           None)
        return rc, lib.rox_last_error().decode()

    def bad(field, v):
        o = abi.Out.from_buffer_copy(bytes(good[1]))
        setattr(o, field, v)
        return [good[0], o]

    cases = [(dict(outs=bad('ld', R - 1)), 'item 1: ld'), (dict(outs=bad('seg', None)), 'item 1'),
             (dict(outs=bad('status', None)), 'item 1'), (dict(n_items=0), 'n_items'), (dict(num_=1), 'num'),
             (dict(num_=16385), 'num'), (dict(dir_row=-1), 'dir_row'), (dict(stride=R - 1), 'weight_stride'),
             (dict(item_=False, cells_=False), 'item and cells')]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith('rox_projected_solid_angle: ') and word in msg, (kw, rc, msg)
        assert (item['n_ok'] == -7).all() and (cells == 7.0).all(), f'{kw}: outputs touched'
    rc, msg = call()
    assert rc == 0, msg
    want = eng.projected_solid_angle(results, num, weight=weight, want_cells=True)
    assert item.tobytes() == want[0].tobytes() and cells.tobytes() == want[1].tobytes()
    eng.close()


def test_analysis_equals_the_pipeline_assembled_by_hand(torch):
    from rayoptics_amd import analyses
    from rayoptics_amd.coatings import Coating
    from rayoptics_amd.engine import make_grid
    from rayoptics_amd.trace import _launch_setup
    model = workloads.TableModel('dblgauss_c2')
    wvls = list(model.workload.table.wvls)
    num = 65
    F, W = len(model.fields), len(wvls)
    ri = analyses.relative_illumination(model, flds=model.fields, wvls=wvls, num_rays=num, cell_maps=True)

    def launch(out_mode):
        fs, wis, opts = [], [], []
        for fld in model.fields:
            for wvl in wvls:
                eng, f, wi, o = _launch_setup(model, fld, wvl, dict(check_apertures=True, apply_vignetting=True), out_mode)
                fs.append(f), wis.append(wi), opts.append(o)
        return eng, wis, int(opts[0].flags), eng.trace_pupil_grids(fs, wis, make_grid((-1., -1.), (1., 1.), num), opts,
                                                                   want_pupil=False)
    eng, wis, flags, results = launch(abi.OUT_LAST)
    items, cells = eng.projected_solid_angle(results, num, want_cells=True)
    assert ri.items.tobytes() == items.tobytes() and ri.cell_maps.tobytes() == cells.tobytes()
    assert ri.items.shape == (F, W) and ri.cell_maps.shape == (F, W, num - 1, num - 1) and ri.omega_t is None
    print('RI of the double Gauss:', np.array2string(ri.poly_ri, precision=4), 'boundary share',
          np.array2string(ri.boundary_share[:, 0], precision=3))
    assert ri.poly_ri[0] == 1.0 and 0.6 < ri.poly_ri[2] < ri.poly_ri[1] < 0.9 and not ri.folded.any()
    assert abs(ri.ri[2, model.workload.ref_wvl_idx] - 0.6592) < 2e-3      # the converged figure of the plain-C trace
    # coated: the FULL launch, the thin-film rows left on the device, row 0 as the weight
    coating = Coating.quarter_wave(1.38, 550.0)
    rt = analyses.relative_illumination(model, flds=model.fields, wvls=wvls, num_rays=num, coatings=coating)
    eng, wis, flags, results = launch(abi.OUT_FULL)
    rows = film_rows(eng, results, flags, wis, coating)
    witems, _c = eng.projected_solid_angle(results, num, weight=rows)
    assert rt.items.tobytes() == witems.tobytes()
    by_hand = analyses.RelativeIllumination(witems.reshape(F, W), [1.0] * W, weighted=True)
    assert np.array_equal(rt.ri_t, by_hand.ri_t) and np.array_equal(rt.omega, ri.omega)
    assert (rt.omega_t < rt.omega).all() and (rt.omega_t > 0.8 * rt.omega).all()
    bare = analyses.relative_illumination(model, flds=model.fields, wvls=wvls, num_rays=num, coatings='bare')
    assert (bare.omega_t < rt.omega_t).all()
