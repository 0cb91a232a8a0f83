"""rox_surface_footprints on the device against the NumPy restatement (tests/footprint_ref.py):
golden packets under the four flag combinations (integers, box, r2_max and maps exactly; centroid,
RMS radius and cos_inc_sum within the pairwise-summation bound of the exact values; the cosine
extremes within 8 * 2^-53), a case with MISSED and TIR rays traced by the oracle, the device's own
FULL packets of the double Gauss and the .zmx zoom (9 items, 256^2 rays), phantom filtering, a
1024^2 x 9 job split into several launches, bit-identical repeats, degenerate inputs, every
argument error, and analyses.beam_footprints on the double Gauss."""
import functools
import math

import numpy as np
import pytest

import footprint_ref as FR
import packets_fixture
from helpers import field_from_arr, fixture
from packets_fixture import torch, trace_packets, upload  # noqa: F401 (torch: the fixture)
from rayoptics_amd import abi, workloads

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SPOT = abi.INTERSECT_OBJ | abi.CHECK_APERTURES | abi.APPLY_VIGNETTING
GROUPS = [('dblgauss', 'rays_ap', 232, 152), ('dblgauss', 'grid_f0', 88, 56), ('dblgauss', 'grid_f2', 116, 28),
          ('cell_phone', 'rays_ap', 114, 78)]
FLAGS = [(False, False), (True, False), (False, True), (True, True)]


host_of = functools.partial(packets_fixture.host_of, want=('seg', 'status', 'fail_surf'))


def log2_ceil(n):
    return math.ceil(math.log2(n)) if n > 1 else 0


def check(rec, maps, ref, ref_maps, terms, what):
    """one item's records [n_seg] against the restatement"""
    for name in ('n', 'n_fail', 'n_inc', 'min', 'max', 'r2_max'):
        assert np.array_equal(rec[name], ref[name]), f'{what}: {name}\n{rec[name]}\n{ref[name]}'
    if ref_maps is not None:
        assert np.array_equal(maps, ref_maps), f'{what}: maps differ in {(maps != ref_maps).sum()} bins'
    for k in range(rec.shape[0]):
        n, ni = int(ref['n'][k]), int(ref['n_inc'][k])
        for name in ('cx', 'cy', 'rms_r', 'cos_inc_min', 'cos_inc_sum', 'cos_exit_min'):
            assert np.isnan(rec[name][k]) == np.isnan(ref[name][k]), f'{what} slot {k}: {name} NaN-ness'
        if n:
            b_ = 4 * log2_ceil(n) * U
            ex, ey = abs(rec['cx'][k] - ref['cx'][k]), abs(rec['cy'][k] - ref['cy'][k])
            # rms_r^2 = sum(dx^2 + dy^2) / n about the centroid: the terms are the squared deviations
            e2 = abs(rec['rms_r'][k] ** 2 - ref['rms_r'][k] ** 2)
            print(f'{what} slot {k}: n {n} cx err {ex:.3g} (bound {b_ * terms["abs_x"][k] / n:.3g}) cy err {ey:.3g} '
                  f'rms^2 err {e2:.3g} (bound {b_ * ref["rms_r"][k] ** 2:.3g})')
            assert ex <= b_ * terms['abs_x'][k] / n, f'{what} slot {k}: cx'
            assert ey <= b_ * terms['abs_y'][k] / n, f'{what} slot {k}: cy'
            assert e2 <= b_ * ref['rms_r'][k] ** 2, f'{what} slot {k}: rms_r'
        if not np.isnan(ref['cos_exit_min'][k]):
            assert abs(rec['cos_exit_min'][k] - ref['cos_exit_min'][k]) <= 8 * U, f'{what} slot {k}: cos_exit_min'
        if ni:
            es = abs(rec['cos_inc_sum'][k] - ref['cos_inc_sum'][k])
            em = abs(rec['cos_inc_min'][k] - ref['cos_inc_min'][k])
            # A deviation from the plain pairwise bound, declared: the restatement forms each cosine
            # without the kernel's fused products, so every TERM differs by up to the 8 * 2^-53 the
            # cosine extremes are allowed (the plain bound is 0 for n_inc = 1); that allowance per
            # term is added to the pairwise bound of the summation itself.
            bs = 4 * log2_ceil(ni) * U * terms['abs_ci'][k] + 8 * U * ni
            print(f'{what} slot {k}: n_inc {ni} cos_inc_sum err {es:.3g} (bound {bs:.3g}) cos_inc_min err {em:.3g}')
            assert es <= bs, f'{what} slot {k}: cos_inc_sum'
            assert em <= 8 * U, f'{what} slot {k}: cos_inc_min'


def run_and_check(eng, table, trace_flags, results, host, what, n_bins=16, combos=FLAGS):
    """``results``: DeviceResults; ``host``: [(seg, status, fail_surf)] of the same packets"""
    n_seg = eng.num_segments(trace_flags)
    for partial, ok_only in combos:
        rec, _m = eng.surface_footprints(results, trace_flags, partial=partial, ok_only=ok_only)
        hw = np.sqrt(np.maximum(rec['r2_max'].max(axis=0), 1e-6)) * 0.9      # some records outside the box
        rec2, maps = eng.surface_footprints(results, trace_flags, partial=partial, ok_only=ok_only, half_width=hw,
                                            n_bins=n_bins)
        assert rec.tobytes() == rec2.tobytes(), f'{what}: records differ with maps'
        assert rec.shape == (len(results), n_seg)
        for i, (seg, st, fs) in enumerate(host):
            ref, ref_maps, terms = FR.footprints(table, trace_flags, seg, st, fs, partial, ok_only, hw, n_bins)
            check(rec[i], maps[i], ref, ref_maps, terms, f'{what} item {i} partial={partial} ok_only={ok_only}')
    return rec


@pytest.mark.parametrize('name,group,n_ok,n_blocked', GROUPS)
def test_golden_packets(torch, name, group, n_ok, n_blocked):
    from rayoptics_amd.engine import TraceEngine
    fx = fixture(name)
    c = fx[group]
    counts = np.bincount(c['status'], minlength=5)
    assert counts[abi.OK] == n_ok and counts[abi.BLOCKED] == n_blocked and counts.sum() == n_ok + n_blocked
    eng = TraceEngine(fx.table)
    res = upload(eng, c['seg'], c['status'], c['fail_surf'])
    run_and_check(eng, fx.table, int(c['flags']), [res], [(c['seg'], c['status'], c['fail_surf'])], f'{name}/{group}')
    eng.close()


def missed_tir_case():
    """the double Gauss without aperture checks over twice its pupil: rays miss and reflect totally"""
    from oracle.oracle import make_opts as mk
    from oracle_engine import OracleEngine
    from rayoptics_amd.engine import make_grid
    fx = fixture('dblgauss')
    c = fx['grid_f2']
    h = OracleEngine(fx.table).trace_pupil_grid(field_from_arr(c['field']), make_grid((-2., -2.), (2., 2.), 33),
                                                int(c['wvl_idx']),
                                                mk(flags=abi.INTERSECT_OBJ, out_mode=abi.OUT_FULL)).to_host()
    return fx.table, abi.INTERSECT_OBJ, h


def test_missed_and_tir_rays(torch):
    from rayoptics_amd.engine import TraceEngine
    table, flags, h = missed_tir_case()
    counts = np.bincount(h.status, minlength=5)
    assert counts[abi.MISSED_SURFACE] >= 1 and counts[abi.TIR] >= 1, counts
    seg = np.array(h.seg)
    ns = FR.nseg(table, flags, h.status, h.fail_surf)
    for r in range(seg.shape[2]):
        seg[ns[r]:, :, r] = np.nan
    eng = TraceEngine(table)
    res = upload(eng, seg, h.status, h.fail_surf)
    rec = run_and_check(eng, table, flags, [res], [(seg, h.status, h.fail_surf)], 'missed/tir')
    assert rec['n_fail'][0, :, abi.MISSED_SURFACE].sum() == counts[abi.MISSED_SURFACE]
    assert rec['n_fail'][0, :, abi.TIR].sum() == counts[abi.TIR]
    eng.close()


def traced_items(eng, wl, num, n_items, flags=SPOT):
    F, W = len(wl.fields), len(wl.table.wvls)
    flds = [wl.fields[(i // W) % F] for i in range(n_items)]
    return trace_packets(eng, flags, flds, [i % W for i in range(n_items)], num)


@pytest.mark.parametrize('name', ['dblgauss_c2', 'zmx_evenasph_c3'])
def test_device_packets_end_to_end(torch, name):
    from rayoptics_amd.engine import TraceEngine
    wl = workloads.load(name)
    eng = TraceEngine(wl.table)
    results = traced_items(eng, wl, 256, 9)
    run_and_check(eng, wl.table, SPOT, results, host_of(results), name, n_bins=128, combos=[(True, False), (False, True)])
    # the nine items fit one launch (unsplit): bit for bit what each item's own call gives
    hw = np.full(eng.num_segments(SPOT), 30.0)
    rec, maps = eng.surface_footprints(results, SPOT, half_width=hw, n_bins=64)
    for i, r in enumerate(results):
        one, m1 = eng.surface_footprints(r, SPOT, half_width=hw, n_bins=64)
        assert one.tobytes() == rec[i:i + 1].tobytes(), f'{name} item {i}: one launch of nine != its own call'
        assert np.array_equal(m1[0], maps[i]), f'{name} item {i}: maps'
    eng.close()


def test_phantom_filtering(torch):
    """a model with a phantom interface, traced with ROX_FILTER_PHANTOMS: the slot map"""
    from rayoptics_amd import SurfaceTable
    from rayoptics_amd.engine import TraceEngine, make_grid, make_opts
    tbl = SurfaceTable.from_prescription([dict(cv=0, thi=10.0), dict(cv=0.02, thi=3.0, n=1.5),
                                          dict(cv=0, thi=2.0, mode='phantom'), dict(cv=-0.01, thi=5.0),
                                          dict(cv=0, thi=0)])
    assert any(r.mode == abi.PHANTOM for r in tbl.rows)
    flags = abi.INTERSECT_OBJ | abi.FILTER_PHANTOMS
    eng = TraceEngine(tbl)
    assert eng.num_segments(flags) == tbl.n_ifcs - 1
    R = 4096
    rng = np.random.default_rng(5)
    pt0 = np.zeros((3, R)); pt0[:2] = rng.uniform(-4, 4, (2, R))
    dir0 = np.zeros((3, R)); dir0[:2] = rng.uniform(-0.2, 0.2, (2, R)); dir0[2] = np.sqrt(1 - (dir0[:2] ** 2).sum(0))
    res = eng.trace_rays(pt0, dir0, 0, make_opts(flags=flags, out_mode=abi.OUT_FULL))
    run_and_check(eng, tbl, flags, [res], host_of([res]), 'phantom')
    eng.close()


def test_split_equals_unsplit_and_repeats(torch):
    """1024^2 rays x 9 items: the partial records exceed the scratch of one launch, so the items
    run as several launches; each item equals its own (unsplit) call bit for bit, a repeat and a
    device destination too"""
    from rayoptics_amd.engine import TraceEngine, footprint_view
    wl = workloads.load('dblgauss_c2')
    eng = TraceEngine(wl.table)
    results = traced_items(eng, wl, 1024, 9)
    hw = np.full(eng.num_segments(SPOT), 25.0)
    rec, maps = eng.surface_footprints(results, SPOT, half_width=hw, n_bins=64)
    again, maps2 = eng.surface_footprints(results, SPOT, half_width=hw, n_bins=64)
    assert rec.tobytes() == again.tobytes() and maps.tobytes() == maps2.tobytes()
    raw, dmaps = eng.surface_footprints(results, SPOT, half_width=hw, n_bins=64, on_device=True)
    assert footprint_view(raw).tobytes() == rec.tobytes()
    assert np.array_equal(dmaps.cpu().numpy().view(np.uint32), maps)
    for i, r in enumerate(results):
        one, m1 = eng.surface_footprints(r, SPOT, half_width=hw, n_bins=64)
        assert one.tobytes() == rec[i:i + 1].tobytes(), f'item {i}'
        assert np.array_equal(m1[0], maps[i]), f'item {i}: maps'
    assert int(rec['n'][:, 0].min()) == 1024 * 1024
    # against the plain NumPy restatement on one item's slots (n and the selections exactly)
    seg, st, fs = host_of(results[4:5])[0]
    ref, _m, _t = FR.footprints(wl.table, SPOT, seg[:, :, ::1], st, fs, exact=False)
    for name in ('n', 'n_fail', 'n_inc', 'min', 'max', 'r2_max'):
        assert np.array_equal(rec[name][4], ref[name]), name
    eng.close()


def test_degenerate_inputs(torch):
    from rayoptics_amd.engine import TraceEngine
    fx = fixture('dblgauss')
    c = fx['grid_f0']
    eng = TraceEngine(fx.table)
    n_seg, _ten, R = c['seg'].shape
    seg = np.full((n_seg, 10, R), np.nan)
    seg[0] = c['seg'][0]
    st = np.full(R, abi.MISSED_SURFACE, np.uint8)
    fs = np.full(R, 1, np.int16)
    res = upload(eng, seg, st, fs)
    rec, _m = eng.surface_footprints([res], int(c['flags']))
    assert rec['n'][0, 0] == R and (rec['n'][0, 1:] == 0).all()
    assert rec['n_fail'][0, 1, abi.MISSED_SURFACE] == R
    e = rec[0, 1:]
    assert np.isposinf(e['min']).all() and np.isneginf(e['max']).all() and np.isneginf(e['r2_max']).all()
    for name in ('cx', 'cy', 'rms_r', 'cos_inc_min', 'cos_inc_sum', 'cos_exit_min'):
        assert np.isnan(e[name]).all(), name
    fs0 = np.zeros(R, np.int16)                         # failed at the object: no record at all
    rec, _m = eng.surface_footprints([upload(eng, seg, st, fs0)], int(c['flags']))
    assert (rec['n'] == 0).all()
    one = upload(eng, c['seg'][:, :, :1], c['status'][:1], c['fail_surf'][:1])
    run_and_check(eng, fx.table, int(c['flags']), [one],
                  [(c['seg'][:, :, :1], c['status'][:1], c['fail_surf'][:1])], 'one ray')
    eng.close()


def test_argument_errors(torch):
    from rayoptics_amd.engine import TraceEngine, load_library, FOOTPRINT_DTYPE
    lib = load_library()
    fx = fixture('dblgauss')
    c = fx['grid_f0']
    eng = TraceEngine(fx.table)
    n_seg, _ten, R = c['seg'].shape
    res = upload(eng, c['seg'], c['status'], c['fail_surf'])
    good = res.out_struct()
    fp = np.zeros((2, n_seg), FOOTPRINT_DTYPE)
    maps = np.zeros((2, n_seg, 4, 4), np.uint32)
    hw = np.full(n_seg, 20.0)

    def call(outs=None, n_items=1, n_rays=R, flags=abi.FP_PARTIAL, fp_p=fp.ctypes.data, hw_p=hw.ctypes.data,
             n_bins=4, maps_p=maps.ctypes.data):
        arr = (abi.Out * 2)(*(outs or [good, good]))
        fp[:] = 0
        fp['n'] = -7
        maps[:] = 77
        rc = lib.rox_surface_footprints(eng._handle, int(c['flags']), flags, n_items, arr, n_rays, fp_p, hw_p,
                                        n_bins, maps_p, None)
        msg = lib.rox_last_error().decode()
        return rc, msg

    def bad(field, value):
        o = abi.Out.from_buffer_copy(bytes(good))
        setattr(o, field, value)
        return [good, o]

    nan_hw, neg_hw = hw.copy(), hw.copy()
    nan_hw[3], neg_hw[2] = np.nan, -1.0
    cases = [(dict(n_items=0), 'n_items'), (dict(n_items=abi.MAX_FOCUS_ITEMS + 1), 'n_items'),
             (dict(outs=bad('seg', None), n_items=2), 'item 1'), (dict(outs=bad('status', None), n_items=2), 'item 1'),
             (dict(outs=bad('fail_surf', None), n_items=2), 'item 1'), (dict(outs=bad('ld', R - 1), n_items=2), 'item 1'),
             (dict(n_rays=0), 'n_rays'), (dict(n_rays=(1 << 28) + 1), 'n_rays'),
             (dict(hw_p=None), 'half_width'), (dict(n_bins=0), 'n_bins'), (dict(n_bins=513), 'n_bins'),
             (dict(hw_p=nan_hw.ctypes.data), 'half_width[3]'), (dict(hw_p=neg_hw.ctypes.data), 'half_width[2]'),
             (dict(flags=4), 'fp_flags'), (dict(fp_p=None, maps_p=None), 'null fp and maps')]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == -1 and 'rox_surface_footprints' in msg and word in msg, (kw, rc, msg)
        assert (fp['n'] == -7).all() and (maps == 77).all(), f'{kw}: outputs touched'
    rc, msg = call()
    assert rc == 0, msg
    assert fp['n'][0, 0] == R and (maps[0, 1:].sum(axis=(1, 2)) > 0).all()     # (slot 0: the object, far outside)
    eng.close()


def test_analysis_on_the_double_gauss(torch):
    """beam_footprints on the TableModel: the dense grid's semi-diameter covers the rim rays' on every
    surface (num_rays odd: the grid holds the rim rays' pupil points), the union map's total is the
    number of counted records inside the map's box.  The rim rays are the pupil points
    vigcalc.trace_boundary_rays traces -- (+-1, 0), (0, +-1) with vignetting applied -- through
    trace_pupil_list: vigcalc.trace_boundary_rays itself imports the reference and reads
    opt_model.optical_spec (fields, pupil_rays), neither of which exists where this test runs (a
    TableModel carries a table and field constants only).  Their radius is taken from the packets
    directly, not through the restatement."""
    from rayoptics_amd import analyses
    model = workloads.TableModel('dblgauss_c2')
    wl = model.workload
    wvls = list(wl.table.wvls)
    num, bins = 65, 32
    bf = analyses.beam_footprints(model, flds=model.fields, wvls=wvls, num_rays=num, maps=bins, keep_packets=True)
    F, W, n_seg = bf.records.shape
    assert (F, W) == (len(model.fields), len(wvls)) and bf.maps.shape == (F, W, n_seg, bins, bins)
    # the rim rays: pupil (+-1, 0), (0, +-1) of every field, traced as the grid's rays are
    px, py = np.array([1., -1., 0., 0.]), np.array([0., 0., 1., -1.])
    rim = np.zeros(n_seg)
    for f in model.fields:
        for wvl in wvls:
            kw = dict(check_apertures=False, apply_vignetting=True)
            eng, rf, wi, opts = analyses._launch_setup(model, f, wvl, kw, abi.OUT_FULL)
            assert int(opts.flags) == bf.trace_flags
            res = eng.trace_pupil_list(rf, px, py, wi, opts)
            seg, st, fs = host_of([res])[0]
            ns = FR.nseg(wl.table, bf.trace_flags, st, fs)
            for r in range(4):                  # max_aperture_at_surf's own loop: len(ray) > i
                for k in range(int(ns[r])):
                    rim[k] = max(rim[k], math.sqrt(seg[k, 0, r] ** 2 + seg[k, 1, r] ** 2))
    assert (bf.semi_diameter >= rim * (1 - 1e-12)).all(), (bf.semi_diameter, rim)
    assert (bf.semi_diameter[1:] > 0).all()
    # the union map against the records inside each slot's box, from the packets themselves
    inside = np.zeros(n_seg, np.int64)
    for i, r in enumerate(bf.results):
        seg, st, fs = host_of([r])[0]
        ref, m, _t = FR.footprints(wl.table, bf.trace_flags, seg, st, fs, True, False, bf.half_width, bins)
        inside += m.sum(axis=(1, 2), dtype=np.int64)
        assert np.array_equal(bf.maps.reshape(F * W, n_seg, bins, bins)[i], m)
    assert np.array_equal(bf.union_map.sum(axis=(1, 2)), inside)
    assert inside.sum() == bf.records['n'].sum()            # the margin keeps every record inside
    ap = bf.clear_apertures(margin=0.05)
    assert len(ap) == wl.table.n_ifcs and np.allclose(ap, bf.semi_diameter * 1.05)
