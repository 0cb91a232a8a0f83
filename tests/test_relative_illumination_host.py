"""Relative illumination without a GPU: the binding and the struct mirror of
rox_projected_solid_angle, the argument errors of the C entry (answered before a device is
touched), closed forms of the NumPy restatement (tests/solidangle_ref.py), the figures of the
method on the shipped double Gauss re-derived through the plain-C trace, and the host logic of
analyses.relative_illumination over an engine double whose trace is that plain-C trace and whose
entry is the restatement.

Bounds.  The affine and the weight cases are exact by construction: dyadic coefficients on a
dyadic grid make every product and sum representable.  Convergence (set where the method was
first checked, on this trace): the corrected RI of fields 1 and 2 of dblgauss_c2 at 65^2 rays lies
within 1e-3 of the value at 257^2 (measured 3e-4 and 3e-5), the axial omega at 65^2 within 0.5 %
of pi * r2_max (measured 0.26 %)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import solidangle_ref as SR
from oracle import oracle
from rayoptics_amd import abi, analyses, workloads
from rayoptics_amd.engine import SA_ITEM_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPOT = abi.INTERSECT_OBJ | abi.CHECK_APERTURES | abi.APPLY_VIGNETTING


@pytest.fixture(scope='module')
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location('rox_build', os.path.join(ROOT, 'ray-optics_amd', 'build.py'))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return abi.declare(C.CDLL(b.build()))


# ---- the binding ----------------------------------------------------------------------------
def test_abi_declares_the_entry(lib):
    assert 'rox_projected_solid_angle' in abi.EXPORTS
    assert lib.rox_projected_solid_angle.restype is C.c_int and len(lib.rox_projected_solid_angle.argtypes) == 9
    assert abi.MAX_SA_NUM == 16384
    with open(os.path.join(ROOT, 'include', 'roxtrace.h')) as f:
        assert '#define ROX_MAX_SA_NUM 16384' in f.read()
    assert abi.ABI_VERSION == 8 and lib.rox_abi_version() == 8


def test_sa_item_layout_matches_header(tmp_path):
    """sizeof / offsetof of rox_sa_item as a C compiler sees include/roxtrace.h against the ctypes
    mirror, and the NumPy dtype against both"""
    st, dt, cname = abi.SaItem, SA_ITEM_DTYPE, 'rox_sa_item'
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/roxtrace.h"', 'int main(void) {',
             f'printf("{cname} %zu\\n", sizeof({cname}));']
    for fname, _t in st._fields_:
        lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['return 0; }']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-o', str(exe), str(src)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got[cname]) == C.sizeof(st) == dt.itemsize == 144
    assert [f for f, _t in st._fields_] == list(dt.names)
    for fname, ctype in st._fields_:
        assert int(got[f'{cname}.{fname}']) == getattr(st, fname).offset == dt.fields[fname][1], fname
        base = dt.fields[fname][0].base
        assert base == (np.int64 if ctype in (C.c_int64, C.c_int64 * 5) else np.float64), fname
    assert dt.fields['n_cells'][0].shape == (5,)


# ---- the C entry's argument errors, without a device --------------------------------------------
def call_sa(lib, over):
    """one rox_projected_solid_angle call on 2 items of 17 x 17 rays (ld 320) with ``over``
    replacing arguments; every pointer is an address the entry never reads: each case fails its
    checks first"""
    a = dict(n_items=2, num=17, outs=True, ld=[320, 320], seg=[8, 8], status=[8, 8], dir_row=3, weight=None,
             weight_stride=0, item=8, cells=8)
    a.update(over)
    outs = (abi.Out * 2)()
    for i in range(2):
        outs[i].seg, outs[i].status, outs[i].ld = a['seg'][i], a['status'][i], a['ld'][i]
    return lib.rox_projected_solid_angle(a['n_items'], a['num'], outs if a['outs'] else None, a['dir_row'],
                                         a['weight'], a['weight_stride'], a['item'], a['cells'], None)


C_ERRORS = [
    ('null outs', dict(outs=False), 'outs'),
    ('null seg', dict(seg=[None, 8]), 'item 0: null'),
    ('null status', dict(status=[8, None]), 'item 1: null'),
    ('null item and cells', dict(item=None, cells=None), 'item and cells'),
    ('num 1', dict(num=1), 'num'),
    ('num over', dict(num=16385), 'num'),
    ('ld < num^2', dict(ld=[320, 288]), 'item 1: ld'),
    ('n_items 0', dict(n_items=0), 'n_items'),
    ('n_items over', dict(n_items=abi.MAX_FOCUS_ITEMS + 1), 'n_items'),
    ('dir_row < 0', dict(dir_row=-1), 'dir_row'),
    ('weight_stride < num^2', dict(weight=8, weight_stride=288), 'weight_stride'),
]


@pytest.mark.parametrize('name,over,word', C_ERRORS, ids=[c[0] for c in C_ERRORS])
def test_c_argument_errors_need_no_device(lib, name, over, word):
    assert call_sa(lib, dict(over)) == -1
    msg = lib.rox_last_error().decode()
    assert msg.startswith('rox_projected_solid_angle: ') and word in msg, msg


# ---- closed forms of the restatement ------------------------------------------------------------
def grid(num):
    x = np.linspace(-1.0, 1.0, num)
    X, Y = np.meshgrid(x, x, indexing='ij')             # x_i outer, y_j inner
    return X.ravel(), Y.ravel()


@pytest.mark.parametrize('sign', [1.0, -1.0])
def test_an_affine_map_gives_every_cell_its_determinant(sign):
    num = 17                                            # h = 1/8
    X, Y = grid(num)
    a, b, c, d = 0.5, 0.25 * sign, -0.125, 0.75 * sign
    det = a * d - b * c
    L, M = a * X + b * Y + 0.0625, c * X + d * Y - 0.5
    rec, cells, _b = SR.solid_angle(L, M, np.zeros(num * num, np.uint8), num)
    assert (cells == det / 64.0).all() and (det < 0) == (sign < 0)
    assert rec['n_cells'].tolist() == [0, 0, 0, 0, 256] and rec['n_ok'] == 289
    assert rec['a_full'] == det * 4.0 and rec['a_tri'] == 0.0 and rec['a_abs'] == abs(det) * 4.0
    assert rec['aw_full'] == rec['a_full'] and rec['aw_tri'] == 0.0
    assert rec['l_min'] == L.min() and rec['m_max'] == M.max() and rec['r2_max'] == (L * L + M * M).max()
    ri = analyses.RelativeIllumination(np.array([[rec]]), [1.0])
    assert ri.omega[0, 0] == abs(det) * 4.0 == ri.omega_raw[0, 0] and not ri.folded.any()
    assert ri.boundary_share[0, 0] == 0.0 and ri.ri[0, 0] == 1.0


def test_a_folded_map_is_flagged():
    num = 17
    X, Y = grid(num)
    rec, cells, _b = SR.solid_angle(X * X, Y, np.zeros(num * num, np.uint8), num)
    assert rec['a_abs'] > 1.9 and abs(rec['a_full']) <= 256 * 2.0 ** -52 * rec['a_abs']
    assert (cells[:8] < 0).all() and (cells[8:] > 0).all()
    assert analyses.RelativeIllumination(np.array([[rec]]), [1.0]).folded.all()


def test_a_power_of_two_weight_scales_the_areas_exactly():
    num = 33
    X, Y = grid(num)
    st = np.where(X * X + Y * Y <= 0.8, abi.OK, abi.BLOCKED).astype(np.uint8)
    L, M = 0.3 * X + 0.01 * X * Y, 0.29 * Y - 0.02 * X * X
    plain, _c, _b = SR.solid_angle(L, M, st, num)
    rec, _c, _b = SR.solid_angle(L, M, st, num, np.full(num * num, 0.5))
    assert rec['n_cells'][3] > 0 and rec['a_tri'] != 0.0
    assert rec['aw_full'] == 0.5 * rec['a_full'] and rec['aw_tri'] == 0.5 * rec['a_tri']
    assert plain['aw_full'] == plain['a_full'] == rec['a_full'] and plain['aw_tri'] == plain['a_tri']


def test_nan_at_failed_rays_never_reaches_a_sum():
    num = 33
    X, Y = grid(num)
    st = np.where(X * X + Y * Y <= 0.8, abi.OK, abi.TIR).astype(np.uint8)
    L, M, w = 0.3 * X, 0.3 * Y, 0.9 + 0.1 * X
    clean, cells0, _b = SR.solid_angle(L, M, st, num, w)
    bad = st != abi.OK
    Ln, Mn, wn = (np.where(bad, np.nan, v) for v in (L, M, w))
    rec, cells1, _b = SR.solid_angle(Ln, Mn, st, num, wn)
    assert rec.tobytes() == clean.tobytes() and np.array_equal(cells0, cells1)
    assert all(math.isfinite(float(rec[n])) for n in SA_ITEM_DTYPE.names if n != 'n_cells')
    none, cells2, _b = SR.solid_angle(Ln, Mn, np.full(num * num, abi.BLOCKED, np.uint8), num, wn)
    assert none['n_ok'] == 0 and none['n_cells'].tolist() == [1024, 0, 0, 0, 0] and not cells2.any()
    assert all(float(none[n]) == 0.0 for n in SR.SUMS) and math.isnan(none['l_min']) and math.isnan(none['r2_max'])
    ri = analyses.RelativeIllumination(np.array([[clean], [none]]), [1.0])
    assert np.isnan(ri.omega[1, 0]) and np.isnan(ri.ri[1, 0]) and np.isnan(ri.fno_eff[1, 0]) and ri.ri[0, 0] == 1.0
    assert np.isnan(ri.chief_dir[1]).all() and np.isnan(ri.poly_ri[1]) and not ri.folded[1, 0]


def test_the_boundary_correction_on_a_disc():
    """L = x, M = y inside the unit disc: the cells counted lie inside it, so raw <= pi, and the
    corrected estimate is the nearer one at every size"""
    for num in (17, 33, 65, 129):
        X, Y = grid(num)
        st = np.where(X * X + Y * Y <= 1.0, abi.OK, abi.BLOCKED).astype(np.uint8)
        rec, _c, _b = SR.solid_angle(X, Y, st, num)
        ri = analyses.RelativeIllumination(np.array([[rec]]), [1.0])
        raw, est = ri.omega_raw[0, 0], ri.omega[0, 0]
        print(f'disc num {num}: raw {raw:.6f} corrected {est:.6f} pi {math.pi:.6f} share {ri.boundary_share[0, 0]:.4f}')
        assert raw <= math.pi and abs(est - math.pi) < abs(raw - math.pi)
        assert 0.0 < ri.boundary_share[0, 0] < 0.2 and not ri.folded.any()
        assert abs(ri.fno_eff[0, 0] - 0.5 / math.sqrt(est / math.pi)) <= 4 * SR.EPS


# ---- the method's figures on the double Gauss, through the plain-C trace --------------------------
def oracle_items(name, num, fields=None, wvl_idx=None, out_mode=abi.OUT_LAST, weight=None):
    wl = workloads.load(name)
    wi = wl.ref_wvl_idx if wvl_idx is None else wvl_idx
    recs = []
    for k in (range(len(wl.fields)) if fields is None else fields):
        o = oracle.make_opts(flags=SPOT, out_mode=out_mode)
        r = oracle.trace_pupil_grid(wl.table, wl.fields[k], oracle.make_grid((-1., -1.), (1., 1.), num), wi, o)
        recs.append(SR.of_packet(np.asarray(r.seg), np.asarray(r.status), num)[0])
    return np.array(recs)


@pytest.fixture(scope='module')
def dblgauss_65_257():
    return {num: analyses.RelativeIllumination(oracle_items('dblgauss_c2', num)[:, None], [1.0]) for num in (65, 257)}


def test_relative_illumination_of_the_double_gauss_converges(dblgauss_65_257):
    coarse, fine = dblgauss_65_257[65], dblgauss_65_257[257]
    for f in (1, 2):
        err = abs(coarse.ri[f, 0] - fine.ri[f, 0])
        print(f'field {f}: RI {coarse.ri[f, 0]:.5f} at 65^2, {fine.ri[f, 0]:.5f} at 257^2, difference {err:.2g}')
        assert err <= 1e-3
    assert coarse.ri[0, 0] == 1.0 and 0.6 < fine.ri[2, 0] < fine.ri[1, 0] < 0.9
    closed = math.pi * float(coarse.items[0, 0]['r2_max'])
    err = abs(coarse.omega[0, 0] - closed) / closed
    print(f'axial omega {coarse.omega[0, 0]:.6f} closed form {closed:.6f} relative error {err:.2%}')
    assert err <= 0.005 and abs(coarse.omega_raw[0, 0] - closed) / closed > 0.02      # the correction is needed
    assert not coarse.folded.any() and not fine.folded.any()
    assert np.array_equal(coarse.na_max, np.sqrt(coarse.items['r2_max']))
    assert abs(coarse.chief_dir[0, 0]).max() < 1e-12 and coarse.chief_dir[2, 0, 1] != 0.0


def test_last_and_full_packets_hold_the_same_rows():
    last = oracle_items('dblgauss_c2', 15, fields=[2])
    full = oracle_items('dblgauss_c2', 15, fields=[2], out_mode=abi.OUT_FULL)
    assert last.tobytes() == full.tobytes() and 0 < last[0]['n_ok'] < 225


# ---- relative_illumination(): the Python layer over an engine double ---------------------------------
def stub_engine():
    import fresnel_ref as FR
    from oracle_engine import OracleEngine

    class StubEngine(OracleEngine):
        """the trace is the plain-C trace, rox_projected_solid_angle and
        rox_surface_transmission are their restatements; every call is recorded"""
        calls = []

        def trace_pupil_grids(self, flds, wvl_idxs, grid, opts_list, **kw):
            self.calls.append(('trace', len(flds), int(grid.num), int(opts_list[0].flags), int(opts_list[0].out_mode)))
            return super().trace_pupil_grids(flds, wvl_idxs, grid, opts_list)

        def surface_transmission(self, results, trace_flags, wvl_idxs, coat_kind=None, coat_value=None,
                                 want_rows=True, fields=False, on_device=False):
            self.calls.append(('tx', len(results), list(wvl_idxs), coat_kind, coat_value, on_device))
            rows = [FR.transmission_a(self.table, trace_flags, r.to_host().seg, r.to_host().status, wi, coat_kind,
                                      coat_value)['rows'] for r, wi in zip(results, wvl_idxs)]
            return np.stack(rows), None, None

        def surface_thinfilm(self, results, trace_flags, wvl_idxs, wvls_nm=None, **kw):
            self.calls.append(('film', len(results), list(wvl_idxs), list(wvls_nm), kw['coat_kind'], kw['on_device']))
            return np.full((len(results), 4, results[0].to_host().status.shape[0]), 0.5), None, None

        def projected_solid_angle(self, results, num, weight=None, weight_row=0, want_cells=False, on_device=False):
            self.calls.append(('sa', len(results), int(num), weight is not None, weight_row, want_cells))
            out = [SR.of_packet(r.to_host().seg, r.to_host().status, num,
                                None if weight is None else weight[i, weight_row])
                   for i, r in enumerate(results)]
            return np.array([o[0] for o in out]), (np.stack([o[1] for o in out]) if want_cells else None)

    StubEngine.calls = []
    return StubEngine


@pytest.fixture
def doubled(monkeypatch):
    model = workloads.TableModel('dblgauss_c2')
    eng = stub_engine()(model.workload.table)

    def setup(opt_model, fld, wvl, kw, out_mode, *a, **k):
        from rayoptics_amd.trace import opts_from_kwargs
        return eng, fld.rox_field, eng.table.wvl_index(wvl), opts_from_kwargs(eng.table.n_ifcs, kw, out_mode)
    monkeypatch.setattr(analyses, '_launch_setup', setup)
    return model, eng


def test_python_layer_without_coatings(doubled):
    model, eng = doubled
    wvls = list(eng.table.wvls)
    F, W, num = len(model.fields), len(wvls), 17
    ri = analyses.relative_illumination(model, flds=model.fields, wvls=wvls, num_rays=num, cell_maps=True)
    assert [c[0] for c in eng.calls] == ['trace', 'sa']             # one LAST launch, one entry call
    _t, n, g, flags, mode = eng.calls[0]
    assert (n, g, mode) == (F * W, num, abi.OUT_LAST) and flags & abi.APPLY_VIGNETTING and flags & abi.CHECK_APERTURES
    assert eng.calls[1] == ('sa', F * W, num, False, 0, True)
    assert ri.items.shape == (F, W) and ri.cell_maps.shape == (F, W, num - 1, num - 1) and ri.omega_t is None
    assert (ri.ri[0] == 1.0).all() and ri.poly_ri[0] == 1.0 and (ri.ri[1:] < 1.0).all() and (ri.ri[2] < ri.ri[1]).all()
    # the records are those of each item's own trace, field-major
    want = oracle_items('dblgauss_c2', num, fields=[2], wvl_idx=1)[0]
    assert ri.items[2, 1].tobytes() == want.tobytes()
    assert np.array_equal(ri.cell_maps.sum(axis=(2, 3)) != 0, ri.items['n_ok'] > 0)
    # the spectral merge, the F-number and the other ref_field
    s = np.array([1.0, 2.0, 3.0])[:W]
    merged = analyses.RelativeIllumination(ri.items, s, ref_field=1)
    assert np.allclose(merged.poly_omega, (ri.omega * s).sum(axis=1) / s.sum(), rtol=8 * SR.EPS, atol=0)
    assert np.array_equal(merged.poly_ri, merged.poly_omega / merged.poly_omega[1]) and merged.poly_ri[1] == 1.0
    assert (merged.ri[1] == 1.0).all() and np.array_equal(merged.ri, ri.omega / ri.omega[1][None, :])
    assert np.array_equal(ri.fno_eff, 1.0 / (2.0 * np.sqrt(ri.omega / np.pi))) and (ri.fno_eff[0] > 1.9).all()
    eng.calls.clear()
    off = analyses.relative_illumination(model, flds=model.fields[:1], wvls=wvls[:1], num_rays=num,
                                         check_apertures=False)
    assert not eng.calls[0][3] & abi.CHECK_APERTURES and off.cell_maps is None and eng.calls[1][5] is False


def test_python_layer_with_coatings(doubled):
    from rayoptics_amd.coatings import Coating
    model, eng = doubled
    wvls = list(eng.table.wvls)[:2]
    kw = dict(flds=model.fields[::2], wvls=wvls, num_rays=9)
    bare = analyses.relative_illumination(model, coatings='bare', **kw)
    assert [c[0] for c in eng.calls] == ['trace', 'tx', 'sa']
    assert eng.calls[0][4] == abi.OUT_FULL and eng.calls[1][1:5] == (4, [0, 1, 0, 1], None, None)
    assert eng.calls[1][5] is True                                  # the rows stay on the device
    assert eng.calls[2] == ('sa', 4, 9, True, 0, False)
    plain = analyses.relative_illumination(model, **kw)
    assert np.array_equal(bare.omega, plain.omega) and np.array_equal(bare.ri, plain.ri)
    assert (bare.omega_t < bare.omega).all() and (bare.omega_t > 0.5 * bare.omega).all()
    assert (bare.ri_t[0] == 1.0).all() and bare.poly_ri_t[0] == 1.0 and plain.omega_t is None
    assert np.abs(bare.ri_t[1] - bare.ri[1]).max() < 0.02           # Fresnel losses change RI a little, not a lot
    eng.calls.clear()
    ideal = analyses.relative_illumination(model, coatings='ideal', **kw)
    assert (eng.calls[1][3] == abi.COAT_IDEAL).all()
    assert np.abs(ideal.omega_t / ideal.omega - 1.0).max() < 1e-12
    eng.calls.clear()
    film = analyses.relative_illumination(model, coatings=Coating.quarter_wave(1.38, 550.0), **kw)
    assert [c[0] for c in eng.calls] == ['trace', 'film', 'sa'] and (eng.calls[1][4] == abi.COAT_STACK).any()
    assert eng.calls[1][3] == [float(eng.table.wvls[w]) for w in (0, 1, 0, 1)] and eng.calls[1][5] is True
    assert np.allclose(film.omega_t, 0.5 * film.omega, rtol=1e-13, atol=0)   # the double's constant T = 1/2


def test_python_layer_argument_checks(doubled):
    model, eng = doubled
    wvls = list(eng.table.wvls)
    for bad in (1, 0, 16385):
        with pytest.raises(ValueError, match='num_rays'):
            analyses.relative_illumination(model, flds=model.fields, wvls=wvls, num_rays=bad)
    with pytest.raises(ValueError, match='ref_field'):
        analyses.relative_illumination(model, flds=model.fields, wvls=wvls, ref_field=len(model.fields))
    with pytest.raises(ValueError, match='coatings'):
        analyses.relative_illumination(model, flds=model.fields, wvls=wvls, coatings='shiny')
    with pytest.raises(ValueError, match='sweep'):
        analyses.relative_illumination(model, wvls=wvls, sweep=5)
    assert eng.calls == []


# ---- the field sweep on the live reference's double Gauss ----------------------------------------
@pytest.mark.needs_reference
def test_sweep_on_the_reference_double_gauss():
    import copy
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), 'golden'))
    import refmodels as rm
    from rayoptics_amd import session, trace
    session._set_engine_factory(stub_engine())
    try:
        opm = rm.dblgauss()
        wvl = opm['osp']['wvls'].central_wvl
        sw = analyses.relative_illumination(opm, wvls=[wvl], num_rays=33, sweep=5)
        assert sw.ri.shape == (5, 1) and len(sw.flds) == 5
        outer = opm['osp']['fov'].fields[-1]
        assert [f.y for f in sw.flds] == [outer.y * t for t in np.linspace(0.0, 1.0, 5)]
        assert all(f.vuy == f.vly == f.vux == f.vlx == 0.0 and f.aim_info is not None for f in sw.flds)
        print('RI against field:', ' '.join(f'{v:.4f}' for v in sw.ri[:, 0]))
        assert sw.ri[0, 0] == 1.0 and (np.diff(sw.ri[:, 0]) <= 0.0).all() and sw.ri[-1, 0] < 1.0
        # the ends are the model's own axial and outermost fields, traced the same way
        own = []
        for f in (opm['osp']['fov'].fields[0], outer):
            g = copy.copy(f)
            g.vux = g.vuy = g.vlx = g.vly = 0.0
            g.aim_info = trace.aim_chief_ray(opm, g)
            own.append(g)
        ends = analyses.relative_illumination(opm, flds=own, wvls=[wvl], num_rays=33)
        assert ends.items[0, 0].tobytes() == sw.items[0, 0].tobytes()
        assert ends.items[1, 0].tobytes() == sw.items[4, 0].tobytes()
    finally:
        session._set_engine_factory(None)
