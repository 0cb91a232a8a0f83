"""Fresnel transmission without a GPU: the binding and the struct mirrors of
rox_surface_transmission, the NumPy restatement (tests/fresnel_ref.py) against closed forms and
against its independent second formulation on the golden packets, the host logic of
analyses.Transmission and transmission(), and the argument errors of the C entry, which answers
them before it touches a device.

Bounds.  Closed forms: 32 * 2^-53 relative -- about four roundings per surface, doubled by the
square, two surfaces.  (A) against (B): the largest |A - B| over the golden cases below was
measured at 2.11e-15 (19 * 2^-53, dblgauss grid_f2, row T1); the test asserts ten times that.
Neither formulation is the code under test."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import fresnel_ref as FR
from helpers import fixture
from rayoptics_amd import SurfaceTable, abi, analyses, workloads
from rayoptics_amd.engine import TX_ITEM_DTYPE, TX_SURFACE_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS, CLOSED, AB_MEASURED, AB_BOUND = FR.EPS, FR.CLOSED, FR.AB_MEASURED, FR.AB_BOUND
AB_CASES = [('dblgauss', 'grid_f0'), ('dblgauss', 'grid_f2'), ('rc_telescope', 'grid_f0'),
            ('rc_telescope', 'grid_f4'), ('tilted_singlet', 'grid_f1')]


@pytest.fixture(scope='module')
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location('rox_build', os.path.join(ROOT, 'ray-optics_amd', 'build.py'))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return abi.declare(C.CDLL(b.build()))


# ---- the binding ----------------------------------------------------------------------------
def test_abi_declares_the_entry(lib):
    assert 'rox_surface_transmission' in abi.EXPORTS
    assert lib.rox_surface_transmission.restype is C.c_int and len(lib.rox_surface_transmission.argtypes) == 15
    assert (abi.TX_FIELDS, abi.COAT_BARE, abi.COAT_IDEAL, abi.COAT_FIXED) == (1, 0, 1, 2)
    with open(os.path.join(ROOT, 'include', 'roxtrace.h')) as f:
        src = f.read()
    assert '#define ROX_TX_FIELDS 1u' in src
    assert 'enum { ROX_COAT_BARE = 0, ROX_COAT_IDEAL = 1, ROX_COAT_FIXED = 2 };' in src
    assert abi.ABI_VERSION == 8 and lib.rox_abi_version() == 8


def test_tx_struct_layouts_match_header(tmp_path):
    """sizeof / offsetof of rox_tx_surface and rox_tx_item as a C compiler sees include/roxtrace.h
    against the ctypes mirrors, and the NumPy dtypes against both"""
    structs = {'rox_tx_surface': (abi.TxSurface, TX_SURFACE_DTYPE), 'rox_tx_item': (abi.TxItem, TX_ITEM_DTYPE)}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/roxtrace.h"', 'int main(void) {']
    for cname, (st, _dt) in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _t in st._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['return 0; }']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-o', str(exe), str(src)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for cname, (st, dt) in structs.items():
        assert int(got[cname]) == C.sizeof(st) == dt.itemsize, cname
        assert [f for f, _t in st._fields_] == list(dt.names)
        for fname, ctype in st._fields_:
            assert int(got[f'{cname}.{fname}']) == getattr(st, fname).offset == dt.fields[fname][1], f'{cname}.{fname}'
            assert dt.fields[fname][0] == (np.int64 if ctype is C.c_int64 else np.float64)


# ---- (A) against closed forms on hand-made packets ----------------------------------------------
def plate(n):
    """object, two flat surfaces around glass of index n, image"""
    return SurfaceTable.from_prescription([dict(cv=0, thi=10.0), dict(cv=0, thi=3.0, n=n), dict(cv=0, thi=5.0),
                                           dict(cv=0, thi=0)])


def one_surface(n1, n2):
    """object in n1, one flat surface into n2, image"""
    return SurfaceTable.from_prescription([dict(cv=0, thi=10.0, n=n1), dict(cv=0, thi=3.0, n=n2), dict(cv=0, thi=0)])


def packet(dirs):
    """a hand-made FULL packet: ``dirs`` [n_seg][3, R] directions, every normal (0, 0, 1)"""
    R = np.asarray(dirs[0]).shape[1]
    seg = np.full((len(dirs), 10, R), np.nan)
    for k, d in enumerate(dirs):
        seg[k, 3:6] = d
        seg[k, 7:10] = np.array([[0.0], [0.0], [1.0]])
    return seg, np.zeros(R, np.uint8)


def test_normal_incidence_on_a_plate():
    for n in (1.5, 1.7552, 2.4):
        z = np.array([[0.0], [0.0], [1.0]])
        seg, status = packet([z, z, z, z])
        a = FR.transmission_a(plate(n), 0, seg, status, 0)
        want = (4.0 * n / (n + 1.0) ** 2) ** 2
        T, T1, T2, D = a['rows'][:, 0]
        for got in (T, T1, T2):
            assert abs(got - want) <= CLOSED * want, (n, got, want)
        assert D == 0.0 and T1 == T2
        one = 4.0 * n / (n + 1.0) ** 2
        assert np.abs(a['Ts'][1:3, 0] - one).max() <= CLOSED * one and np.array_equal(a['Ts'], a['Tp'])
        assert np.array_equal(a['ci'], np.ones((4, 1)))


def test_brewster_incidence_in_the_xz_plane():
    """at atan(n) in the x-z plane the x-like state is p: nothing is reflected at the first
    surface; the y-like state is s with Ts = 4 n^2 / (n^2 + 1)^2"""
    for n in (1.5, 1.7552, 2.4):
        th = math.atan(n)
        d0 = np.array([[math.sin(th)], [0.0], [math.cos(th)]])
        d1 = np.array([[math.cos(th)], [0.0], [math.sin(th)]])      # sin(theta_t) = cos(theta_i) there
        seg, status = packet([d0, d1, d1])
        a = FR.transmission_a(one_surface(1.0, n), 0, seg, status, 0, fields=True)
        T, T1, T2, D = a['rows'][:4, 0]
        want = 4.0 * n * n / (n * n + 1.0) ** 2
        assert abs(T1 - 1.0) <= CLOSED, (n, T1)
        assert abs(T2 - want) <= CLOSED * want, (n, T2, want)
        assert abs(T - (1.0 + want) / 2.0) <= CLOSED and abs(D - (1.0 - want) / (1.0 + want)) <= 2 * CLOSED
        E1, E2 = a['rows'][4:7, 0], a['rows'][7:10, 0]
        assert abs(E1 @ d1[:, 0]) <= CLOSED and abs(E2 @ d1[:, 0]) <= CLOSED      # transverse to the ray
        assert abs(E2[1]) == np.abs(E2).max() and E1[1] == 0.0


def test_energy_is_conserved_at_a_bare_interface():
    """Ts + Rs = 1 and Tp + Rp = 1 over angles and index pairs, the reflectances from the
    amplitude ratios rs = (n1 ci - n2 ct)/(n1 ci + n2 ct), rp = (n2 ci - n1 ct)/(n2 ci + n1 ct)"""
    for n1, n2 in ((1.0, 1.5), (1.0, 2.4), (1.33, 1.7552), (1.5, 1.0), (1.7552, 1.33)):
        lim = math.asin(min(1.0, n2 / n1))
        th = np.linspace(0.0, 0.98 * min(lim, math.pi / 2), 61)
        az = np.linspace(0.0, 6.0, th.size)
        si, ci = np.sin(th), np.cos(th)
        st = n1 * si / n2
        ct = np.sqrt(1.0 - st * st)
        d0 = np.stack([si * np.cos(az), si * np.sin(az), ci])
        d1 = np.stack([st * np.cos(az), st * np.sin(az), ct])
        seg, status = packet([d0, d1, d1])
        a = FR.transmission_a(one_surface(n1, n2), 0, seg, status, 0)
        Rs = ((n1 * ci - n2 * ct) / (n1 * ci + n2 * ct)) ** 2
        Rp = ((n2 * ci - n1 * ct) / (n2 * ci + n1 * ct)) ** 2
        assert np.abs(a['Ts'][1] + Rs - 1.0).max() <= CLOSED, (n1, n2)
        assert np.abs(a['Tp'][1] + Rp - 1.0).max() <= CLOSED, (n1, n2)
        # in the plane of incidence's own basis the states do not mix: T1 and T2 lie between Ts and Tp
        lo, hi = np.minimum(a['Ts'][1], a['Tp'][1]), np.maximum(a['Ts'][1], a['Tp'][1])
        for j in (0, 1, 2):
            assert (a['rows'][j] >= lo - CLOSED).all() and (a['rows'][j] <= hi + CLOSED).all()


def test_failed_rays_are_nan_and_do_not_count():
    z = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]])
    seg, status = packet([z, z, z, z])
    status[1] = abi.BLOCKED
    seg[2:, :, 1] = np.nan
    a = FR.transmission_a(plate(1.5), 0, seg, status, 0)
    assert np.isnan(a['rows'][:, 1]).all() and not np.isnan(a['rows'][:, [0, 2]]).any()
    surf, item = FR.records(a)
    assert item['n_ok'] == 2 and item['n_rays'] == 3 and (surf['n'] == 2).all()
    status[:] = abi.BLOCKED
    surf, item = FR.records(FR.transmission_a(plate(1.5), 0, seg, status, 0))
    assert item['n_ok'] == 0 and item['t_sum'] == 0.0 and math.isnan(item['t_min']) and math.isnan(item['d_max'])
    assert (surf['ts_sum'] == 0.0).all() and np.isnan(surf['ci_min']).all()


def test_coatings_in_the_restatement():
    th = 0.5
    d0 = np.array([[math.sin(th)], [0.0], [math.cos(th)]])
    st = math.sin(th) / 1.5
    d1 = np.array([[st], [0.0], [math.sqrt(1.0 - st * st)]])
    seg, status = packet([d0, d1, d0, d0])
    tbl = plate(1.5)
    kind = np.full(4, abi.COAT_IDEAL, np.int32)
    val = np.ones((4, 2))
    a = FR.transmission_a(tbl, 0, seg, status, 0, kind, val)
    assert np.abs(a['rows'][:3, 0] - 1.0).max() <= CLOSED and a['rows'][3, 0] <= CLOSED
    kind[2], val[2] = abi.COAT_FIXED, (0.9, 0.8)
    a = FR.transmission_a(tbl, 0, seg, status, 0, kind, val)
    T, T1, T2, _D = a['rows'][:, 0]
    assert abs(T1 - 0.8) <= CLOSED and abs(T2 - 0.9) <= CLOSED       # the x-like state is p in the x-z plane
    assert a['Ts'][2, 0] == 0.9 and a['Tp'][2, 0] == 0.8


def test_a_and_b_share_the_axis_at_normal_incidence():
    """at exactly normal incidence a fixed coating with Ts != Tp makes the result depend on the
    axis chosen for s^: both formulations take the one the header names"""
    z = np.array([[0.0], [0.0], [1.0]])
    seg, status = packet([z, z, z, z])
    tbl = plate(1.5)
    kind = np.array([0, abi.COAT_FIXED, abi.COAT_BARE, 0], np.int32)
    val = np.array([(1.0, 1.0), (0.9, 0.8), (1.0, 1.0), (1.0, 1.0)])
    a = FR.transmission_a(tbl, 0, seg, status, 0, kind, val)['rows'][:, 0]
    b = FR.transmission_b(tbl, 0, seg, status, 0, kind, val)[:, 0]
    assert np.abs(a - b).max() <= AB_BOUND and abs(a[1] - a[2]) > 0.05


# ---- (A) against (B) on the golden packets ------------------------------------------------------
def test_a_against_b_on_golden_packets():
    worst, where = 0.0, None
    for name, case in AB_CASES:
        fx = fixture(name)
        c = fx[case]
        args = (fx.table, int(c['flags']), c['seg'], c['status'], int(c['wvl_idx']))
        a, b = FR.transmission_a(*args), FR.transmission_b(*args)
        ok = a['ok']
        assert ok.sum() >= 20 and np.isnan(b[:, ~ok]).all() and np.isnan(a['rows'][:, ~ok]).all()
        dev = np.abs(a['rows'][:, ok] - b[:, ok])
        if dev.max() > worst:
            worst, where = float(dev.max()), (name, case, int(dev.max(axis=1).argmax()))
    print(f'largest |A - B| = {worst:.3e} ({worst / EPS:.1f} * 2^-53) at {where}')
    assert worst <= AB_BOUND, (worst, where)
    assert worst >= AB_MEASURED / 10, 'the recorded figure no longer describes the formulations'
    mirrors = [r.mode for r in fixture('rc_telescope').table.rows].count(abi.REFLECT)
    eye = np.eye(3).ravel().tolist()
    turned = [list(r.rt) != eye for r in fixture('tilted_singlet').table.rows]
    orders = {r.rt_order for r in fixture('tilted_singlet').table.rows}
    assert mirrors == 2 and sum(turned) >= 2 and orders == {abi.RT_F_ORDER, abi.RT_C_ORDER}


def test_a_skew_ray_is_not_the_product_of_mean_coefficients():
    fx = fixture('dblgauss')
    c = fx['grid_f2']
    a = FR.transmission_a(fx.table, int(c['flags']), c['seg'], c['status'], int(c['wvl_idx']))
    naive = np.prod((a['Ts'] + a['Tp']) / 2.0, axis=0)
    T = a['rows'][0, a['ok']]
    assert np.abs(T - naive).max() > 100 * EPS and np.abs(T - naive).max() < 1e-2


# ---- Transmission on synthetic records ----------------------------------------------------------
def synthetic(F=3, W=2, n_seg=5, seed=0):
    rng = np.random.default_rng(seed)
    item = np.zeros((F, W), TX_ITEM_DTYPE)
    item['n_rays'] = 100
    item['n_ok'] = rng.integers(40, 100, (F, W))
    item['t_sum'] = item['n_ok'] * rng.uniform(0.6, 0.9, (F, W))
    item['d_sum'] = item['n_ok'] * rng.uniform(0.0, 0.05, (F, W))
    item['d_max'] = rng.uniform(0.05, 0.1, (F, W))
    surf = np.zeros((F, W, n_seg), TX_SURFACE_DTYPE)
    surf['n'] = item['n_ok'][:, :, None]
    surf['t_sum'] = surf['n'] * rng.uniform(0.9, 1.0, (F, W, n_seg))
    surf['t_sum'][:, :, 0] = surf['t_sum'][:, :, -1] = surf['n'][:, :, 0]
    return item, surf


def test_transmission_merges():
    item, surf = synthetic()
    F, W, n_seg = surf.shape
    slot_ifc = [0, 1, 3, 4, 5]
    s = np.array([1.0, 3.0])
    rows = np.arange(F * W * 4 * 9, dtype=np.float64).reshape(F * W, 4, 9)
    tx = analyses.Transmission(item, surf, slot_ifc, s, rows=rows, num_rays=3)
    T = item['t_sum'] / item['n_ok']
    thr = item['t_sum'] / 100.0
    assert np.array_equal(tx.T, T) and np.array_equal(tx.throughput, thr) and (tx.throughput <= tx.T).all()
    assert np.allclose(tx.poly_T, (T * s).sum(axis=1) / 4.0, rtol=4 * EPS, atol=0)
    assert np.allclose(tx.poly_throughput, (thr * s).sum(axis=1) / 4.0, rtol=4 * EPS, atol=0)
    assert tx.relative[0] == 1.0 and np.array_equal(tx.relative, tx.poly_throughput / tx.poly_throughput[0])
    assert np.array_equal(tx.surface_T, surf['t_sum'] / surf['n'])
    assert np.array_equal(tx.diattenuation_max, item['d_max'])
    assert np.array_equal(tx.diattenuation_mean, item['d_sum'] / item['n_ok'])
    loss = 1.0 - surf['t_sum'].sum(axis=(0, 1)) / surf['n'].sum(axis=(0, 1))
    assert [k for k, _i, _l in tx.surface_loss] == sorted(range(n_seg), key=lambda k: (-loss[k], k))
    assert all(i == slot_ifc[k] and l == loss[k] for k, i, l in tx.surface_loss)
    assert tx.surface_loss[0][2] == loss.max() and tx.surface_loss[-1][2] == 0.0
    assert tx.T_map.shape == (F, W, 3, 3) and tx.D_map.shape == (F, W, 3, 3) and tx.E1 is None
    assert np.shares_memory(tx.T_map, rows) and tx.T_map[1, 1, 2, 1] == rows[3, 0, 7] and tx.D_map[0, 1, 0, 2] == rows[1, 3, 2]
    other = analyses.Transmission(item, surf, slot_ifc, s, ref_field=2)
    assert other.relative[2] == 1.0 and other.T_map is None and np.array_equal(other.pupil_fraction, np.ones(F))
    # a vignetted field's grid spans less of the pupil: its rays weigh less
    box = np.array([1.0, 0.8, 0.6])
    vig = analyses.Transmission(item, surf, slot_ifc, s, pupil_fraction=box)
    assert np.array_equal(vig.relative, tx.poly_throughput * box / (tx.poly_throughput[0] * box[0]))
    assert np.array_equal(vig.poly_throughput, tx.poly_throughput) and vig.relative[0] == 1.0
    with pytest.raises(ValueError, match='pupil_fraction'):
        analyses.Transmission(item, surf, slot_ifc, s, pupil_fraction=[1.0, 1.0])
    with pytest.raises(ValueError, match='ref_field'):
        analyses.Transmission(item, surf, slot_ifc, s, ref_field=3)


def test_transmission_of_an_item_without_a_ray():
    item, surf = synthetic()
    item['n_ok'][1, 0] = 0
    item['t_sum'][1, 0] = item['d_sum'][1, 0] = 0.0
    item['d_max'][1, 0] = np.nan
    surf['n'][1, 0] = 0
    surf['t_sum'][1, 0] = 0.0
    tx = analyses.Transmission(item, surf, range(5), [1.0, 1.0])
    assert np.isnan(tx.T[1, 0]) and tx.throughput[1, 0] == 0.0 and np.isnan(tx.surface_T[1, 0]).all()
    assert tx.poly_T[1] == tx.T[1, 1] and tx.poly_throughput[1] == tx.throughput[1, 1] / 2.0
    assert np.isfinite(tx.relative).all()


# ---- transmission(): the Python layer over an engine double ------------------------------------------
class _Engine:
    def __init__(self, table):
        self.table = table
        self.calls = []

    def trace_pupil_grids(self, flds, wis, grid, opts_list, want_pupil=True):
        self.calls.append(('trace', len(flds), int(grid.num), int(opts_list[0].flags), int(opts_list[0].out_mode)))
        return [object()] * len(flds)

    def slot_interfaces(self, flags=0):
        return list(range(self.table.n_ifcs))

    def surface_transmission(self, results, trace_flags, wvl_idxs, coat_kind=None, coat_value=None, want_rows=True,
                             fields=False, on_device=False):
        n = len(results)
        self.calls.append(('tx', n, list(wvl_idxs), coat_kind, coat_value, want_rows, fields))
        item, surf = synthetic(n, 1, self.table.n_ifcs, seed=5)
        rows = np.zeros((n, 10 if fields else 4, 25)) if want_rows else None
        return rows, surf.reshape(n, -1), item.reshape(n)


@pytest.fixture
def doubled(monkeypatch):
    model = workloads.TableModel('dblgauss_c2')
    eng = _Engine(model.workload.table)

    def setup(opt_model, fld, wvl, kw, out_mode, *a, **k):
        from rayoptics_amd.trace import opts_from_kwargs
        return eng, fld.rox_field, eng.table.wvl_index(wvl), opts_from_kwargs(eng.table.n_ifcs, kw, out_mode)
    monkeypatch.setattr(analyses, '_launch_setup', setup)
    return model, eng


def test_transmission_python_layer(doubled):
    model, eng = doubled
    wvls = list(model.workload.table.wvls)
    F, W, N = len(model.fields), len(wvls), eng.table.n_ifcs
    tx = analyses.transmission(model, flds=model.fields, wvls=wvls, num_rays=5, fields=True)
    assert [c[0] for c in eng.calls] == ['trace', 'tx']             # one launch, one reduction
    _t, n, num, flags, mode = eng.calls[0]
    assert (n, num, mode) == (F * W, 5, abi.OUT_FULL)
    assert flags & abi.APPLY_VIGNETTING and flags & abi.CHECK_APERTURES
    _x, n, wis, kind, value, want_rows, fields = eng.calls[1]
    assert n == F * W and wis == [w for _f in range(F) for w in range(W)] and kind is None and value is None
    assert want_rows and fields
    assert tx.T.shape == (F, W) and tx.surface_T.shape == (F, W, N) and tx.relative.shape == (F,)
    assert tx.T_map.shape == (F, W, 5, 5) and tx.E1.shape == (F, W, 3, 5, 5) and tx.results is None
    want = [(2.0 - f.vlx - f.vux) * (2.0 - f.vly - f.vuy) / 4.0 for f in model.fields]
    assert tx.pupil_fraction.tolist() == want and want[0] == 1.0 and want[-1] < 1.0
    eng.calls.clear()
    tx = analyses.transmission(model, flds=model.fields[:1], wvls=wvls[:1], num_rays=5, check_apertures=False,
                               pupil_maps=False, keep_packets=True)
    assert not eng.calls[0][3] & abi.CHECK_APERTURES and eng.calls[1][5] is False and tx.T_map is None
    assert len(tx.results) == 1
    # the packets of an earlier call: nothing is traced
    eng.calls.clear()

    class _R:
        R = 25
    again = analyses.transmission(model, flds=model.fields[:1], wvls=wvls[:1], num_rays=5, packets=[_R()])
    assert [c[0] for c in eng.calls] == ['tx'] and np.array_equal(again.T, tx.T)
    with pytest.raises(ValueError, match='packets'):
        analyses.transmission(model, flds=model.fields[:1], wvls=wvls[:1], num_rays=6, packets=[_R()])


def test_transmission_coatings(doubled):
    model, eng = doubled
    tbl = eng.table
    N = tbl.n_ifcs
    kw = dict(flds=model.fields[:1], wvls=list(tbl.wvls)[:1], num_rays=5)
    analyses.transmission(model, coatings='ideal', **kw)
    kind, value = eng.calls[-1][3:5]
    assert kind.dtype == np.int32 and (kind == abi.COAT_IDEAL).all() and value.shape == (N, 2)
    analyses.transmission(model, coatings=0.99, **kw)
    kind, value = eng.calls[-1][3:5]
    nt = np.asarray(tbl.n_table)
    glass_air = [i for i in range(1, N - 1) if tbl.rows[i].mode == abi.TRANSMIT
                 and (nt[:, i - 1] == 1.0).all() != (nt[:, i] == 1.0).all()]
    assert 0 < len(glass_air) < N - 2                               # the double Gauss has cemented surfaces
    assert np.flatnonzero(kind == abi.COAT_FIXED).tolist() == glass_air and (kind[kind != abi.COAT_FIXED] == 0).all()
    assert (value[glass_air] == 0.99).all()
    analyses.transmission(model, coatings=(0.9, 0.8), **kw)
    assert (eng.calls[-1][4][glass_air] == (0.9, 0.8)).all()
    analyses.transmission(model, coatings={1: 'ideal', 2: 0.5, 3: (0.9, 0.8), 4: 'bare'}, **kw)
    kind, value = eng.calls[-1][3:5]
    assert kind[:5].tolist() == [0, 1, 2, 2, 0] and value[2].tolist() == [0.5, 0.5] and value[3].tolist() == [0.9, 0.8]


@pytest.mark.parametrize('bad', ['perfect', 1.5, -0.1, float('nan'), (0.9, 0.8, 0.7), (0.9, 1.2), {0: 'ideal'},
                                 {99: 0.9}, {'a': 0.9}, {1: 'shiny'}, {1: 1.5}, {1: (0.5, float('nan'))}, object()])
def test_transmission_refuses_bad_coatings(doubled, bad):
    model, eng = doubled
    with pytest.raises(ValueError, match='coatings'):
        analyses.transmission(model, flds=model.fields[:1], wvls=list(eng.table.wvls)[:1], num_rays=5, coatings=bad)
    assert eng.calls == []


def test_transmission_argument_checks(doubled):
    model, eng = doubled
    wvls = list(eng.table.wvls)
    for bad in (0, -3, 16385):
        with pytest.raises(ValueError, match='num_rays'):
            analyses.transmission(model, flds=model.fields, wvls=wvls, num_rays=bad)
    with pytest.raises(ValueError, match='items'):
        analyses.transmission(model, flds=[], wvls=wvls)
    with pytest.raises(ValueError, match='ref_field'):
        analyses.transmission(model, flds=model.fields, wvls=wvls, ref_field=len(model.fields))
    assert eng.calls == []


# ---- the C entry's argument errors, without a device --------------------------------------------
def call_tx(lib, over):
    """one rox_surface_transmission call on 2 items x 300 rays (ld 320) with ``over`` replacing
    arguments; ``sys`` and every packet pointer are addresses the entry never reads: each case
    fails its checks first"""
    a = dict(sys=8, trace_flags=0, tx_flags=0, n_items=2, ld=[320, 320], seg=[8, 8], status=[8, 8], n_rays=300,
             wvl_idx=[0, 1], n_coat=0, coat_kind=None, coat_value=None, rows=8, ld_rows=320, surf=8, item=8)
    a.update(over)
    n = max(len(a['ld']), 1)
    outs = (abi.Out * n)()
    for i in range(len(a['ld'])):
        outs[i].seg, outs[i].status, outs[i].fail_surf, outs[i].ld = a['seg'][i], a['status'][i], 8, a['ld'][i]
    keep = []

    def arr(v, dtype):
        if v is None:
            return None
        v = np.ascontiguousarray(np.asarray(v, dtype=dtype))
        keep.append(v)
        return v.ctypes.data

    return lib.rox_surface_transmission(a['sys'], a['trace_flags'], a['tx_flags'], a['n_items'], outs, a['n_rays'],
                                        arr(a['wvl_idx'], np.int32), a['n_coat'], arr(a['coat_kind'], np.int32),
                                        arr(a['coat_value'], np.float64), a['rows'], a['ld_rows'], a['surf'],
                                        a['item'], None)


def c_error_cases():
    bare3 = dict(n_coat=3, coat_kind=[0, 0, 0], coat_value=[(1.0, 1.0)] * 3)
    nan = float('nan')
    return [
        ('null sys', dict(sys=None), 'sys'),
        ('null outputs', dict(rows=None, surf=None, item=None), 'rows, surf and item'),
        ('n_items 0', dict(n_items=0), 'n_items'),
        ('n_items over', dict(n_items=abi.MAX_FOCUS_ITEMS + 1), 'n_items'),
        ('n_rays 0', dict(n_rays=0), 'n_rays'),
        ('n_rays over', dict(n_rays=2 ** 28 + 1), 'n_rays'),
        ('ld < n_rays', dict(ld=[320, 299]), 'item 1: ld'),
        ('ld_rows < n_rays', dict(ld_rows=299), 'ld_rows'),
        ('null seg', dict(seg=[None, 8]), 'item 0'),
        ('unknown flag', dict(tx_flags=2), 'tx_flags'),
        ('null wvl_idx', dict(wvl_idx=None), 'wvl_idx'),
        ('wvl_idx outside the table', dict(wvl_idx=[0, -1]), 'item 1: wvl_idx'),
        ('coating kind 7', dict(bare3, coat_kind=[0, 7, 0]), 'coat_kind[1]'),
        ('coating kind -1', dict(bare3, coat_kind=[0, 0, -1]), 'coat_kind[2]'),
        ('fixed value 1.5', dict(bare3, coat_kind=[0, 2, 0], coat_value=[(1, 1), (0.9, 1.5), (1, 1)]), 'coat_value[1][1]'),
        ('fixed value nan', dict(bare3, coat_kind=[0, 2, 0], coat_value=[(1, 1), (nan, 0.9), (1, 1)]), 'coat_value[1][0]'),
        ('fixed value negative', dict(bare3, coat_kind=[0, 0, 2], coat_value=[(1, 1), (1, 1), (-0.1, 0.9)]),
         'coat_value[2][0]'),
        ('kinds without values', dict(bare3, coat_value=None), 'coat_kind and coat_value'),
        ('n_coat 0', dict(bare3, n_coat=0), 'n_coat'),
    ]


@pytest.mark.parametrize('name,over,word', c_error_cases(), ids=[c[0] for c in c_error_cases()])
def test_c_argument_errors_need_no_device(lib, name, over, word):
    assert call_tx(lib, dict(over)) == -1
    msg = lib.rox_last_error().decode()
    assert msg.startswith('rox_surface_transmission: ') and word in msg, msg
