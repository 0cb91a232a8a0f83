"""Thin-film coatings without a GPU: physics identities of coatings.Coating.coefficients and of the
NumPy restatement (tests/thinfilm_ref.py, the recursive Airy summation), the two against each
other, the table building and the routing of analyses.transmission over an engine double, and the
argument errors rox_surface_thinfilm answers before it reads the system.  (What it can only refuse
once it has read the system -- a stack on a dummy, thin-lens or phase interface, a mirror's stack
without sub_index -- needs a device for the system: tests/test_gpu_thinfilm.py; the Python layer
refuses the same here.)

Bounds.  Closed forms and identities of a few layers: CLOSED = 64 * 2^-53 -- a layer is about
thirty complex operations on values of modulus <= 2, and the identities hold for the exact
values.  The two formulations against each other: AGREE = 4096 * 2^-53 -- up to 8 media, about 64
roundings each, and admittances up to 8 times the amplitudes they produce at cos >= 0.1 (the p
admittance N^2 / g of a metal).  Neither was taken from a run of either formulation."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import thinfilm_ref as TR
from rayoptics_amd import SurfaceTable, abi, analyses, coatings, workloads
from rayoptics_amd.coatings import Coating
from test_transmission_host import packet, plate, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = TR.EPS
CLOSED = 64 * EPS
AGREE = 4096 * EPS
AL = 0.96 + 6.7j                    # aluminium near 550 nm


@pytest.fixture(scope='module')
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location('rox_build', os.path.join(ROOT, 'ray-optics_amd', 'build.py'))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return abi.declare(C.CDLL(b.build()))


def airy_of(c, n_in, n_out, wvl, ci):
    ci = np.asarray(ci, dtype=np.float64)
    idx = c.indices(wvl)
    return TR.airy(n_in, n_out, idx, c.thicknesses, wvl, n_in * n_in * (1.0 - ci * ci), n_in * ci)


# ---- physics ----------------------------------------------------------------------------------
def test_the_restatement_and_coefficients_agree():
    rng = np.random.default_rng(7)
    worst = 0.0
    for trial in range(120):
        L = int(rng.integers(0, 7))
        lay = [(complex(rng.uniform(1.2, 2.5), float(rng.choice([0.0, 0.0, 0.05, 3.0])) * rng.uniform()),
                rng.uniform(0.0, 300.0)) for _ in range(L)]
        n1, n2 = rng.uniform(1.0, 1.8), rng.uniform(1.0, 1.8)
        if trial % 3 == 0:
            n2 = complex(rng.uniform(0.1, 2.0), rng.uniform(1.0, 7.0))
        ci, wvl = rng.uniform(0.1, 1.0, 9), rng.uniform(400.0, 700.0)
        co = Coating(lay).coefficients(n1, n2, wvl, ci)
        rs, rp, ts, tp = airy_of(Coating(lay), n1, n2, wvl, ci)
        ct = TR._sqrt_up(complex(n2) ** 2 - n1 * n1 * (1.0 - ci * ci)) / n2
        err = max(np.abs(co.rs - rs).max(), np.abs(co.rp - rp).max(), np.abs(co.ts - ts).max(),
                  np.abs(co.tp - tp * ci / ct).max())
        worst = max(worst, float(err))
    print(f'largest |coefficients - Airy| = {worst:.3g} ({worst / EPS:.0f} * 2^-53), bound {AGREE:.3g}')
    assert worst <= AGREE


def test_energy_is_conserved_by_lossless_stacks():
    ci = np.linspace(0.1, 1.0, 19)
    stacks = [Coating([(1.38, 99.6)]), Coating([(1.38, 100.0), (2.1, 120.0), (1.62, 80.0), (1.46, 90.0)]),
              Coating([])]
    for c in stacks:
        for n_in, n_out in ((1.0, 1.52), (1.52, 1.0), (1.7, 1.52)):
            lim = math.sqrt(max(0.0, 1.0 - min(1.0, n_out / n_in) ** 2))     # cos of the critical angle
            cc = ci[ci > lim + 0.05]
            co = c.coefficients(n_in, n_out, 550.0, cc)
            assert np.abs(co.Rs + co.Ts - 1.0).max() <= CLOSED and np.abs(co.Rp + co.Tp - 1.0).max() <= CLOSED
            rs, rp, ts, tp = airy_of(c, n_in, n_out, 550.0, cc)
            ct = np.sqrt(1.0 - (n_in / n_out) ** 2 * (1.0 - cc * cc))
            q = n_out * ct / (n_in * cc)
            assert np.abs(np.abs(rs) ** 2 + q * np.abs(ts) ** 2 - 1.0).max() <= CLOSED
            assert np.abs(np.abs(rp) ** 2 + q * np.abs(tp * cc / ct) ** 2 - 1.0).max() <= CLOSED
    # a layer in frustrated total reflection: an 80 nm air gap between two glasses beyond the
    # critical angle of glass-air (sin = 0.8 > 1 / 1.52); light tunnels, nothing is lost
    gap = Coating([(1.0, 80.0)])
    cc = np.array([0.6, 0.55, 0.5])
    co = gap.coefficients(1.52, 1.52, 550.0, cc)
    assert (co.Ts > 0.05).all() and (co.Ts < 0.95).all() and (np.abs(co.Ts - co.Tp) > 1e-3).all()
    assert np.abs(co.Rs + co.Ts - 1.0).max() <= CLOSED and np.abs(co.Rp + co.Tp - 1.0).max() <= CLOSED
    rs, rp, ts, tp = airy_of(gap, 1.52, 1.52, 550.0, cc)
    assert np.abs(np.abs(rs) ** 2 + np.abs(ts) ** 2 - 1.0).max() <= CLOSED
    assert np.abs(np.abs(rp) ** 2 + np.abs(tp) ** 2 - 1.0).max() <= CLOSED


def test_quarter_wave_and_half_wave_layers_at_normal_incidence():
    for n0, n1, ns in ((1.0, 1.38, 1.52), (1.0, 1.38, 1.9), (1.52, 1.7, 1.0)):
        qw = Coating.quarter_wave(n1, 550.0)
        assert qw.layers[0][1] == 550.0 / (4.0 * n1)
        want = ((n0 * ns - n1 * n1) / (n0 * ns + n1 * n1)) ** 2
        co = qw.coefficients(n0, ns, 550.0)
        assert abs(co.Rs - want) <= CLOSED and abs(co.Rp - want) <= CLOSED and abs(co.rs - co.rp) <= CLOSED
        rs, rp, _ts, _tp = airy_of(qw, n0, ns, 550.0, 1.0)
        assert abs(abs(rs) ** 2 - want) <= CLOSED and abs(abs(rp) ** 2 - want) <= CLOSED
        # a half-wave layer is absent
        hw = Coating([(n1, 550.0 / (2.0 * n1))])
        bare = ((n0 - ns) / (n0 + ns)) ** 2
        co = hw.coefficients(n0, ns, 550.0)
        assert abs(co.Rs - bare) <= CLOSED and abs(co.Ts - (1.0 - bare)) <= CLOSED
        rs, _rp, ts, _tp = airy_of(hw, n0, ns, 550.0, 1.0)
        assert abs(abs(rs) ** 2 - bare) <= CLOSED and abs(ns / n0 * abs(ts) ** 2 - (1.0 - bare)) <= CLOSED
    # MgF2 on crown glass: 1.26 % instead of 4.26 %
    assert abs(Coating.quarter_wave(1.38, 550.0).coefficients(1.0, 1.52, 550.0).Rs - 0.01260) < 1e-5


def test_transmission_is_the_same_in_both_directions():
    c = Coating([(1.38, 100.0), (2.1, 120.0), (1.46, 90.0)])
    ci = np.linspace(0.2, 1.0, 9)
    ct = np.sqrt(1.0 - (1.0 / 1.52) ** 2 * (1.0 - ci * ci))
    fwd = c.coefficients(1.0, 1.52, 600.0, ci)
    back = c.reversed().coefficients(1.52, 1.0, 600.0, ct)
    assert [m for m, _d in c.reversed().layers] == [1.46, 2.1, 1.38]
    assert np.abs(fwd.Ts - back.Ts).max() <= CLOSED and np.abs(fwd.Tp - back.Tp).max() <= CLOSED
    assert np.abs(fwd.Rs - back.Rs).max() <= CLOSED and np.abs(fwd.Rp - back.Rp).max() <= CLOSED


def test_a_micrometre_of_metal_is_the_bulk_metal():
    ci = np.linspace(0.1, 1.0, 10)
    film = Coating([(AL, 1000.0)]).coefficients(1.0, 1.52, 550.0, ci)
    bulk = Coating([]).coefficients(1.0, AL, 550.0, ci)
    for name in ('rs', 'rp'):
        assert np.abs(getattr(film, name) - getattr(bulk, name)).max() <= CLOSED, name
    # e^(-2 Im delta) = e^(-153): nothing comes through, and nothing overflowed on the way
    assert np.isfinite(np.array(film)).all() and (film.Ts < 1e-60).all() and (film.Tp < 1e-60).all()
    assert 0.90 < bulk.Rs[-1] < 0.93                     # aluminium reflects about 92 %
    rs, rp, ts, tp = airy_of(Coating([(AL, 1000.0)]), 1.0, 1.52, 550.0, ci)
    assert np.abs(rs - bulk.rs).max() <= CLOSED and np.abs(rp - bulk.rp).max() <= CLOSED
    assert np.abs(ts).max() < 1e-30 and np.isfinite(ts).all() and np.isfinite(tp).all()


def test_normal_incidence_does_not_polarize():
    for c, n_out in ((Coating([(1.46, 100.0)]), AL), (Coating([(1.38, 100.0), (2.1, 50.0)]), 1.52)):
        co = c.coefficients(1.0, n_out, 550.0, 1.0)
        assert abs(co.rs - co.rp) <= CLOSED and abs(co.Rs - co.Rp) <= CLOSED and abs(co.Ts - co.Tp) <= CLOSED
    # ... and the carried fields say the same: a coated plate on axis
    z = np.array([[0.0], [0.0], [1.0]])
    seg, status = packet([z, z, z, z])
    tbl = plate(1.5)
    c = Coating([(1.38, 100.0), (2.1, 50.0)])
    kind = np.array([0, abi.COAT_STACK, abi.COAT_STACK, 0], np.int32)
    first, thick, index, sub = coatings.stack_tables(tbl, {1: c, 2: c.reversed()})
    a = TR.thinfilm(tbl, 0, seg, status, 0, 587.6, kind, np.ones((4, 2)), TR.stack_dict(first, thick, index, sub))
    T, T1, T2, D = a['rows'][:, 0]
    assert D <= CLOSED and abs(T1 - T2) <= CLOSED
    one = c.coefficients(1.0, 1.5, 587.6).Ts
    assert abs(T - one * one) <= CLOSED and abs(a['Ts'][1, 0] - one) <= CLOSED and abs(a['Ts'][2, 0] - one) <= CLOSED


def test_materials():
    assert coatings.index_of(1.38, 500.0) == 1.38 and coatings.index_of(AL, 500.0) == AL
    assert coatings.index_of(lambda w: 1.4 + w / 1e4, 500.0) == 1.45
    assert coatings.index_of(([400.0, 600.0], [1.5, 1.4 + 0.2j]), 500.0) == 1.45 + 0.1j

    class Medium:
        def rindex(self, wvl):
            return 1.5 + (600.0 - wvl) * 1e-4
    assert coatings.index_of(Medium(), 500.0) == 1.51
    for bad in ('glass', -1.0, 1.5 - 0.1j, float('nan'), ([500.0, 400.0], [1.5, 1.5]), ([400.0], [1.5, 1.6])):
        with pytest.raises(ValueError, match='Coating'):
            coatings.index_of(bad, 500.0)
    for bad in ([(1.38,)], [(1.38, -1.0)], [(1.38, float('nan'))], [1.38], [(1.38, 1.0)] * 65):
        with pytest.raises(ValueError, match='Coating'):
            Coating(bad)
    with pytest.raises(ValueError, match='re <= 0'):
        Coating([(0.0 + 2.0j, 10.0)]).indices(500.0)


# ---- the tables -----------------------------------------------------------------------------
def two_wavelength_plate(mode='transmit', **kw):
    return SurfaceTable.from_prescription(
        [dict(cv=0, thi=10.0), dict(cv=0, thi=3.0, n=[1.52, 1.51], mode=mode, **kw), dict(cv=0, thi=5.0),
         dict(cv=0, thi=0)], wvls=(486.1, 656.3))


def test_stack_tables():
    tbl = two_wavelength_plate()
    disp = lambda w: 1.38 + (550.0 - w) * 1e-4          # noqa: E731
    c = Coating([(disp, 100.0), (2.1 + 0.01j, 50.0)])
    first, thick, index, sub = coatings.stack_tables(tbl, {2: c})
    assert first.dtype == np.int32 and first.tolist() == [0, 0, 0, 2, 2] and thick.tolist() == [100.0, 50.0]
    assert index.shape == (2, 2, 2) and sub is None
    assert index[0].tolist() == [[disp(486.1), 0.0], [2.1, 0.01]] and index[1, 0].tolist() == [disp(656.3), 0.0]
    first, thick, index, sub = coatings.stack_tables(tbl, {})
    assert first.tolist() == [0] * 5 and thick.shape == (0,) and index.shape == (2, 0, 2) and sub is None
    # a mirror: the substrate per wavelength
    mir = two_wavelength_plate(mode='reflect')
    al = ([400.0, 700.0], [0.5 + 4.8j, 1.9 + 8.4j])
    first, thick, index, sub = coatings.stack_tables(mir, {1: Coating([(1.46, 100.0)], substrate=al)})
    assert first.tolist() == [0, 0, 1, 1, 1] and sub.shape == (2, 4, 2)
    v = coatings.index_of(al, 486.1)
    assert sub[0, 1].tolist() == [v.real, v.imag] and sub[0, 2].tolist() == [1.0, 0.0]
    with pytest.raises(ValueError, match='mirror 1 has no substrate'):
        coatings.stack_tables(mir, {1: Coating([(1.46, 100.0)])})
    # where a Coating does not belong
    thin = two_wavelength_plate()
    thin.rows[1].profile = abi.THINLENS
    for i, t in ((0, tbl), (3, tbl), (1, two_wavelength_plate(mode='dummy')), (1, thin)):
        with pytest.raises(ValueError, match=f'interface {i} takes no Coating'):
            coatings.stack_tables(t, {i: c})
    ph = two_wavelength_plate()
    ph.rows[1].ph.kind = abi.PH_NONE + 1
    with pytest.raises(ValueError, match='interface 1 takes no Coating'):
        coatings.stack_tables(ph, {1: c})
    # more layers in all than a call takes: 66 surfaces of 64 layers
    many = SurfaceTable.from_prescription([dict(cv=0, thi=1.0)] + [dict(cv=0, thi=1.0, n=1.5 if i % 2 == 0 else 1.0)
                                                                   for i in range(66)] + [dict(cv=0, thi=0)])
    big = Coating([(1.38, 10.0)] * abi.MAX_COAT_LAYERS)
    assert coatings.stack_tables(many, {i: big for i in range(1, 65)})[0][-1] == abi.MAX_COAT_LAYERS_TOTAL
    with pytest.raises(ValueError, match='4160 layers in all'):
        coatings.stack_tables(many, {i: big for i in range(1, 66)})


# ---- transmission(): the routing over an engine double -------------------------------------------
class _Engine:
    def __init__(self, table):
        self.table = table
        self.calls = []

    def trace_pupil_grids(self, flds, wis, grid, opts_list, want_pupil=True):
        self.calls.append(('trace', len(flds)))
        return [object()] * len(flds)

    def slot_interfaces(self, flags=0):
        return list(range(self.table.n_ifcs))

    def _answer(self, n, want_rows, n_rows):
        item, surf = synthetic(n, 1, self.table.n_ifcs, seed=5)
        rows = np.arange(n * n_rows * 25, dtype=np.float64).reshape(n, n_rows, 25) if want_rows else None
        return rows, surf.reshape(n, -1), item.reshape(n)

    def surface_transmission(self, results, trace_flags, wvl_idxs, coat_kind=None, coat_value=None, want_rows=True,
                             fields=False, on_device=False):
        self.calls.append(('tx', len(results), list(wvl_idxs), coat_kind, coat_value))
        return self._answer(len(results), want_rows, 10 if fields else 4)

    def surface_thinfilm(self, results, trace_flags, wvl_idxs, wvls_nm=None, coat_kind=None, coat_value=None,
                         stack_first=None, layer_thickness=None, layer_index=None, sub_index=None, want_rows=True,
                         fields=False, on_device=False):
        self.calls.append(('film', len(results), list(wvl_idxs), list(wvls_nm), coat_kind, coat_value, stack_first,
                           layer_thickness, layer_index, sub_index))
        return self._answer(len(results), want_rows, 16 if fields else 4)


@pytest.fixture
def doubled(monkeypatch):
    model = workloads.TableModel('dblgauss_c2')
    eng = _Engine(model.workload.table)

    def setup(opt_model, fld, wvl, kw, out_mode, *a, **k):
        from rayoptics_amd.trace import opts_from_kwargs
        return eng, fld.rox_field, eng.table.wvl_index(wvl), opts_from_kwargs(eng.table.n_ifcs, kw, out_mode)
    monkeypatch.setattr(analyses, '_launch_setup', setup)
    return model, eng


def test_transmission_routes_a_coating(doubled):
    model, eng = doubled
    tbl = eng.table
    N, wvls = tbl.n_ifcs, list(tbl.wvls)
    nt = np.asarray(tbl.n_table)
    kw = dict(flds=model.fields[:2], wvls=wvls, num_rays=5)
    c = Coating([(1.38, 100.0), (lambda w: 2.0 + w * 1e-4, 50.0)])
    tx = analyses.transmission(model, coatings=c, fields=True, **kw)
    assert [x[0] for x in eng.calls] == ['trace', 'film']               # one launch, one reduction
    _f, n, wis, wv, kind, value, first, thick, index, sub = eng.calls[1]
    assert n == 2 * len(wvls) and wis == [0, 1, 2, 0, 1, 2] and wv == wvls * 2
    air = [bool((nt[:, i] == 1.0).all()) for i in range(N)]
    glass_air = [i for i in range(1, N - 1) if tbl.rows[i].mode == abi.TRANSMIT and air[i - 1] != air[i]]
    assert np.flatnonzero(kind == abi.COAT_STACK).tolist() == glass_air and (kind[kind != abi.COAT_STACK] == 0).all()
    assert first.tolist() == [2 * sum(j < i for j in glass_air) for i in range(N + 1)]
    assert sub is None and index.shape == (len(wvls), 2 * len(glass_air), 2)
    for k, i in enumerate(glass_air):                                   # flipped where the glass comes first
        want = [100.0, 50.0] if air[i - 1] else [50.0, 100.0]
        assert thick[2 * k:2 * k + 2].tolist() == want, i
        outer = 2 * k if air[i - 1] else 2 * k + 1
        assert index[:, outer].tolist() == [[1.38, 0.0]] * len(wvls)
        assert index[:, 4 * k + 1 - outer, 0].tolist() == [2.0 + w * 1e-4 for w in wvls]       # dispersion
    assert {air[i - 1] for i in glass_air} == {True, False}
    # complex fields from the 16 rows
    assert tx.E1.dtype == np.complex128 and tx.E1.shape == (2, len(wvls), 3, 5, 5)
    rows = np.arange(6 * 16 * 25, dtype=np.float64).reshape(6, 16, 25)
    assert tx.E1[1, 2, 0, 3, 4] == complex(rows[5, 4, 19], rows[5, 10, 19])
    assert tx.E2[0, 1, 2, 0, 0] == complex(rows[1, 9, 0], rows[1, 15, 0]) and tx.T_map[0, 0, 0, 1] == rows[0, 0, 1]
    # a dict: as written where the air comes first, the other kinds alongside
    eng.calls.clear()
    g_in, g_out = [i for i in glass_air if air[i - 1]][0], [i for i in glass_air if not air[i - 1]][0]
    cemented = [i for i in range(1, N - 1) if not air[i - 1] and not air[i]][0]
    assert (g_in, g_out, cemented) == (1, 2, 4)
    analyses.transmission(model, coatings={g_in: c, g_out: c, cemented: c, 3: 'ideal', 5: (0.9, 0.8)}, **kw)
    _f, n, wis, wv, kind, value, first, thick, index, sub = eng.calls[-1]
    assert kind[:6].tolist() == [0, 3, 3, 1, 3, 2] and value[5].tolist() == [0.9, 0.8] and first[-1] == 6
    assert thick[first[g_in]:first[g_in + 1]].tolist() == [100.0, 50.0]
    assert thick[first[g_out]:first[g_out + 1]].tolist() == [50.0, 100.0]
    assert thick[first[cemented]:first[cemented + 1]].tolist() == [100.0, 50.0]
    # without a Coating the call is the one it was
    eng.calls.clear()
    analyses.transmission(model, coatings=0.99, **kw)
    analyses.transmission(model, **kw)
    assert [x[0] for x in eng.calls] == ['trace', 'tx', 'trace', 'tx'] and eng.calls[3][3] is None


def test_transmission_refuses_a_coating_where_it_does_not_belong(doubled):
    model, eng = doubled
    kw = dict(flds=model.fields[:1], wvls=list(eng.table.wvls)[:1], num_rays=5)
    for bad in ({0: Coating([])}, {eng.table.n_ifcs - 1: Coating([])}, {1: [Coating([])]}):
        with pytest.raises(ValueError, match='coatings'):
            analyses.transmission(model, coatings=bad, **kw)
    assert eng.calls == []


def test_transmission_puts_a_metal_on_a_mirror(monkeypatch):
    model = workloads.TableModel('rc_telescope_c4')
    eng = _Engine(model.workload.table)

    def setup(opt_model, fld, wvl, kw, out_mode, *a, **k):
        from rayoptics_amd.trace import opts_from_kwargs
        return eng, fld.rox_field, eng.table.wvl_index(wvl), opts_from_kwargs(eng.table.n_ifcs, kw, out_mode)
    monkeypatch.setattr(analyses, '_launch_setup', setup)
    kw = dict(flds=model.fields[:1], wvls=list(eng.table.wvls), num_rays=5)
    al = Coating([(1.46, 100.0)], substrate=AL)
    analyses.transmission(model, coatings={1: al, 2: Coating([], substrate=AL)}, **kw)
    _f, n, wis, wv, kind, value, first, thick, index, sub = eng.calls[-1]
    assert kind.tolist() == [0, 3, 3, 0, 0] and first.tolist() == [0, 0, 1, 1, 1, 1] and thick.tolist() == [100.0]
    assert sub[0, 1].tolist() == [AL.real, AL.imag] and sub[0, 2].tolist() == [AL.real, AL.imag]
    with pytest.raises(ValueError, match='mirror 1 has no substrate'):
        analyses.transmission(model, coatings={1: Coating([(1.46, 100.0)])}, **kw)
    # a bare Coating goes on glass-air surfaces: this telescope has none, the call stays the old one
    eng.calls.clear()
    analyses.transmission(model, coatings=al, **kw)
    assert [x[0] for x in eng.calls] == ['trace', 'tx']


# ---- the binding and the C entry's argument errors, without a device -------------------------------
def test_abi_declares_the_entry(lib):
    assert 'rox_surface_thinfilm' in abi.EXPORTS
    assert lib.rox_surface_thinfilm.restype is C.c_int and len(lib.rox_surface_thinfilm.argtypes) == 20
    assert (abi.COAT_STACK, abi.MAX_COAT_LAYERS, abi.MAX_COAT_LAYERS_TOTAL) == (3, 64, 4096)
    with open(os.path.join(ROOT, 'include', 'roxtrace.h')) as f:
        src = f.read()
    assert 'ROX_COAT_STACK = 3' in src and '#define ROX_MAX_COAT_LAYERS 64' in src
    assert '#define ROX_MAX_COAT_LAYERS_TOTAL 4096' in src and abi.ABI_VERSION == 8 and lib.rox_abi_version() == 8


def call_tf(lib, over):
    """one rox_surface_thinfilm call on 2 items x 300 rays over 4 interfaces, a 2-layer stack on
    interface 1, with ``over`` replacing arguments; ``sys`` and every packet pointer are addresses
    the entry never reads: each case fails its checks first"""
    a = dict(sys=8, tx_flags=0, n_items=2, n_rays=300, wvl_idx=[0, 1], wvl=[486.1, 656.3], n_coat=4,
             coat_kind=[0, 3, 0, 0], coat_value=[(1.0, 1.0)] * 4, stack_first=[0, 0, 2, 2, 2],
             layer_thickness=[100.0, 50.0], layer_index=[(1.38, 0.0), (2.1, 0.01)], sub_index=None, rows=8,
             ld_rows=320, surf=8, item=8)
    a.update(over)
    outs = (abi.Out * 2)()
    for o in outs:
        o.seg, o.status, o.fail_surf, o.ld = 8, 8, 8, 320
    keep = []

    def arr(v, dtype):
        if v is None:
            return None
        v = np.ascontiguousarray(np.asarray(v, dtype=dtype))
        keep.append(v)
        return v.ctypes.data

    return lib.rox_surface_thinfilm(a['sys'], 0, a['tx_flags'], a['n_items'], outs, a['n_rays'],
                                    arr(a['wvl_idx'], np.int32), arr(a['wvl'], np.float64), a['n_coat'],
                                    arr(a['coat_kind'], np.int32), arr(a['coat_value'], np.float64),
                                    arr(a['stack_first'], np.int32), arr(a['layer_thickness'], np.float64),
                                    arr(a['layer_index'], np.float64), arr(a['sub_index'], np.float64), a['rows'],
                                    a['ld_rows'], a['surf'], a['item'], None)


def c_error_cases():
    nan = float('nan')
    return [
        ('null sys', dict(sys=None), 'sys'),
        ('unknown flag', dict(tx_flags=2), 'tx_flags'),
        ('n_rays 0', dict(n_rays=0), 'n_rays'),
        ('coating kind 4', dict(coat_kind=[0, 4, 0, 0]), 'coat_kind[1]'),
        ('65 layers', dict(stack_first=[0, 0, 65, 65, 65], layer_thickness=[1.0] * 65,
                           layer_index=[(1.5, 0.0)] * 65), 'stack_first[1]: 65 layers'),
        ('4097 layers in all', dict(n_coat=70, coat_kind=[0] + [3] * 68 + [0], coat_value=[(1.0, 1.0)] * 70,
                                    stack_first=[0, 0] + [min(64 * i, 4097) for i in range(1, 69)] + [4097],
                                    layer_thickness=[1.0] * 4097, layer_index=[(1.5, 0.0)] * 4097), 'more than 4096'),
        ('offsets that decrease', dict(stack_first=[0, 0, 2, 1, 2]), 'stack_first[2]'),
        ('offsets that do not start at 0', dict(stack_first=[1, 1, 2, 2, 2]), 'stack_first[0]'),
        ('layers without the kind', dict(coat_kind=[0, 0, 0, 0]), 'stack_first[1]'),
        ('the kind without offsets', dict(stack_first=None), 'coat_kind[1]'),
        ('offsets without kinds', dict(coat_kind=None, coat_value=None), 'stack_first'),
        ('negative thickness', dict(layer_thickness=[100.0, -1.0]), 'layer_thickness[1]'),
        ('nan thickness', dict(layer_thickness=[nan, 50.0]), 'layer_thickness[0]'),
        ('infinite thickness', dict(layer_thickness=[100.0, float('inf')]), 'layer_thickness[1]'),
        ('im n < 0', dict(layer_index=[(1.38, 0.0), (2.1, -0.01)]), 'layer_index[0][1]'),
        ('re n = 0', dict(layer_index=[(0.0, 1.0), (2.1, 0.0)]), 'layer_index[0][0]'),
        ('re n nan', dict(layer_index=[(nan, 0.0), (2.1, 0.0)]), 'layer_index[0][0]'),
        ('wvl 0', dict(wvl=[486.1, 0.0]), 'item 1: wvl'),
        ('wvl negative', dict(wvl=[-486.1, 656.3]), 'item 0: wvl'),
        ('wvl nan', dict(wvl=[nan, 656.3]), 'item 0: wvl'),
        ('layers without wvl', dict(wvl=None), 'wvl, layer_thickness and layer_index'),
        ('layers without thicknesses', dict(layer_thickness=None), 'wvl, layer_thickness and layer_index'),
        ('layers without indices', dict(layer_index=None), 'wvl, layer_thickness and layer_index'),
        ('kinds without values', dict(coat_value=None), 'coat_kind and coat_value'),
    ]


@pytest.mark.parametrize('name,over,word', c_error_cases(), ids=[c[0] for c in c_error_cases()])
def test_c_argument_errors_need_no_device(lib, name, over, word):
    assert call_tf(lib, dict(over)) == -1
    msg = lib.rox_last_error().decode()
    assert msg.startswith('rox_surface_thinfilm: ') and word in msg, msg


def test_the_old_entry_still_refuses_a_stack(lib):
    from test_transmission_host import call_tx
    assert call_tx(lib, dict(n_coat=3, coat_kind=[0, 3, 0], coat_value=[(1.0, 1.0)] * 3)) == -1
    assert 'coat_kind[1] = 3 is not a ROX_COAT_* kind' in lib.rox_last_error().decode()
