"""Beam footprints without a GPU: the NumPy restatement of rox_surface_footprints
(tests/footprint_ref.py) against the reference's own vigcalc.max_aperture_at_surf on the golden
packets and against HostPackets.nseg, and the Python layer of analyses.beam_footprints --
BeamFootprints' merges, clear_apertures and every argument check -- over an engine double."""
import numpy as np
import pytest

import footprint_ref as FR
from helpers import fixture
from oracle import refshim
from rayoptics_amd import abi, workloads

if refshim.available():         # before rayoptics_amd.traceerror is imported: it adopts the reference's classes
    refshim.install()
from rayoptics_amd import analyses                  # noqa: E402
from rayoptics_amd.engine import FOOTPRINT_DTYPE    # noqa: E402
from rayoptics_amd.raypkg import HostPackets        # noqa: E402

GROUPS = [('dblgauss', 'rays_ap'), ('dblgauss', 'grid_f0'), ('dblgauss', 'grid_f2'), ('cell_phone', 'rays_ap')]


class _Host:
    def __init__(self, c):
        self.seg, self.op, self.status, self.fail_surf, self.pupil = c['seg'], c['op'], c['status'], c['fail_surf'], None


def packets(name, group):
    fx = fixture(name)
    c = fx[group]
    return fx.table, c, HostPackets(_Host(c), fx.table, int(c['flags']), abi.OUT_FULL, 587.6)


@pytest.mark.parametrize('name,group', GROUPS)
def test_nseg_is_hostpackets_nseg(name, group):
    table, c, pk = packets(name, group)
    ns = FR.nseg(table, int(c['flags']), c['status'], c['fail_surf'])
    assert ns.tolist() == [pk.nseg(r) for r in range(c['status'].shape[0])]


@pytest.mark.needs_reference
@pytest.mark.parametrize('name,group', GROUPS)
def test_semi_diameter_is_max_aperture_at_surf(name, group):
    """sqrt(r2_max) with partial records == the reference's max_aperture_at_surf on the same
    packets, exactly, for every surface; where the reference gives up (None: a ray ended before
    the surface) the restatement counted fewer records than rays"""
    from rayoptics.raytr.vigcalc import max_aperture_at_surf
    table, c, pk = packets(name, group)
    R = c['status'].shape[0]
    rayset = [[pk.pkg(r, named=True) for r in range(R)]]
    rec, _m, _t = FR.footprints(table, int(c['flags']), c['seg'], c['status'], c['fail_surf'], partial=True)
    some_none = False
    for i in range(c['seg'].shape[0]):
        ref = max_aperture_at_surf(rayset, i)
        if ref is None:
            some_none = True
            assert rec['n'][i] < R
        else:
            assert rec['n'][i] == R
            assert np.sqrt(rec['r2_max'][i]) == ref, (i, np.sqrt(rec['r2_max'][i]), ref)
    assert some_none                                    # every group holds blocked rays


def records(F, W, n_seg, seed=0):
    rng = np.random.default_rng(seed)
    rec = np.zeros((F, W, n_seg), FOOTPRINT_DTYPE)
    rec['n'] = 100
    rec['n_fail'][..., 1:] = rng.integers(0, 5, (F, W, n_seg, 4))
    rec['r2_max'] = rng.uniform(1.0, 9.0, (F, W, n_seg))
    rec['min'] = -rng.uniform(1.0, 3.0, (F, W, n_seg, 2))
    rec['max'] = rng.uniform(1.0, 3.0, (F, W, n_seg, 2))
    rec['cos_inc_min'] = rng.uniform(0.5, 1.0, (F, W, n_seg))
    rec['cos_inc_min'][:, :, 0] = np.nan                # the object: no incidence
    rec['r2_max'][:, :, n_seg - 1] = -np.inf            # a slot nothing reached
    return rec


def test_merges_and_clear_apertures():
    F, W, n_seg, B = 3, 2, 5, 4
    rec = records(F, W, n_seg)
    rng = np.random.default_rng(1)
    maps = rng.integers(0, 3, (F, W, n_seg, B, B)).astype(np.uint32)
    slot_ifc = [0, 1, 3, 4, 5]                          # interface 2: a filtered phantom
    bf = analyses.BeamFootprints(rec, slot_ifc, 6, abi.FILTER_PHANTOMS, maps, np.ones(n_seg))
    flat = rec.reshape(F * W, n_seg)
    want = np.sqrt(np.maximum(flat['r2_max'].max(axis=0), 0.0))
    assert np.array_equal(bf.semi_diameter[:-1], want[:-1]) and bf.semi_diameter[-1] == 0.0
    assert np.array_equal(bf.bbox[:, 0], flat['min'].min(axis=0)) and np.array_equal(bf.bbox[:, 1], flat['max'].max(axis=0))
    assert np.isnan(bf.max_aoi[0]) and (bf.max_aoi_item[0] == -1).all()
    for k in range(1, n_seg):
        f, w = bf.max_aoi_item[k]
        assert rec['cos_inc_min'][f, w, k] == rec['cos_inc_min'][:, :, k].min()
        assert bf.max_aoi[k] == np.degrees(np.arccos(rec['cos_inc_min'][f, w, k]))
    assert np.array_equal(bf.lost_by_field, rec['n_fail'].sum(axis=1)) and bf.lost_by_field.shape == (F, n_seg, 5)
    assert np.array_equal(bf.lost, rec['n_fail'].sum(axis=(0, 1)))
    assert np.array_equal(bf.field_maps, maps.astype(np.int64).sum(axis=1))
    assert np.array_equal(bf.union_map, maps.astype(np.int64).sum(axis=(0, 1)))
    assert np.array_equal(bf.overlap, (maps.sum(axis=1) > 0).sum(axis=0))
    ap = bf.clear_apertures()
    assert ap.shape == (6,) and ap[2] == 0.0 and np.array_equal(ap[slot_ifc], bf.semi_diameter)
    assert np.array_equal(bf.clear_apertures(0.1)[slot_ifc], bf.semi_diameter * 1.1)
    for bad in (-0.1, np.nan, np.inf):
        with pytest.raises(ValueError, match='margin'):
            bf.clear_apertures(bad)
    before = rec.copy()
    bf.clear_apertures(0.5)
    assert rec.tobytes() == before.tobytes()


class _Engine:
    """what beam_footprints asks of an engine, answered from canned records"""

    def __init__(self, table):
        self.table = table
        self.calls = []

    def trace_pupil_grids(self, flds, wis, grid, opts_list, want_pupil=True):
        self.calls.append(('trace', len(flds), int(grid.num), int(opts_list[0].flags), int(opts_list[0].out_mode)))
        return [object()] * len(flds)

    def slot_interfaces(self, flags=0):
        return list(range(self.table.n_ifcs))

    def surface_footprints(self, results, trace_flags, partial=True, ok_only=False, half_width=None, n_bins=0,
                           on_device=False, want_records=True):
        n_seg = self.table.n_ifcs
        self.calls.append(('fp', len(results), partial, ok_only, n_bins,
                           None if half_width is None else np.array(half_width)))
        rec = records(len(results), 1, n_seg, seed=3).reshape(len(results), n_seg) if want_records else None
        maps = np.ones((len(results), n_seg, n_bins, n_bins), np.uint32) if n_bins else None
        return rec, maps


@pytest.fixture
def doubled(monkeypatch):
    model = workloads.TableModel('dblgauss_c2')
    eng = _Engine(model.workload.table)

    def setup(opt_model, fld, wvl, kw, out_mode, *a, **k):
        from rayoptics_amd.trace import opts_from_kwargs
        return eng, fld.rox_field, eng.table.wvl_index(wvl), opts_from_kwargs(eng.table.n_ifcs, kw, out_mode)
    monkeypatch.setattr(analyses, '_launch_setup', setup)
    return model, eng


def test_beam_footprints_python_layer(doubled):
    model, eng = doubled
    wvls = list(model.workload.table.wvls)
    F, W, N = len(model.fields), len(wvls), eng.table.n_ifcs
    bf = analyses.beam_footprints(model, flds=model.fields, wvls=wvls, num_rays=33, maps=8, partial=False, ok_only=True)
    kinds = [c[0] for c in eng.calls]
    assert kinds == ['trace', 'fp', 'fp']               # one launch, the records, then the maps
    _t, n, num, flags, mode = eng.calls[0]
    assert (n, num, mode) == (F * W, 33, abi.OUT_FULL)
    assert flags & abi.APPLY_VIGNETTING and not flags & abi.CHECK_APERTURES
    assert eng.calls[1][2:5] == (False, True, 0) and eng.calls[2][2:5] == (False, True, 8)
    hw = eng.calls[2][5]
    r2 = bf.records['r2_max'].reshape(F * W, N).max(axis=0)
    assert np.array_equal(hw[:-1], np.sqrt(r2[:-1]) * analyses.FOOTPRINT_MAP_MARGIN) and hw[-1] == 1.0
    assert bf.records.shape == (F, W, N) and bf.maps.shape == (F, W, N, 8, 8)
    assert (bf.overlap == F).all() and (bf.union_map == F * W).all()
    assert bf.results is None
    eng.calls.clear()
    bf = analyses.beam_footprints(model, flds=model.fields[:1], wvls=wvls[:1], num_rays=5, check_apertures=True)
    assert [c[0] for c in eng.calls] == ['trace', 'fp'] and bf.maps is None and bf.union_map is None
    assert eng.calls[0][3] & abi.CHECK_APERTURES


def test_beam_footprints_argument_checks(doubled):
    model, eng = doubled
    wvls = list(model.workload.table.wvls)
    kw = dict(flds=model.fields, wvls=wvls)
    for bad in (0, -3, 16385):
        with pytest.raises(ValueError, match='num_rays'):
            analyses.beam_footprints(model, num_rays=bad, **kw)
    for bad in (-1, 513):
        with pytest.raises(ValueError, match='maps'):
            analyses.beam_footprints(model, maps=bad, **kw)
    with pytest.raises(ValueError, match='items'):
        analyses.beam_footprints(model, flds=[], wvls=wvls)
    with pytest.raises(ValueError, match='items'):
        analyses.beam_footprints(model, flds=model.fields * 400, wvls=wvls)
    assert eng.calls == []
