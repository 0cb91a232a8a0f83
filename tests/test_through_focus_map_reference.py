"""analyses.through_focus_map against the LIVE reference (build container only): every (field,
wavelength) item of the map is built as through_focus builds its one scan, so stats[f, w] equals
through_focus(flds[f], wvls[w]) bit for bit, and at every focus each item's rows equal the
reference's own focus_wavefront (RayGrid route, rayoptics/raytr/analyses.py:735-791) and
focus_fan (:277-345).  No GPU here: an engine double serves the batched entry as item-wise
oracle ROX_OUT_FAN launches (one per item and plane).  The same comparisons run on the GPU box
against the stored fixture (test_gpu_through_focus_map.py)."""
import numpy as np
import pytest

from oracle import oracle
from rayoptics_amd import abi

pytestmark = pytest.mark.needs_reference


@pytest.fixture(scope='module')
def ref():
    import sys
    import os
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), 'golden'))
    import refmodels as rm
    return rm


class _Rows:
    def __init__(self, rows, status):
        self._h = (rows, status)

    def to_host(self):
        return self._h


def map_oracle_engine():
    from oracle_engine import OracleEngine
    from test_through_focus_reference import _numpy_stats

    class MapOracleEngine(OracleEngine):
        """rox_trace_through_focus and rox_trace_through_focus_grids served as oracle
        ROX_OUT_FAN launches, one per (item, plane)"""

        def _item(self, fld, grid, wvl_idx, opts, planes):
            assert opts.out_mode == abi.OUT_FAN
            rows, status = [], None
            for p in planes:
                o = oracle.make_opts(flags=opts.flags, out_mode=abi.OUT_FAN, first_surf=opts.first_surf,
                                     last_surf=opts.last_surf, eps=opts.eps, fuzz=opts.fuzz, foc=p.foc,
                                     image_pt=(p.image_pt[0], p.image_pt[1]), wf=p.wf)
                h = oracle.trace_pupil_grid(self.table, fld, grid, wvl_idx, o)
                seg = np.asarray(h.seg).reshape(3, -1)
                rows.append(np.where(h.status == abi.OK, seg, np.nan))
                status = h.status
            rows = np.stack(rows)
            return _numpy_stats(rows, status), rows, status

        def trace_pupil_grid_focus(self, fld, grid, wvl_idx, opts, planes, want_rows=False,
                                   want_stats=True):
            stats, rows, status = self._item(fld, grid, wvl_idx, opts, planes)
            stats = stats if want_stats else None
            return (stats, _Rows(rows, status)) if want_rows else stats

        def trace_pupil_grids_focus(self, flds, wvl_idxs, grids, opts_list, planes, want_rows=False,
                                    want_stats=True):
            n = len(flds)
            assert len(wvl_idxs) == len(grids) == len(opts_list) == len(planes) == n
            assert len({(g.kind, g.num) for g in grids}) == 1
            assert len({(o.flags & (abi.FILTER_PHANTOMS | abi.FAST_FP64), o.first_surf, o.last_surf)
                        for o in opts_list}) == 1
            items = [self._item(*a) for a in zip(flds, grids, wvl_idxs, opts_list, planes)]
            stats = np.stack([i[0] for i in items]) if want_stats else None
            if not want_rows:
                return stats
            return stats, _Rows(np.stack([i[1] for i in items]), np.stack([i[2] for i in items]))
    return MapOracleEngine


@pytest.fixture()
def engine():
    from rayoptics_amd import session
    session._set_engine_factory(map_oracle_engine())
    yield
    session._set_engine_factory(None)


@pytest.mark.parametrize('model', ['dblgauss', 'zmx_evenasph_c3'])
def test_map_equals_through_focus_and_the_references_refocus_functions(ref, engine, model):
    import rayoptics.raytr.analyses as ref_an
    from rayoptics_amd import analyses
    opm = getattr(ref, model)()
    osp = opm['osp']
    flds, wvls = list(osp['fov'].fields), list(osp['wvls'].wavelengths)
    focs = [-0.04, 0.0, 0.025]
    num = 9
    m = analyses.through_focus_map(opm, focs, num_rays=num, rows=True)
    F, W = len(flds), len(wvls)
    assert m.stats.shape == (F, W, 3) and m.rows.shape == (F, W, 3, 3, num * num)
    assert m.ref_wvl == osp['wvls'].central_wvl
    np.testing.assert_array_equal(m.field_wts, [f.wt for f in flds])
    np.testing.assert_array_equal(m.spectral_wts, osp['wvls'].spectral_wts)
    n_ok = 0
    for f, fld in enumerate(flds):
        for w, wvl in enumerate(wvls):
            single = analyses.through_focus(opm, fld, wvl, focs, num_rays=num, rows=True)
            assert m.stats[f, w].tobytes() == single.stats.tobytes(), (model, f, w)
            assert np.array_equal(m.rows[f, w], single.rows, equal_nan=True), (model, f, w)
            grid_pkg = ref_an.trace_wavefront(opm, fld, wvl, focs[0], num_rays=num)
            for k, foc in enumerate(focs):
                exp = np.array(ref_an.focus_wavefront(opm, grid_pkg, fld, wvl, foc), dtype=float)[:, :, 2]
                np.testing.assert_array_equal(m.rows[f, w, k, 2].reshape(num, num), exp)
                n_ok += int(np.isfinite(exp).sum())
    assert n_ok > F * W * 3 * 20
    # the fan route, one field x every wavelength
    fld = flds[-1]
    fm = analyses.through_focus_map(opm, focs, flds=[fld], num_rays=11, xy=1, rows=True)
    for w, wvl in enumerate(wvls):
        fan_pkg = ref_an.trace_fan(opm, fld, wvl, focs[0], 1, num_rays=11)
        for k, foc in enumerate(focs):
            fan = ref_an.focus_fan(opm, fan_pkg, fld, wvl, foc)
            for r, item in enumerate(fan):
                if len(item) == 2:
                    assert tuple(fm.rows[0, w, k, :, r]) == tuple(item[1]), (model, w, k, r)
                else:
                    assert np.isnan(fm.rows[0, w, k, :, r]).all()


def test_the_fixture_is_what_the_reference_gives(ref, engine):
    """tests/golden/through_focus_map.npz (what the GPU tests scan) against the live reference:
    its per-(field, wavelength, focus) spheres give the stored focus_wavefront / focus_fan
    through through_focus_map"""
    import focus_map_fixture as FM
    from rayoptics_amd import analyses
    z = FM.load()
    for name in FM.MODELS:
        m = FM.FocusMapFixtureModel(z, name)
        focs = [m.focs[k] for k in m.ref_focs]
        g = analyses.through_focus_map(m, focs, num_rays=13, rows=True, **m.map_kwargs())
        f = analyses.through_focus_map(m, focs, num_rays=15, xy=1, rows=True, **m.map_kwargs())
        for fi in range(len(m.fields)):
            for wi in range(len(m.wvls)):
                for j in range(len(focs)):
                    exp = m.z['focus_wavefront'][fi, wi, j][:, :, 2].reshape(-1)
                    np.testing.assert_array_equal(g.rows[fi, wi, j, 2], exp)
                    exp = m.z['focus_fan'][fi, wi, j][:, 2:5].T
                    assert np.array_equal(f.rows[fi, wi, j], exp, equal_nan=True), (name, fi, wi, j)
