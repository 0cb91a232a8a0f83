"""analyses.through_focus_psf against the LIVE reference (build container only).  At every focus
the OPD grid handed to the PSF equals the reference's focus_wavefront on the RayGrid route
(rayoptics/raytr/analyses.py:735-791) bit for bit, the PSF is its calc_psf (:848-875) within
1e-12, and delta_x / delta_xp equal its calc_psf_scaling (:818-845) with that focus's reference
sphere exactly.  No GPU here: an engine double serves the through-focus rows as K oracle FAN
launches (test_through_focus_reference.py's double) and rox_focus_psf as oracle.calc_psf plus a
NumPy Strehl ratio.  The GPU tests run the same comparison against tests/golden/
through_focus_psf.npz, which the last test checks against the live reference."""
import numpy as np
import pytest

from oracle import oracle
from rayoptics_amd import abi
from test_through_focus_reference import focus_oracle_engine

pytestmark = pytest.mark.needs_reference

NDIM = 32


@pytest.fixture(scope='module')
def ref():
    import sys
    import os
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), 'golden'))
    import refmodels as rm
    return rm


def focus_psf_oracle_engine():
    base = focus_oracle_engine()

    class FocusPsfOracleEngine(base):
        """rox_focus_psf served as oracle.calc_psf of each plane's OPD grid; the grids are kept"""
        opd_grids = []

        def focus_psf(self, focus_rows, ndim, maxdim, wave_scale, want_psf=True):
            from rayoptics_amd.engine import FOCUS_PSF_STATS_DTYPE
            rows, status = focus_rows.to_host()
            K = rows.shape[0]
            R = ndim * ndim
            psf = np.empty((1, K, maxdim, maxdim))
            stats = np.zeros((1, K), dtype=FOCUS_PSF_STATS_DTYPE)
            type(self).opd_grids = []
            for k in range(K):
                w = np.where(status[:R] == abi.OK, wave_scale * rows[k, 2, :R], np.nan).reshape(ndim, ndim)
                type(self).opd_grids.append(w)
                psf[0, k] = oracle.calc_psf(w, ndim, maxdim)
                ok = ~np.isnan(w)
                n = int(ok.sum())
                stats['n'][0, k] = n
                stats['strehl'][0, k] = abs(np.exp(1j * 2 * np.pi * w[ok]).sum()) ** 2 / n ** 2 if n else np.nan
            return (psf if want_psf else None), stats

    return FocusPsfOracleEngine


class _Host:
    """stands in for a torch tensor: through_focus_psf reads psf[0] and copies it to the host"""

    def __init__(self, a):
        self.a = a

    def __getitem__(self, i):
        return _Host(self.a[i])

    def cpu(self):
        return self

    def numpy(self):
        return self.a


@pytest.fixture()
def engine():
    from rayoptics_amd import session
    cls = focus_psf_oracle_engine()

    class Engine(cls):
        def focus_psf(self, *a, **kw):
            psf, stats = super().focus_psf(*a, **kw)
            return (None if psf is None else _Host(psf)), stats
    session._set_engine_factory(Engine)
    yield Engine
    session._set_engine_factory(None)


def _focs(opm, wvl):
    fod = opm['analysis_results']['parax_data'].fod
    depth = opm.nm_to_sys_units(wvl) / (2 * fod.img_na ** 2)
    return list(np.linspace(-3 * depth, 3 * depth, 7))


@pytest.mark.parametrize('fi,maxdim', [(0, 64), (-1, 48), (-1, 64)])
def test_equals_the_references_focus_wavefront_calc_psf_and_scaling(ref, engine, fi, maxdim):
    import rayoptics.raytr.analyses as ref_an
    import rayoptics.raytr.trace as ref_trace
    from rayoptics_amd import analyses
    opm = ref.dblgauss()
    fld = opm['osp']['fov'].fields[fi]
    wvl = opm['seq_model'].central_wavelength()
    focs = _focs(opm, wvl)
    res = analyses.through_focus_psf(opm, fld, wvl, focs, num_rays=NDIM, maxdim=maxdim)
    grids = engine.opd_grids
    assert len(grids) == len(focs) and res.psf.shape == (len(focs), maxdim, maxdim)
    grid_pkg = ref_an.trace_wavefront(opm, fld, wvl, focs[0], num_rays=NDIM)
    radii = []
    for k, foc in enumerate(focs):
        exp = np.rollaxis(np.array(ref_an.focus_wavefront(opm, grid_pkg, fld, wvl, foc), dtype=float), 2)[2]
        assert np.array_equal(np.isnan(grids[k]), np.isnan(exp)) and np.isfinite(exp).sum() > 500
        if fi == 0:
            # on axis, at one focus of seven, the through-focus FAN rows themselves differ from the
            # reference by 8.9e-16 waves in 2 of 740 entries (through_focus gives the same rows):
            # the PSF stage adds nothing to that
            ok = ~np.isnan(exp)
            assert np.max(np.abs(grids[k][ok] - exp[ok])) <= np.spacing(np.max(np.abs(exp[ok]))), k
            assert np.count_nonzero(grids[k][ok] != exp[ok]) <= 2, k
        else:
            assert np.array_equal(grids[k], exp, equal_nan=True), k
        assert np.max(np.abs(res.psf[k] - ref_an.calc_psf(exp, NDIM, maxdim))) <= 1e-12, k
        ref_sphere, _cr = ref_trace.setup_pupil_coords(opm, fld, wvl, foc)
        fld.ref_sphere = ref_sphere
        dx, dxp = ref_an.calc_psf_scaling(opm, fld, wvl, NDIM, maxdim)
        assert res.delta_x[k] == dx and res.delta_xp[k] == dxp, k
        radii.append(ref_sphere[2])
    assert len(set(radii)) == len(radii)            # the sphere moves with foc: one radius per focus
    assert (res.best_focus_strehl, res.best_focus_strehl_kind) == analyses.best_focus(focs, -res.strehl)


def test_the_fixture_is_what_the_reference_gives(ref, engine):
    """tests/golden/through_focus_psf.npz (what the GPU tests compare with) against the live
    reference: its OPD grids, PSFs and scalings are those the reference gives now"""
    import os
    import rayoptics.raytr.analyses as ref_an
    import rayoptics.raytr.trace as ref_trace
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'through_focus_psf.npz'))
    opm = ref.dblgauss()
    wvl = opm['seq_model'].central_wavelength()
    for i, fi in enumerate((0, -1)):
        d = {k.split('/', 1)[1]: z[k] for k in z.files if k.startswith(f'f{i}/')}
        fld = opm['osp']['fov'].fields[fi]
        focs = [float(f) for f in d['focs']]
        assert np.array_equal(d['focs'], _focs(opm, wvl))
        grid_pkg = ref_an.trace_wavefront(opm, fld, wvl, focs[0], num_rays=NDIM)
        for k, foc in enumerate(focs):
            exp = np.rollaxis(np.array(ref_an.focus_wavefront(opm, grid_pkg, fld, wvl, foc), dtype=float), 2)[2]
            assert np.array_equal(d['opd'][k], exp, equal_nan=True), (i, k)
            ref_sphere, _cr = ref_trace.setup_pupil_coords(opm, fld, wvl, foc)
            assert d['ref_radius'][k] == ref_sphere[2]
            fld.ref_sphere = ref_sphere
            for j, M in enumerate(d['maxdims']):
                assert tuple(d['psf_scaling'][k, j]) == ref_an.calc_psf_scaling(opm, fld, wvl, NDIM, int(M))
        for j, k in enumerate(d['psf_focs']):
            assert np.array_equal(d['psf'][j], ref_an.calc_psf(d['opd'][k], NDIM, int(d['psf_maxdim'])))
