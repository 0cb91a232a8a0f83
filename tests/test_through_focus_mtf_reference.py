"""analyses.through_focus_mtf against the LIVE reference (build container only).  Each item's OTFs
are the line OTFs (tests/line_otf.py) of the reference's calc_psf (rayoptics/raytr/analyses.py:
848-875) of its focus_wavefront grid (:735-791), at its calc_psf_scaling pitch (:818-845); and
the orientation of the line OTF -- pixel j at image coordinate -p (j - M/2) -- agrees with the
reference's own spot centroid for an off-axis field with x and y components.  No GPU here: an
engine double serves the batched trace as oracle ROX_OUT_FAN launches
(test_through_focus_map_reference.py's double), rox_focus_psf as oracle.calc_psf and
rox_focus_mtf as the NumPy line OTF.  The GPU tests run the same comparisons against
tests/golden/through_focus_mtf.npz."""
import numpy as np
import pytest

import line_otf as LO
from oracle import oracle
from rayoptics_amd import abi
from test_through_focus_map_reference import map_oracle_engine

pytestmark = pytest.mark.needs_reference


@pytest.fixture(scope='module')
def ref():
    import sys
    import os
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), 'golden'))
    import refmodels as rm
    return rm


class _Host:
    """stands in for a torch tensor of PSFs: through_focus_mtf copies it to the host"""

    def __init__(self, a):
        self.a = a

    def cpu(self):
        return self

    def numpy(self):
        return self.a


class _Rows:
    """the FocusRows of the double: rows and status as host arrays, sliced per item group"""

    def __init__(self, rows, status):
        self.rows, self.status = np.asarray(rows), np.asarray(status)

    def to_host(self):
        return self.rows, self.status


@pytest.fixture()
def engine():
    from rayoptics_amd import session
    base = map_oracle_engine()

    class Engine(base):
        def trace_pupil_grids_focus(self, *a, **kw):
            stats, rows = super().trace_pupil_grids_focus(*a, **kw)
            return stats, _Rows(*rows.to_host())

        def focus_psf(self, focus_rows, ndim, maxdim, wave_scale, want_psf=True):
            from rayoptics_amd.engine import FOCUS_PSF_STATS_DTYPE
            rows, status = np.asarray(focus_rows.rows), np.asarray(focus_rows.status)
            n_items, K = rows.shape[:2]
            R = ndim * ndim
            psf = np.empty((n_items, K, maxdim, maxdim))
            for i in range(n_items):
                for k in range(K):
                    w = np.where(status[i, :R] == abi.OK, wave_scale[i] * rows[i, k, 2, :R], np.nan)
                    psf[i, k] = oracle.calc_psf(w.reshape(ndim, ndim), ndim, maxdim)
            return _Host(psf), np.zeros((n_items, K), dtype=FOCUS_PSF_STATS_DTYPE)

        def focus_mtf(self, psf, pitch, freqs, on_device=False):
            return LO.line_otf(psf.a, pitch, freqs)
    session._set_engine_factory(Engine)
    yield Engine
    session._set_engine_factory(None)


def _field(opm, x, y):
    """an osp field, or a new one aimed at the central wavelength as OpticalSpecs.update_model
    aims osp's (its chief ray kept, so that get_chief_ray_pkg does not re-aim it at whichever
    wavelength comes first)"""
    import rayoptics.raytr.trace as ref_trace
    from rayoptics.raytr.opticalspec import Field
    for f in opm['osp']['fov'].fields:
        if (f.x, f.y) == (x, y):
            return f
    fld = Field(x=x, y=y)
    wvl = opm['osp']['wvls'].central_wvl
    fld.aim_info = ref_trace.aim_chief_ray(opm, fld, wvl)
    fld.chief_ray = ref_trace.trace_chief_ray(opm, fld, wvl, 0.0)
    return fld


def test_otfs_are_the_line_otfs_of_the_references_psfs(ref, engine):
    import rayoptics.raytr.analyses as ref_an
    import rayoptics.raytr.trace as ref_trace
    from rayoptics_amd import analyses
    opm = ref.dblgauss()
    # two meridional fields and one with an x component
    flds = [_field(opm, 0.0, 0.0), _field(opm, 0.0, 0.7142857142857143), _field(opm, 0.18, 0.24)]
    wvls = [float(w) for w in opm['osp']['wvls'].wavelengths]
    focs = [-0.01, 0.0, 0.01]
    ndim, M = 32, 64
    nu = np.array([0.0, 10.0, 30.0, 60.0, 90.0])
    res = analyses.through_focus_mtf(opm, focs, nu, flds=flds, num_rays=ndim, maxdim=M, field_wts=[1.0] * 3,
                                     psf=True)
    assert res.otf.shape == (3, 3, 3, 2, nu.size) and list(res.meridional) == [True, True, False]
    for f, fld in enumerate(flds):
        for w, wvl in enumerate(wvls):
            grid_pkg = ref_an.trace_wavefront(opm, fld, wvl, focs[0], num_rays=ndim)
            for k, foc in enumerate(focs):
                opd = np.rollaxis(np.array(ref_an.focus_wavefront(opm, grid_pkg, fld, wvl, foc), dtype=float), 2)[2]
                ref_sphere, _cr = ref_trace.setup_pupil_coords(opm, fld, wvl, foc)
                fld.ref_sphere = ref_sphere
                _dx, dxp = ref_an.calc_psf_scaling(opm, fld, wvl, ndim, M)
                assert res.pitch[f, w, k] == dxp
                ref_psf = ref_an.calc_psf(opd, ndim, M)
                assert np.max(np.abs(res.psf[f, w, k] - ref_psf)) <= 1e-12, (f, w, k)
                exp = LO.line_otf(ref_psf, dxp, nu)
                assert np.array_equal(np.isnan(exp), np.isnan(res.otf[f, w, k]))
                assert np.nanmax(np.abs(res.otf[f, w, k] - exp)) <= 1e-12, (f, w, k)
    assert np.array_equal(res.tangential[:2], res.poly_mtf[:2, :, 1])
    assert np.array_equal(res.sagittal[:2], res.poly_mtf[:2, :, 0])
    assert np.isnan(res.tangential[2]).all() and np.isnan(res.sagittal[2]).all()


def test_orientation_agrees_with_the_references_spot_centroid(ref):
    """the reference's own chain -- focus_wavefront, calc_psf, calc_psf_scaling -- on a pupil grid
    fine enough that its PSF does not alias (256 rays across, maxdim 512): with pixel j at image
    coordinate -p (j - M/2) the PSF's centroid is the geometric centroid of the reference's rays
    about the image point within 5 %, in x and in y, for a field with both components"""
    import rayoptics.raytr.analyses as ref_an
    import rayoptics.raytr.trace as ref_trace
    opm = ref.dblgauss()
    fld = _field(opm, 0.18, 0.24)
    wvl = opm['osp']['wvls'].central_wvl
    n, M, foc = 256, 512, 0.0
    grid_pkg = ref_an.trace_wavefront(opm, fld, wvl, foc, num_rays=n)
    opd = np.rollaxis(np.array(ref_an.focus_wavefront(opm, grid_pkg, fld, wvl, foc), dtype=float), 2)[2]
    ref_sphere, _cr = ref_trace.setup_pupil_coords(opm, fld, wvl, foc)
    fld.ref_sphere = ref_sphere
    _dx, p = ref_an.calc_psf_scaling(opm, fld, wvl, n, M)
    pts = []
    for row in grid_pkg[0]:
        for _px, _py, ray_pkg in row:
            if ray_pkg is not None:
                ray = ray_pkg[0]
                pts.append((ray[-1][0] + foc / ray[-1][1][2] * ray[-1][1] - ref_sphere[0])[:2])
    geo = np.mean(pts, axis=0)
    got = LO.psf_centroid(ref_an.calc_psf(opd, n, M), p)
    assert np.all(np.abs(geo) > 3 * p)
    assert np.all(np.sign(got) == np.sign(geo))
    assert np.all(np.abs(got - geo) <= 0.05 * np.abs(geo)), (got / p, geo / p)
