"""Generates tests/golden/through_focus_psf.npz by RUNNING THE REFERENCE ITSELF (imported through
oracle/refshim.py; build container only).

    python tests/golden/make_through_focus_psf.py

The double Gauss at two fields (on axis and full field, the central wavelength), K = 7 focus
shifts spanning +-3 Rayleigh depths lambda / (2 NA^2) around the paraxial focus, an NDIM x NDIM
pupil grid.  Per field, under the key prefix f<i>/ (the layout tests/focus_fixture.py reads):
  * the surface table (JSON), the field constants (rox_field bytes), the vignetting box,
    convert_to_opd, wvl / wvl_idx, the focus shifts, and the paraxial enp_radius / exp_radius
    calc_psf_scaling reads;
  * per focus: trace.setup_pupil_coords(opm, fld, wvl, foc) (trace.py:608-624) as a
    rox_wavefront and image_pt = ref_sphere[0][:2], and the reference-sphere radius
    ref_sphere[2];
  * per focus: the OPD grid of analyses.focus_wavefront(trace_wavefront(...), foc)
    (analyses.py:735-791), np.rollaxis(grid, 2)[2], in waves, NaN where no ray passes;
  * per focus and per maxdim in MAXDIMS: calc_psf_scaling (:818-845) -> (delta_x, delta_xp);
  * analyses.calc_psf (:848-875) of the OPD grid at the three focus shifts PSF_FOCS, at one
    maxdim per field (a power of two on axis, not one at full field: the file stays small).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, '..', '..'))

import refmodels as rm  # noqa: E402  (installs the reference shim)
import rayoptics_amd as ra  # noqa: E402
from rayoptics_amd.table import field_from_model, wavefront_from_model, wavefront_to_array  # noqa: E402

import rayoptics.raytr.trace as trace  # noqa: E402
import rayoptics.raytr.analyses as analyses  # noqa: E402

NDIM = 32
MAXDIMS = (64, 48)              # 48: not a power of two (the block still fits: 9 + 32 <= 48)
FIELDS = ((0, 64), (-1, 48))    # (field index, the maxdim its stored PSFs use)
K = 7
PSF_FOCS = (0, 3, 6)            # indices into the focus shifts


def field_case(opm, fi, psf_maxdim):
    osp = opm['osp']
    fld = osp['fov'].fields[fi]
    wvl = opm['seq_model'].central_wavelength()
    fod = opm['analysis_results']['parax_data'].fod
    depth = opm.nm_to_sys_units(wvl) / (2 * fod.img_na ** 2)       # Rayleigh depth
    focs = np.linspace(-3 * depth, 3 * depth, K)
    d = {}
    d['table_json'] = np.array(json.dumps(ra.SurfaceTable.from_seq_model(opm['seq_model']).to_dict()))
    d['field'] = np.frombuffer(bytes(field_from_model(opm, fld)), dtype=np.uint8).copy()   # rox_field
    d['wvl'] = np.float64(wvl)
    d['wvl_idx'] = np.int64(list(osp['wvls'].wavelengths).index(wvl))
    d['convert_to_opd'] = np.float64(1 / opm.nm_to_sys_units(wvl))
    vig_bbox = fld.vignetting_bbox(osp['pupil'], oversize=1.)
    d['bbox'] = np.array([vig_bbox[0], vig_bbox[1]], dtype=float)
    d['focs'] = np.array(focs, dtype=float)
    d['enp_radius'] = np.float64(fod.enp_radius)
    d['exp_radius'] = np.float64(fod.exp_radius)
    d['ndim'] = np.int64(NDIM)
    d['maxdims'] = np.array(MAXDIMS, dtype=np.int64)
    d['psf_maxdim'] = np.int64(psf_maxdim)
    d['psf_focs'] = np.array(PSF_FOCS, dtype=np.int64)
    wfs, ipts, radii, opds, scal, psfs = [], [], [], [], [], []
    grid_pkg = analyses.trace_wavefront(opm, fld, wvl, float(focs[0]), num_rays=NDIM)
    for k, foc in enumerate(focs):
        ref_sphere, cr_pkg = trace.setup_pupil_coords(opm, fld, wvl, float(foc))
        wfs.append(wavefront_to_array(wavefront_from_model(opm, fld, cr_pkg, ref_sphere)))
        ipts.append(np.array(ref_sphere[0][:2], dtype=float))
        radii.append(float(ref_sphere[2]))
        grid = analyses.focus_wavefront(opm, grid_pkg, fld, wvl, float(foc))
        opd = np.rollaxis(np.array(grid, dtype=float), 2)[2]
        opds.append(opd)
        fld.ref_sphere = ref_sphere             # what calc_psf_scaling reads (ref_sphere[2])
        scal.append([analyses.calc_psf_scaling(opm, fld, wvl, NDIM, M) for M in MAXDIMS])
        if k in PSF_FOCS:
            psfs.append(analyses.calc_psf(opd, NDIM, psf_maxdim))
    d['wavefront'] = np.stack(wfs)
    d['image_pt'] = np.stack(ipts)
    d['ref_radius'] = np.array(radii)
    d['opd'] = np.stack(opds)                   # [K][NDIM][NDIM] waves
    d['psf_scaling'] = np.array(scal)           # [K][len(MAXDIMS)][2]: (delta_x, delta_xp)
    d['psf'] = np.stack(psfs)                   # [len(PSF_FOCS)][psf_maxdim][psf_maxdim]
    return d


def main():
    opm = rm.dblgauss()
    out = {}
    for i, (fi, pm) in enumerate(FIELDS):
        out.update({f'f{i}/{k}': v for k, v in field_case(opm, fi, pm).items()})
    path = os.path.join(HERE, 'through_focus_psf.npz')
    np.savez_compressed(path, **out)
    print(f'through_focus_psf.npz: {os.path.getsize(path) / 1024:.0f} KiB')


if __name__ == '__main__':
    main()
