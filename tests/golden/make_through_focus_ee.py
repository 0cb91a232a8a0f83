"""Generates tests/golden/through_focus_ee.npz by RUNNING THE REFERENCE ITSELF (imported through
oracle/refshim.py; build container only).

    python tests/golden/make_through_focus_ee.py

The double Gauss of tests/golden/make_through_focus_mtf.py -- its 3 wavelengths, the same 2
fields (on axis, and off axis with an x component, aimed at the central wavelength) and the same
K = 3 focus shifts -- on the square pupil grid analyses.through_focus_ee traces (trace_wavefront's
grid, :735-766) at NDIM.  Under the key prefix dblgauss/ (the layout tests/focus_map_fixture.py
reads): the model data as in through_focus_mtf.npz, and per (field, wavelength, focus) every
ray's transverse aberration about image_pt as focus_pupil_coords forms it (analyses.py:561-580),
in grid[a][b] order (a stepping pupil x), NaN where the reference traced no ray; the grid is
'ndim' rays over each field's 'bbox'.  NDIM keeps the file well under the size limit.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, '..', '..'))

import make_through_focus_mtf as mtf  # noqa: E402  (installs the reference shim through refmodels)
import refmodels as rm  # noqa: E402
import rayoptics_amd as ra  # noqa: E402
from rayoptics_amd.table import field_from_model, wavefront_from_model, wavefront_to_array  # noqa: E402

import rayoptics.raytr.trace as trace  # noqa: E402
import rayoptics.raytr.analyses as analyses  # noqa: E402

NDIM = 32
K = mtf.K
C_WAVEFRONT = mtf.C_WAVEFRONT


def transverse(grid, ref_sphere, foc):
    """[n, n, 2] each ray of a trace_ray_grid grid carried to focus shift foc as
    focus_pupil_coords carries it (analyses.py:568-576), about the image point; NaN: no ray"""
    n = len(grid)
    out = np.full((n, n, 2), np.nan)
    for a, row in enumerate(grid):
        for b, (_px, _py, ray_pkg) in enumerate(row):
            if ray_pkg is None:
                continue
            ray = ray_pkg[0]
            dist = foc / ray[-1][1][2]
            out[a, b] = (ray[-1][0] + dist * ray[-1][1] - ref_sphere[0])[:2]
    return out


def main():
    opm = rm.dblgauss()
    osp = opm['osp']
    wvls = [float(w) for w in osp['wvls'].wavelengths]
    central = float(osp['wvls'].central_wvl)
    flds = mtf.fields(opm, central)
    fod = opm['analysis_results']['parax_data'].fod
    depth = opm.nm_to_sys_units(central) / (2 * fod.img_na ** 2)
    focs = np.linspace(-2 * depth, 2 * depth, K)
    d = {}
    d['table_json'] = np.array(json.dumps(ra.SurfaceTable.from_seq_model(opm['seq_model']).to_dict()))
    d['fields'] = np.stack([np.frombuffer(bytes(field_from_model(opm, f)), dtype=np.uint8).copy()
                            for f in flds])
    d['field_xy'] = np.array([(f.x, f.y) for f in flds], dtype=float)
    d['field_wts'] = np.array([f.wt for f in flds], dtype=float)
    d['wvls'] = np.array(wvls)
    d['spectral_wts'] = np.array(osp['wvls'].spectral_wts, dtype=float)
    d['central_wvl'] = np.float64(central)
    d['units_per_nm'] = np.float64(opm.nm_to_sys_units(1.0))
    d['bbox'] = np.array([[b[0], b[1]] for b in (f.vignetting_bbox(osp['pupil'], oversize=1.) for f in flds)],
                         dtype=float)
    d['focs'] = np.array(focs, dtype=float)
    d['ref_focs'] = np.arange(K)
    d['ndim'] = np.int64(NDIM)
    F, W = len(flds), len(wvls)
    wfs = np.zeros((F, W, K, C_WAVEFRONT), dtype=np.uint8)
    ipts = np.zeros((F, W, K, 2))
    abr = np.zeros((F, W, K, NDIM, NDIM, 2))
    for fi, fld in enumerate(flds):
        for wi, wvl in enumerate(wvls):
            grid_pkg = analyses.trace_wavefront(opm, fld, wvl, float(focs[0]), num_rays=NDIM)
            for k, foc in enumerate(focs):
                foc = float(foc)
                ref_sphere, cr_pkg = trace.setup_pupil_coords(opm, fld, wvl, foc)
                wfs[fi, wi, k] = wavefront_to_array(wavefront_from_model(opm, fld, cr_pkg, ref_sphere))
                ipts[fi, wi, k] = ref_sphere[0][:2]
                abr[fi, wi, k] = transverse(grid_pkg[0], ref_sphere, foc)
    d['wavefront'] = wfs
    d['image_pt'] = ipts
    d['abr'] = abr                      # [F][W][K][NDIM][NDIM][2] about image_pt, NaN: no ray
    out = {f'dblgauss/{k}': v for k, v in d.items()}
    path = os.path.join(HERE, 'through_focus_ee.npz')
    np.savez_compressed(path, **out)
    print(f'through_focus_ee.npz: {os.path.getsize(path) / 1024:.0f} KiB')


if __name__ == '__main__':
    main()
