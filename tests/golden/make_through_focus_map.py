"""Generates tests/golden/through_focus_map.npz by RUNNING THE REFERENCE ITSELF (imported through
oracle/refshim.py; build container only).

    python tests/golden/make_through_focus_map.py

For two models -- every field at every wavelength -- and a range of focus shifts `foc`, the
fixture holds what a field-and-wavelength through-focus map needs and what the reference makes
of it:
  * the surface table (JSON); per field the field constants (rox_field bytes), the vignetting box
    and the field weight; the wavelengths, the spectral weights and the central wavelength; the
    system units per nm;
  * per (field, wavelength, focus): trace.setup_pupil_coords(opm, fld, wvl, foc)
    (trace.py:608-624) as a rox_wavefront (table.wavefront_from_model with that focus's chief ray
    and reference sphere) and image_pt = ref_sphere[0][:2];
  * per (field, wavelength) at three of the focus shifts (REF_FOCS): the reference's refocus
    functions -- analyses.focus_wavefront(trace_wavefront(...), foc) (analyses.py:735-791)
    [num][num][3] and analyses.focus_fan(trace_fan(...), foc) (:277-345) as [num][5] rows
    (px, py, dx, dy, opd; NaN where the reference has no ray).
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

# (model, focus shifts): the double Gauss's 3 fields x 3 wavelengths, the .zmx even-asphere zoom's
MODELS = (('dblgauss', np.linspace(-1.2, 0.4, 11)),
          ('zmx_evenasph_c3', np.linspace(-0.6, 0.8, 11)))
REF_FOCS = (0, 5, 10)           # indices into the focus shifts of the stored reference outputs
NUM_GRID, NUM_FAN = 13, 15
C_WAVEFRONT = 512              # sizeof(rox_wavefront)


def fan_rows(fan_data, num):
    out = np.full((num, 5), np.nan)
    for r, item in enumerate(fan_data):
        if len(item) == 2:                      # ((px, py), (dx, dy, opd))
            out[r] = list(item[0]) + list(item[1])
        else:                                   # (px, py, nan): no ray
            out[r, :2] = item[:2]
    return out


def model_case(name, focs):
    opm = getattr(rm, name)()
    osp = opm['osp']
    flds = list(osp['fov'].fields)
    wvls = [float(w) for w in osp['wvls'].wavelengths]
    d = {}
    d['table_json'] = np.array(json.dumps(ra.SurfaceTable.from_seq_model(opm['seq_model']).to_dict()))
    d['fields'] = np.stack([np.frombuffer(bytes(field_from_model(opm, f)), dtype=np.uint8).copy()
                            for f in flds])
    d['field_wts'] = np.array([f.wt for f in flds], dtype=float)
    d['wvls'] = np.array(wvls)
    d['spectral_wts'] = np.array(osp['wvls'].spectral_wts, dtype=float)
    d['central_wvl'] = np.float64(osp['wvls'].central_wvl)
    d['units_per_nm'] = np.float64(opm.nm_to_sys_units(1.0))
    d['bbox'] = np.array([[b[0], b[1]] for b in (f.vignetting_bbox(osp['pupil'], oversize=1.) for f in flds)],
                         dtype=float)
    d['focs'] = np.array(focs, dtype=float)
    d['ref_focs'] = np.array(REF_FOCS)
    F, W, K = len(flds), len(wvls), len(focs)
    wfs = np.zeros((F, W, K, C_WAVEFRONT), dtype=np.uint8)
    ipts = np.zeros((F, W, K, 2))
    grids = np.zeros((F, W, len(REF_FOCS), NUM_GRID, NUM_GRID, 3))
    fans = np.zeros((F, W, len(REF_FOCS), NUM_FAN, 5))
    for fi, fld in enumerate(flds):
        for wi, wvl in enumerate(wvls):
            for k, foc in enumerate(focs):
                ref_sphere, cr_pkg = trace.setup_pupil_coords(opm, fld, wvl, float(foc))
                wfs[fi, wi, k] = wavefront_to_array(wavefront_from_model(opm, fld, cr_pkg, ref_sphere))
                ipts[fi, wi, k] = ref_sphere[0][:2]
            grid_pkg = analyses.trace_wavefront(opm, fld, wvl, float(focs[0]), num_rays=NUM_GRID)
            fan_pkg = analyses.trace_fan(opm, fld, wvl, float(focs[0]), 1, num_rays=NUM_FAN)
            for j, k in enumerate(REF_FOCS):
                foc = float(focs[k])
                grids[fi, wi, j] = np.array(analyses.focus_wavefront(opm, grid_pkg, fld, wvl, foc), dtype=float)
                fans[fi, wi, j] = fan_rows(analyses.focus_fan(opm, fan_pkg, fld, wvl, foc), NUM_FAN)
    d['wavefront'] = wfs
    d['image_pt'] = ipts
    d['focus_wavefront'] = grids
    d['focus_fan'] = fans
    return {f'{name}/{k}': v for k, v in d.items()}


def main():
    out = {}
    for name, focs in MODELS:
        out.update(model_case(name, focs))
    path = os.path.join(HERE, 'through_focus_map.npz')
    np.savez_compressed(path, **out)
    print(f'through_focus_map.npz: {os.path.getsize(path) / 1024:.0f} KiB, {[m[0] for m in MODELS]}')


if __name__ == '__main__':
    main()
