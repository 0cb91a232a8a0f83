"""Generates tests/golden/through_focus.npz by RUNNING THE REFERENCE ITSELF (imported through
oracle/refshim.py; build container only).

    python tests/golden/make_through_focus.py

For a few models (one field, the central wavelength) and a range of focus shifts `foc`, the
fixture holds what a through-focus scan needs per focus and what the reference makes of it:
  * the surface table (JSON), the field constants (rox_field bytes), the vignetting box,
    convert_to_opd;
  * per focus: trace.setup_pupil_coords(opm, fld, wvl, foc) (trace.py:608-624) as a
    rox_wavefront (table.wavefront_from_model with that focus's chief ray and reference sphere,
    the kind as the reference's sphere decides it) and image_pt = ref_sphere[0][:2];
  * per focus: the reference's refocus functions on a traced grid / fan --
    analyses.focus_wavefront(trace_wavefront(...), foc) (analyses.py:735-791, the RayGrid route)
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

# (model, field index, focus shifts: the RMS spot and RMS wavefront minima lie inside each range)
MODELS = (('dblgauss', -1, np.linspace(-1.2, 0.4, 11)),
          ('zmx_evenasph_c3', -1, np.linspace(-0.6, 0.8, 11)))
NUM_GRID, NUM_FAN = 13, 15


def fan_rows(fan_data, num):
    out = np.full((num, 5), np.nan)
    for r, item in enumerate(fan_data):
        if len(item) == 2:                      # ((px, py), (dx, dy, opd))
            out[r] = list(item[0]) + list(item[1])
        else:                                   # (px, py, nan): no ray
            out[r, :2] = item[:2]
    return out


def model_case(name, fi, focs):
    opm = getattr(rm, name)()
    osp = opm['osp']
    fld = osp['fov'].fields[fi]
    wvl = opm['seq_model'].central_wavelength()
    d = {}
    d['table_json'] = np.array(json.dumps(ra.SurfaceTable.from_seq_model(opm['seq_model']).to_dict()))
    d['field'] = np.frombuffer(bytes(field_from_model(opm, fld)), dtype=np.uint8).copy()   # rox_field
    d['wvl'] = np.float64(wvl)
    d['wvl_idx'] = np.int64(list(osp['wvls'].wavelengths).index(wvl))
    d['convert_to_opd'] = np.float64(1 / opm.nm_to_sys_units(wvl))
    vig_bbox = fld.vignetting_bbox(osp['pupil'], oversize=1.)
    d['bbox'] = np.array([vig_bbox[0], vig_bbox[1]], dtype=float)
    d['focs'] = np.array(focs, dtype=float)
    wfs, ipts, grids, fans = [], [], [], []
    grid_pkg = analyses.trace_wavefront(opm, fld, wvl, float(focs[0]), num_rays=NUM_GRID)
    fan_pkg = analyses.trace_fan(opm, fld, wvl, float(focs[0]), 1, num_rays=NUM_FAN)
    for foc in focs:
        ref_sphere, cr_pkg = trace.setup_pupil_coords(opm, fld, wvl, float(foc))
        wfs.append(wavefront_to_array(wavefront_from_model(opm, fld, cr_pkg, ref_sphere)))
        ipts.append(np.array(ref_sphere[0][:2], dtype=float))
        grids.append(np.array(analyses.focus_wavefront(opm, grid_pkg, fld, wvl, float(foc)), dtype=float))
        fans.append(fan_rows(analyses.focus_fan(opm, fan_pkg, fld, wvl, float(foc)), NUM_FAN))
    d['wavefront'] = np.stack(wfs)
    d['image_pt'] = np.stack(ipts)
    d['focus_wavefront'] = np.stack(grids)
    d['focus_fan'] = np.stack(fans)
    return {f'{name}/{k}': v for k, v in d.items()}


def main():
    out = {}
    for name, fi, focs in MODELS:
        out.update(model_case(name, fi, focs))
    path = os.path.join(HERE, 'through_focus.npz')
    np.savez_compressed(path, **out)
    print(f'through_focus.npz: {os.path.getsize(path) / 1024:.0f} KiB, {[m[0] for m in MODELS]}')


if __name__ == '__main__':
    main()
