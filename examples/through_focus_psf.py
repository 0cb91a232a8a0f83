#!/usr/bin/env python3
"""Diffraction through focus on the device: one trace of the pupil grid at K focus shifts
(rox_trace_through_focus), then each focus's PSF and Strehl ratio straight from the rows in HBM
(rox_focus_psf).  Prints the Strehl curve, the diffraction best focus (the Strehl peak) beside
the geometric ones, and how far the PSF peak moves.  Stand-alone: the double Gauss table, its
field constants and the reference sphere at each focus come from a stored fixture
(tests/golden/through_focus.npz, made by the reference's setup_pupil_coords); behind ray-optics
the call is the same with the live OpticalModel, which forms each focus's sphere itself.

    python examples/through_focus_psf.py [num_rays] [maxdim]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main(num_rays=64, maxdim=256):
    import rayoptics_amd  # noqa: F401
    from rayoptics_amd import SurfaceTable, abi, analyses, workloads
    from rayoptics_amd.table import wavefront_from_array
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'through_focus.npz'))
    d = {k.split('/', 1)[1]: z[k] for k in z.files if k.startswith('dblgauss/')}
    tbl = SurfaceTable.from_dict(json.loads(str(d['table_json'])))
    fld = abi.Field.from_buffer_copy(d['field'].tobytes())
    focs = [float(f) for f in d['focs']]
    wvl = float(d['wvl'])

    class Model(workloads.TableModel):
        def setup_pupil_coords(self, fld, wvl, foc, image_pt=None, image_delta=None):
            k = focs.index(float(foc))              # the stored sphere of this focus
            fld.rox_wavefront = wavefront_from_array(d['wavefront'][k])
            return (np.r_[d['image_pt'][k], 0.0], None, None, None), None

    m = Model(workloads.SimpleWorkload(tbl, [fld], [tuple(d['image_pt'][0])], ref_wvl_idx=int(d['wvl_idx'])))
    m._units_per_nm = 1.0 / (float(d['convert_to_opd']) * wvl)
    m.fields[0]._vig_bbox = (d['bbox'][0], d['bbox'][1])
    r = analyses.through_focus_psf(m, m.fields[0], wvl, focs, num_rays=num_rays, maxdim=maxdim)
    print(f'double Gauss, {wvl:.1f} nm, {num_rays}^2 rays into {maxdim}^2 PSFs, {len(focs)} focus shifts')
    for k, f in enumerate(r.focs):
        u, v = np.unravel_index(int(np.argmax(r.psf[k])), r.psf[k].shape)
        print(f'  foc {f:+.3f}  {r.n[k]:7d} rays  Strehl {r.strehl[k]:.4f}  rms spot {r.stats["rms_spot"][k]:.5f}'
              f'  rms OPD {r.stats["opd_rms"][k]:7.3f} waves  PSF peak at ({u - maxdim // 2:+d}, {v - maxdim // 2:+d})')
    geo = analyses.ThroughFocus(r.focs, r.stats, None, None)
    print(f'  best focus: Strehl {r.best_focus_strehl:+.4f} ({r.best_focus_strehl_kind}), '
          f'spot {geo.best_focus_spot:+.4f} ({geo.best_focus_spot_kind}), '
          f'wavefront {geo.best_focus_wavefront:+.4f} ({geo.best_focus_wavefront_kind})')


if __name__ == '__main__':
    main(*(int(a) for a in sys.argv[1:3]))
