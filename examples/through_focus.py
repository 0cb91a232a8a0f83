#!/usr/bin/env python3
"""Through-focus scan on the device: one trace of the pupil grid, evaluated at K focus shifts in
the same launch (rox_trace_through_focus), reduced per focus to the RMS spot radius and the RMS
wavefront error, and the best focus of each curve.  Stand-alone: the double Gauss table, its
field constants and the reference sphere at each focus come from a stored fixture
(tests/golden/through_focus.npz, made by the reference's setup_pupil_coords); behind ray-optics
the call is the same with the live OpticalModel, which forms each focus's sphere itself.

    python examples/through_focus.py [num_rays]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main(num_rays=256):
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
    r = analyses.through_focus(m, m.fields[0], wvl, focs, num_rays=num_rays)
    print(f'double Gauss, {wvl:.1f} nm, {num_rays}^2 rays, {len(focs)} focus shifts in one launch')
    for f, n, s, w in zip(r.focs, r.stats['n'], r.rms_spot, r.rms_wavefront):
        print(f'  foc {f:+.3f}  {n:7d} rays  rms spot {s:.5f}  rms OPD {w:7.3f} waves')
    print(f'  best focus: spot {r.best_focus_spot:+.4f} ({r.best_focus_spot_kind}), '
          f'wavefront {r.best_focus_wavefront:+.4f} ({r.best_focus_wavefront_kind})')


if __name__ == '__main__':
    main(*(int(a) for a in sys.argv[1:2]))
