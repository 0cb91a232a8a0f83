#!/usr/bin/env python3
"""Through-focus map on the device: every field at every wavelength of the double Gauss scanned
through focus in ONE launch (rox_trace_through_focus_grids), merged into white-light statistics
per field -- the best focus per field (field curvature from real rays) and the best single focus
for the whole field.  Stand-alone: the table, field constants, vignetting boxes, weights and the
reference sphere at each (field, wavelength, focus) come from a stored fixture
(tests/golden/through_focus_map.npz, made by the reference's setup_pupil_coords); behind ray-optics
the call is the same with the live OpticalModel, whose osp supplies fields, wavelengths and weights.

    python examples/through_focus_map.py [num_rays] [model]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402


def main(num_rays=128, model='dblgauss'):
    import rayoptics_amd  # noqa: F401
    from rayoptics_amd import analyses
    import focus_map_fixture as FM
    m = FM.FocusMapFixtureModel(FM.load(), model)
    r = analyses.through_focus_map(m, m.focs, num_rays=num_rays, **m.map_kwargs())
    F, W, K = r.stats.shape
    print(f'{model}: {F} fields x {W} wavelengths, {num_rays}^2 rays, {K} focus shifts in one launch')
    print('  per field and wavelength, best focus of the RMS spot:')
    for f in range(F):
        row = '  '.join(f'{w:.1f} nm {b:+.4f}' for w, b in zip(r.wvls, r.best_focus_spot[f]))
        print(f'    field {f}: {row}')
    print('  white light (spectral weights ' + ', '.join(f'{s:g}' for s in r.spectral_wts) + '):')
    for f in range(F):
        i = int(np.nanargmin(r.poly['rms_spot'][f]))
        print(f'    field {f}: best focus {r.best_focus_field[f]:+.4f} ({r.best_focus_field_kind[f]}), '
              f'rms spot {r.poly["rms_spot"][f, i]:.5f} at foc {r.focs[i]:+.3f}')
    print(f'  best focus for the whole field: {r.best_focus:+.4f} ({r.best_focus_kind})')


if __name__ == '__main__':
    main(*(int(a) for a in sys.argv[1:2]), *sys.argv[2:3])
