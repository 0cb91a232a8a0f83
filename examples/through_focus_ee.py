#!/usr/bin/env python3
"""Encircled energy through focus on the device: one trace of every (field, wavelength) pupil grid
at K focus shifts (rox_trace_through_focus_grids), then the geometric EE of every spot
(rox_focus_ee: exact ray counts and order-statistic radii) and the diffraction EE of every PSF
(rox_focus_psf then rox_focus_psf_ee) without the rows or the PSFs leaving HBM, and the
polychromatic merge per field on the host.  Prints EE50 / EE80 through focus and the best focus
by EE80.  Stand-alone: the double Gauss table, its field constants, the reference sphere of each
(field, wavelength, focus) and calc_psf_scaling's pitch come from stored fixtures
(tests/golden/through_focus_ee.npz and through_focus_mtf.npz, made by the reference itself);
behind ray-optics the call is the same with the live OpticalModel.

    python examples/through_focus_ee.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402


def main():
    import rayoptics_amd  # noqa: F401
    from rayoptics_amd import analyses
    import focus_map_fixture as FM
    golden = os.path.join(ROOT, 'tests', 'golden')
    m = FM.FocusMapFixtureModel(np.load(os.path.join(golden, 'through_focus_ee.npz')), 'dblgauss')
    pitch = np.load(os.path.join(golden, 'through_focus_mtf.npz'))['dblgauss/psf_scaling'][:, :, :, 1, 1]
    n = int(m.z['ndim'])
    geo = analyses.through_focus_ee(m, m.focs, fractions=(0.5, 0.8), num_rays=n, **m.map_kwargs())
    dif = analyses.through_focus_ee(m, m.focs, fractions=(0.5, 0.8), kind='diffraction', num_rays=n,
                                    maxdim=4 * n, pitch=pitch, **m.map_kwargs())
    print(f'double Gauss, {len(m.fields)} fields x {len(m.wvls)} wavelengths, {n}^2 rays, '
          f'{len(m.focs)} focus shifts; radii in um.  The diffraction EE is that of the {4 * n}^2 PSF window '
          f'(radius {1e3 * pitch.min() * 2 * n:.1f} um and up): NaN where a fraction lies beyond it')
    for f in range(len(m.fields)):
        print(f'  field {f}: polychromatic EE50 / EE80, geometric | diffraction')
        for k, foc in enumerate(geo.focs):
            g = ' / '.join(f'{1e3 * v:7.3f}' for v in geo.poly_ee_radius[f, k])
            d = ' / '.join(f'{1e3 * v:7.3f}' for v in dif.poly_ee_radius[f, k])
            print(f'    foc {foc:+.4f}  {g}  |  {d}   Strehl {dif.strehl[f, :, k].round(3)}')
        print(f'    best focus by EE80 (geometric): {geo.best_focus[f, 1]:+.4f} ({geo.best_focus_kind[f, 1]}); '
              f'by EE50 (diffraction): {dif.best_focus[f, 0]:+.4f} ({dif.best_focus_kind[f, 0]})')
    print(f'  best focus over the field: by EE80 (geometric) {geo.best_focus_all[1]:+.4f}, '
          f'by EE50 (diffraction) {dif.best_focus_all[0]:+.4f}')


if __name__ == '__main__':
    main()
