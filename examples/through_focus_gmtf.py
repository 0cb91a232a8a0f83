#!/usr/bin/env python3
"""Geometric MTF through focus on the device, beside the diffraction MTF: one trace of every
(field, wavelength) pupil grid at K focus shifts (rox_trace_through_focus_grids), then
rox_focus_gmtf sums exp(-2 pi i nu u) over the rays in HBM, along x, y and each field's
tangential and sagittal directions, at any frequency.  The double Gauss here is far from the
diffraction limit (transverse aberrations up to 0.1 mm), so the spot decides its MTF: the
geometric curve is the one a designer reads, and it exists for the field off the y-z plane, where
through_focus_mtf has no tangential / sagittal pair, and above the PSF grid's Nyquist frequency,
where through_focus_mtf is NaN.  Stand-alone: the table, its field constants and the reference
sphere of each (field, wavelength, focus) come from stored fixtures made by the reference itself
(tests/golden/through_focus_ee.npz, and calc_psf_scaling's pitch from through_focus_mtf.npz);
behind ray-optics the call is the same with the live OpticalModel.

    python examples/through_focus_gmtf.py"""
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
    nu = np.array([0.0, 2.0, 5.0, 10.0, 20.0, 40.0])            # lp/mm
    kw = m.map_kwargs()
    g = analyses.through_focus_gmtf(m, m.focs, nu, num_rays=64, lsf_bins=64, **kw)
    d = analyses.through_focus_mtf(m, m.focs, nu, num_rays=32, maxdim=128, pitch=pitch, **kw)
    freqs = ', '.join(f'{v:g}' for v in nu)
    print(f'double Gauss, {len(m.fields)} fields x {len(m.wvls)} wavelengths, {len(m.focs)} focus shifts; '
          f'geometric from 64^2 rays, diffraction from 32^2 rays into 128^2 PSFs')
    for f in range(len(m.fields)):
        t, s = g.dirs[f, 2], g.dirs[f, 3]
        print(f'  field {f}: tangential ({t[0]:+.3f}, {t[1]:+.3f}), sagittal ({s[0]:+.3f}, {s[1]:+.3f}); '
              f'polychromatic MTF at {freqs} lp/mm')
        for k, foc in enumerate(g.focs):
            print(f'    foc {foc:+.4f}  geometric T  ' + ' '.join(f'{v:.3f}' for v in g.tangential[f, k]))
            print(f'                 geometric S  ' + ' '.join(f'{v:.3f}' for v in g.sagittal[f, k]))
            print(f'                 geometric y  ' + ' '.join(f'{v:.3f}' for v in g.poly_mtf[f, k, 1]))
            print(f'                 diffraction y ' + ' '.join(f'{v:.3f}' for v in d.poly_mtf[f, k, 1]))
        print('    best focus along T: ' + ', '.join(
            f'{v:+.4f} ({kd})' for v, kd in zip(g.best_focus[f, 2], g.best_focus_kind[f, 2])))
        e = g.lsf_edges[f, 1, 2]
        print(f'    line spread along T at foc {g.focs[1]:+.4f}: {g.lsf_inside[f, 1, 2]:.3f} of the light within '
              f'+-{(e[-1] - e[0]) / 2:.3f} mm of the polychromatic centroid; edge spread at the centre bin '
              f'{g.esf[f, 1, 2, e.size // 2 - 1]:.3f}')
    print('  best focus over the field (geometric): ' + ', '.join(
        f'{v:+.4f} ({kd})' for v, kd in zip(g.best_focus_all, g.best_focus_all_kind)))


if __name__ == '__main__':
    main()
