#!/usr/bin/env python3
"""MTF through focus on the device: one trace of every (field, wavelength) pupil grid at K focus
shifts (rox_trace_through_focus_grids), each plane's PSF (rox_focus_psf) and its line OTFs along
image x and y (rox_focus_mtf) without the PSFs leaving HBM, then the polychromatic merge per field
on the host.  Prints the polychromatic MTF through focus at a few frequencies and the best focus
per field, direction and frequency.  Stand-alone: the double Gauss table, its field constants,
the reference sphere of each (field, wavelength, focus) and calc_psf_scaling's pitch come from a
stored fixture (tests/golden/through_focus_mtf.npz, made by the reference itself); behind
ray-optics the call is the same with the live OpticalModel, which forms the spheres and the pitch
itself.

    python examples/through_focus_mtf.py"""
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
    m = FM.FocusMapFixtureModel(np.load(os.path.join(ROOT, 'tests', 'golden', 'through_focus_mtf.npz')),
                                'dblgauss')
    ndim, M = int(m.z['ndim']), int(m.z['maxdims'][0])
    pitch = m.z['psf_scaling'][:, :, :, 0, 1]               # calc_psf_scaling's delta_xp, mm
    nu = np.array([0.0, 10.0, 20.0, 40.0])                  # lp/mm
    r = analyses.through_focus_mtf(m, m.focs, nu, num_rays=ndim, maxdim=M, pitch=pitch, **m.map_kwargs())
    print(f'double Gauss, {len(m.fields)} fields x {len(m.wvls)} wavelengths, {ndim}^2 rays into {M}^2 PSFs, '
          f'{len(m.focs)} focus shifts')
    for f in range(len(m.fields)):
        kind = 'tangential (y) / sagittal (x)' if r.meridional[f] else 'y / x (field off the y-z plane)'
        print(f'  field {f}: polychromatic MTF {kind} at {", ".join(f"{v:g}" for v in nu)} lp/mm')
        for k, foc in enumerate(r.focs):
            y = ' '.join(f'{v:.3f}' for v in r.poly_mtf[f, k, 1])
            x = ' '.join(f'{v:.3f}' for v in r.poly_mtf[f, k, 0])
            print(f'    foc {foc:+.4f}  {y}  /  {x}   Strehl {r.strehl[f, :, k].round(3)}')
        for d, name in ((1, 'y'), (0, 'x')):
            print(f'    best focus along {name}: ' + ', '.join(
                f'{v:+.4f} ({kd})' for v, kd in zip(r.best_focus[f, d], r.best_focus_kind[f, d])))
    print('  best focus over the field: ' + ', '.join(
        f'{v:+.4f} ({kd})' for v, kd in zip(r.best_focus_all, r.best_focus_all_kind)))


if __name__ == '__main__':
    main()
