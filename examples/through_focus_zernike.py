#!/usr/bin/env python3
"""Zernike fits of the wavefront through focus on the device: one trace of every (field,
wavelength) pupil grid at K focus shifts (rox_trace_through_focus_grids), then a least-squares
Fringe Zernike fit of every plane's OPD (rox_focus_zernike) without the rows leaving HBM.  Prints
the classical terms through focus, the residual after the fit, and where the defocus term
crosses zero.  Stand-alone: the double Gauss table, its field constants and the reference sphere
of each (field, wavelength, focus) come from a stored fixture (tests/golden/through_focus_mtf.npz,
made by the reference itself); behind ray-optics the call is the same with the live OpticalModel.

    python examples/through_focus_zernike.py"""
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
    res = analyses.through_focus_zernike(m, m.focs, num_rays=64, terms='fringe', n_terms=37, circle='bbox',
                                         **m.map_kwargs())
    ref = m.wvls.index(m.central_wvl)
    show = [3, 4, 5, 6, 7, 8]                           # defocus, astigmatism, coma, spherical
    print(f'double Gauss, {len(m.fields)} fields, {m.central_wvl} nm, 64^2 rays, Fringe 37; waves')
    print('                 ' + ' '.join(f'{res.names[j][:12]:>12}' for j in show) + '   rms  residual')
    for f in range(len(m.fields)):
        print(f'  field {f}')
        for k, foc in enumerate(res.focs):
            c = res.coef[f, ref, k]
            s = res.stats[f, ref, k]
            print(f'    foc {foc:+.4f} ' + ' '.join(f'{c[j]:12.5f}' for j in show)
                  + f'  {s["rms"]:.4f}  {s["rms_residual"]:.2e}')
        print(f'    defocus term crosses zero at {res.defocus_zero_field[f]:+.5f} '
              f'({res.defocus_zero_field_kind[f]})')


if __name__ == '__main__':
    main()
