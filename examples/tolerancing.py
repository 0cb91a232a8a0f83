#!/usr/bin/env python3
"""What the lens does as built: tolerancing of the double Gauss from ONE nominal trace
(analyses.tolerance_sensitivity).  One FULL launch over every (field, wavelength), one
through-focus launch for the nominal OPD, one rox_wave_differentials call -- the first-order
change of every ray's optical path under every rigid-body, figure and index perturbation of every
surface, reduced to a covariance where the packets are -- and the rest is host algebra: the RMS
wavefront with each tolerance of a standard set at +- its magnitude after refocus, the worst
offenders, the RSS budget and a 10^4-trial Monte Carlo percentile table.  Stand-alone: the table,
the field constants and the reference spheres come from tests/golden/through_focus_map.npz; behind
ray-optics the call is the same with the live OpticalModel.

    python examples/tolerancing.py [num_rays] [commercial|precision]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    import rayoptics_amd  # noqa: F401
    from rayoptics_amd import analyses
    import focus_map_fixture as FM
    num = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    grade = sys.argv[2] if len(sys.argv) > 2 else 'commercial'
    m = FM.FocusMapFixtureModel(FM.load(), 'dblgauss')
    foc = m.focs[int(np.argmin(np.abs(m.focs)))]
    t0 = time.perf_counter()
    ts = analyses.tolerance_sensitivity(m, flds=m.fields, wvls=m.wvls, num_rays=num, foc=foc, grade=grade,
                                        field_wts=m.field_wts)
    t1 = time.perf_counter()
    F = len(m.fields)
    print(f'double Gauss, {F} fields x {len(m.wvls)} wavelengths, {num}^2 rays each, {len(ts.names)} tolerances '
          f'({grade}), compensator: {", ".join(ts.comp_names)}; {1e3 * (t1 - t0):.1f} ms')
    print(f'nominal RMS wavefront per field (waves): ' + ' '.join(f'{v:.4f}' for v in ts.nominal_rms)
          + f'   refocused by {ts.nominal_comp[0]:+.4f}: ' + ' '.join(f'{v:.4f}' for v in ts.nominal_compensated))
    print(ts.table(12))
    t0 = time.perf_counter()
    rms, pct = ts.monte_carlo(10000, dist='uniform', seed=1)
    t1 = time.perf_counter()
    print(f'Monte Carlo, 10000 trials on the host in {1e3 * (t1 - t0):.1f} ms; RMS wavefront (waves) per field')
    print('  percentile ' + ' '.join(f'field {f:d}' for f in range(F)))
    for p, row in zip((50, 90, 98), pct):
        print(f'  {p:9d}% ' + ' '.join(f'{v:7.4f}' for v in row))
    worst = int(np.argmax((ts.quadratic.fw[None, :] * ts.delta_rms).sum(axis=1)))
    sh = ts.image_shift[worst]
    print(f'image motion under "{ts.names[worst]}" at its magnitude, per field (x, y): '
          + ' '.join(f'({a:+.4f}, {b:+.4f})' for a, b in sh))


if __name__ == '__main__':
    main()
