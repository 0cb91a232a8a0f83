#!/usr/bin/env python3
"""What an anti-reflection coating buys, and what an aluminium mirror costs: thin-film stacks in
the transmission analysis (analyses.transmission with coatings.Coating; rox_surface_thinfilm over
the packets where they are).  First the reflectance of the coatings against wavelength and angle
on the host (Coating.coefficients, no GPU), then the double Gauss bare, with a quarter wave of
MgF2 and with a three-layer quarter-half-quarter coating on every glass-air surface -- per field
and wavelength, at the edge of the pupil, and the diattenuation -- and the RC telescope with
protected aluminium on both mirrors.  Stand-alone: the tables come from ray-optics_amd/data.

    python examples/transmission_coated.py [num_rays]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def aluminium(wvl_nm):
    """a rough n + ik of evaporated aluminium over the visible (0.6 + 5.4i at 450 nm, 1.6 + 7.6i at 650)"""
    return complex(0.6 + (wvl_nm - 450.0) * 5e-3, 5.4 + (wvl_nm - 450.0) * 1.1e-2)


def main():
    import rayoptics_amd  # noqa: F401
    from rayoptics_amd import abi, analyses, workloads
    from rayoptics_amd.coatings import Coating
    num = int(sys.argv[1]) if len(sys.argv) > 1 else 257
    mgf2 = Coating.quarter_wave(1.38, 550.0, name='MgF2 quarter wave')
    qhq = Coating([(1.38, 550.0 / 4 / 1.38), (2.1, 550.0 / 2 / 2.1), (1.62, 550.0 / 4 / 1.62)],
                  name='quarter-half-quarter')
    print('reflectance of a coated crown glass surface (n = 1.52), unpolarized, in per cent')
    print('  wvl (nm)      bare at 0 / 45 deg      MgF2 at 0 / 45 deg       QHQ at 0 / 45 deg')
    for wvl in (450.0, 500.0, 550.0, 600.0, 650.0):
        cells = []
        for c in (Coating([]), mgf2, qhq):
            co = c.coefficients(1.0, 1.52, wvl, np.cos(np.deg2rad([0.0, 45.0])))
            cells.append('   '.join(f'{v:8.3f}' for v in 50.0 * (co.Rs + co.Rp)))
        print(f'  {wvl:8.1f}   ' + '     '.join(cells))

    model = workloads.TableModel('dblgauss_c2')
    wvls = list(model.workload.table.wvls)
    kw = dict(flds=model.fields, wvls=wvls, num_rays=num)
    runs = [('bare', analyses.transmission(model, **kw)), ('MgF2', analyses.transmission(model, coatings=mgf2, **kw)),
            ('QHQ', analyses.transmission(model, coatings=qhq, **kw))]
    F, W = runs[0][1].T.shape
    print(f'double Gauss, {F} fields x {W} wavelengths, {num}^2 rays each: mean T, pupil minimum, largest '
          f'diattenuation')
    for f in range(F):
        for w in range(W):
            cells = [f'{name} {tx.T[f, w]:.4f} ({tx.items[f, w]["t_min"]:.4f}, D {tx.diattenuation_max[f, w]:.4f})'
                     for name, tx in runs]
            print(f'  field {f}  {wvls[w]:6.1f} nm   ' + '   '.join(cells))
    for name, tx in runs:
        print(f'  {name:5s} polychromatic T per field ' + ' '.join(f'{v:.4f}' for v in tx.poly_T) + '; costliest: '
              + ', '.join(f'interface {i} {100 * loss:.2f} %' for _k, i, loss in tx.surface_loss[:3]))

    rc = workloads.TableModel('rc_telescope_c4')
    mirrors = [i for i, r in enumerate(rc.workload.table.rows) if r.mode == abi.REFLECT]
    protected = Coating([(1.46, 550.0 / 2 / 1.46)], substrate=aluminium, name='Al + half wave of SiO2')
    t = analyses.transmission(rc, flds=rc.fields, wvls=list(rc.workload.table.wvls), num_rays=num,
                              coatings={i: protected for i in mirrors})
    print('RC telescope, protected aluminium on both mirrors: T per field '
          + ' '.join(f'{v:.4f}' for v in t.poly_T) + f'; largest diattenuation {np.nanmax(t.diattenuation_max):.5f}')


if __name__ == '__main__':
    main()
