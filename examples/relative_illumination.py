#!/usr/bin/env python3
"""How bright the image corner is compared with the centre: radiometric relative illumination of
the double Gauss on the device -- one launch of a dense pupil grid for every (field, wavelength),
then rox_projected_solid_angle over the rows where they are (analyses.relative_illumination).  For
a Lambertian object the irradiance at an image point is proportional to the area the bundle
covers in the direction cosines it arrives with; cos^4, pupil aberration, distortion and
vignetting are all in that area.  Prints the relative illumination of every field, geometric and
with the Fresnel losses of bare and of quarter-wave coated surfaces, the effective F-number, the
direction of arrival and how much the boundary correction contributes (the handle on
convergence).  Stand-alone: the table and the field constants come from
ray-optics_amd/data/dblgauss_c2.json; behind ray-optics the call is the same with the live
OpticalModel, and ``sweep=n`` gives the curve against field.

    python examples/relative_illumination.py [num_rays]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import rayoptics_amd  # noqa: F401
    from rayoptics_amd import analyses, workloads
    from rayoptics_amd.coatings import Coating
    num = int(sys.argv[1]) if len(sys.argv) > 1 else 257
    model = workloads.TableModel('dblgauss_c2')
    wvls = list(model.workload.table.wvls)
    kw = dict(flds=model.fields, wvls=wvls, num_rays=num)
    geo = analyses.relative_illumination(model, **kw)
    bare = analyses.relative_illumination(model, coatings='bare', **kw)
    coated = analyses.relative_illumination(model, coatings=Coating.quarter_wave(1.38, 550.0), **kw)
    F, W = geo.ri.shape
    print(f'double Gauss, {F} fields x {W} wavelengths, {num}^2 rays each')
    print('  field  wvl (nm)   omega (sr)      RI   RI bare  RI coated   F/# eff   arrives at (L, M)     boundary')
    for f in range(F):
        for w in range(W):
            L, M = geo.chief_dir[f, w]
            print(f'  {f:5d}  {wvls[w]:8.1f}  {geo.omega[f, w]:11.6f}  {geo.ri[f, w]:6.4f}  {bare.ri_t[f, w]:8.4f}  '
                  f'{coated.ri_t[f, w]:9.4f}  {geo.fno_eff[f, w]:8.3f}   ({L:8.5f}, {M:8.5f})  '
                  f'{100 * geo.boundary_share[f, w]:7.2f} %')
    print('  polychromatic (field 0 = 1): geometric ' + ' '.join(f'{v:.4f}' for v in geo.poly_ri)
          + '   bare ' + ' '.join(f'{v:.4f}' for v in bare.poly_ri_t)
          + '   coated ' + ' '.join(f'{v:.4f}' for v in coated.poly_ri_t))
    print(f'  light arriving on axis, coated over bare: {np.mean(coated.omega_t[0] / bare.omega_t[0]):.4f}; '
          f'pupil map folded anywhere: {bool(geo.folded.any())}')


if __name__ == '__main__':
    main()
