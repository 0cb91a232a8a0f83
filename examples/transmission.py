#!/usr/bin/env python3
"""How much of the light arrives: Fresnel transmission and polarization ray tracing of the double
Gauss on the device -- one FULL launch of a dense pupil grid for every (field, wavelength), then
rox_surface_transmission over the packets where they are (analyses.transmission).  Prints the
transmission of every field and wavelength for bare surfaces and with a 99.5 % coating on every
glass-air surface, the surfaces that cost the most, the apodization of the pupil, the
diattenuation, and each field's transmission relative to the axial one with vignetting counted
(not radiometric relative illumination: no pupil-area, cos^4 or distortion term -- that is
examples/relative_illumination.py).  Stand-alone:
the table and the field constants come from ray-optics_amd/data/dblgauss_c2.json; behind
ray-optics the call is the same with the live OpticalModel.

    python examples/transmission.py [num_rays]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import rayoptics_amd  # noqa: F401
    from rayoptics_amd import analyses, workloads
    num = int(sys.argv[1]) if len(sys.argv) > 1 else 257
    model = workloads.TableModel('dblgauss_c2')
    wvls = list(model.workload.table.wvls)
    kw = dict(flds=model.fields, wvls=wvls, num_rays=num)
    bare = analyses.transmission(model, **kw)
    coated = analyses.transmission(model, coatings=0.995, pupil_maps=False, **kw)
    F, W = bare.T.shape
    print(f'double Gauss, {F} fields x {W} wavelengths, {num}^2 rays each')
    print('  field  wvl (nm)   T bare   T coated   throughput   pupil T min .. max    D mean    D max')
    for f in range(F):
        for w in range(W):
            it = bare.items[f, w]
            print(f'  {f:5d}  {wvls[w]:8.1f}  {bare.T[f, w]:7.4f}  {coated.T[f, w]:9.4f}  {bare.throughput[f, w]:11.4f}   '
                  f'{it["t_min"]:8.4f} .. {it["t_max"]:6.4f}  {bare.diattenuation_mean[f, w]:8.5f}  '
                  f'{bare.diattenuation_max[f, w]:7.5f}')
    print('  relative transmission including vignetting (field 0 = 1): bare '
          + ' '.join(f'{v:.4f}' for v in bare.relative) + '   coated ' + ' '.join(f'{v:.4f}' for v in coated.relative))
    print('  the surfaces that cost the most (bare): '
          + ', '.join(f'interface {i} {100 * loss:.2f} %' for _k, i, loss in bare.surface_loss[:4]))
    edge = bare.T_map[F - 1, W // 2]
    print(f'  edge field, central wavelength: T over the pupil {np.nanmin(edge):.4f} .. {np.nanmax(edge):.4f}, '
          f'{int(np.isnan(edge).sum())} of {edge.size} rays vignetted')


if __name__ == '__main__':
    main()
