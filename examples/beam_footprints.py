#!/usr/bin/env python3
"""Beam footprints on every surface of the double Gauss, on the device: one FULL launch of a dense
pupil grid for every (field, wavelength), then rox_surface_footprints over the packets where they
are (analyses.beam_footprints).  Prints, per surface, the semi-diameter the dense grid finds beside
the model's current max_aperture, the largest angle of incidence with the (field, wavelength)
that produced it, and the rays lost there with apertures checked.  Stand-alone: the table and the
field constants come from ray-optics_amd/data/dblgauss_c2.json; behind ray-optics the call is the
same with the live OpticalModel.

    python examples/beam_footprints.py [num_rays]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import rayoptics_amd  # noqa: F401
    from rayoptics_amd import abi, analyses, workloads
    num = int(sys.argv[1]) if len(sys.argv) > 1 else 257
    model = workloads.TableModel('dblgauss_c2')
    tbl = model.workload.table
    wvls = list(tbl.wvls)
    kw = dict(flds=model.fields, wvls=wvls, num_rays=num)
    bf = analyses.beam_footprints(model, maps=64, **kw)
    clipped = analyses.beam_footprints(model, check_apertures=True, **kw)
    F, W, _n = bf.records.shape
    print(f'double Gauss, {F} fields x {W} wavelengths, {num}^2 rays each; lengths in system units')
    print('  ifc  semi-diameter  max_aperture  max AOI (deg)  (field, wvl)   lost with apertures checked '
          '(missed / TIR / blocked)   fields overlapping')
    for k, i in enumerate(bf.slot_ifc):
        lost = clipped.lost[k]
        lit = bf.overlap[k][bf.overlap[k] > 0]
        print(f'  {i:3d}  {bf.semi_diameter[k]:13.6f}  {tbl.rows[i].max_aperture:12.6f}  {bf.max_aoi[k]:13.4f}  '
              f'{tuple(int(v) for v in bf.max_aoi_item[k])!s:12}   {lost[abi.MISSED_SURFACE]:8d} / {lost[abi.TIR]:6d} / '
              f'{lost[abi.BLOCKED]:8d}            {lit.mean() if lit.size else 0.0:.2f} of {F}')
    ap = bf.clear_apertures(margin=0.02)
    print('  clear apertures with a 2 % margin: ' + ' '.join(f'{v:.4f}' for v in ap))


if __name__ == '__main__':
    main()
