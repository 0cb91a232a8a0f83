#!/usr/bin/env python3
"""Huygens PSFs on a detector's pixel grid, through focus, on the device: two launches trace every
(field, wavelength) item's pupil grid for the rays' points, directions and OPDs at the image, and
one rox_huygens_psf call sums their plane wavelets at every pixel of every focus plane -- a complex
GEMM on the fp64 matrix cores.  All wavelengths of a field land on one window, so the
polychromatic PSF is a plain weighted sum with the lateral colour in it.  Prints per field the
Strehl curve, the diffraction best focus, how far the blue PSF's peak sits from the red one's and
the share of the light in the window's border ring, and writes the polychromatic stack as .npy.
Stand-alone: the double Gauss table, its field constants and the reference spheres come from a
stored fixture (tests/golden/through_focus_map.npz, made by the reference's setup_pupil_coords);
behind ray-optics the call is ``huygens_psf(opt_model, pitch, size, focs)`` with the live
OpticalModel, which forms the spheres itself.

    python examples/huygens_psf.py [num_rays] [size] [pitch_um]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main(num_rays=128, size=96, pitch_um=2.0):
    import rayoptics_amd  # noqa: F401
    from rayoptics_amd import SurfaceTable, abi, analyses, workloads
    from rayoptics_amd.table import wavefront_from_array
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'through_focus_map.npz'))
    d = {k.split('/', 1)[1]: z[k] for k in z.files if k.startswith('dblgauss/')}
    tbl = SurfaceTable.from_dict(json.loads(str(d['table_json'])))
    wvls = [float(w) for w in d['wvls']]
    stored = [float(f) for f in d['focs']]
    k_ref = len(stored) // 2 + 2                        # the stored sphere nearest the paraxial focus
    flds = [abi.Field.from_buffer_copy(b.tobytes()) for b in d['fields']]

    class Model(workloads.TableModel):
        def setup_pupil_coords(self, fld, wvl, foc, image_pt=None, image_delta=None):
            f, w, k = self.fields.index(fld), wvls.index(float(wvl)), stored.index(float(foc))
            fld.rox_wavefront = wavefront_from_array(d['wavefront'][f, w, k])
            return (np.r_[d['image_pt'][f, w, k], 0.0], None, None, None), None

    ref = wvls.index(float(d['central_wvl']))
    m = Model(workloads.SimpleWorkload(tbl, flds, [tuple(d['image_pt'][f, ref, 0]) for f in range(len(flds))],
                                       ref_wvl_idx=ref), sys_units_per_nm=float(d['units_per_nm']))
    focs = np.linspace(stored[0], stored[-1], 17)       # any planes: the spheres stay where they are
    pitch = 1e-3 * float(pitch_um)
    order = [ref] + [w for w in range(len(wvls)) if w != ref]       # the window follows the first wavelength
    h = analyses.huygens_psf(m, pitch, size=int(size), focs=focs, flds=m.fields, wvls=[wvls[w] for w in order],
                             num_rays=int(num_rays), ref_foc=stored[k_ref])
    print(f'double Gauss, {len(flds)} fields x {len(wvls)} wavelengths, {num_rays}^2 rays, '
          f'{size} x {size} pixels of {pitch_um:g} um, {len(focs)} planes')
    for f in range(len(flds)):
        print(f'  field {f}: window origin ({h.origins[f, 0]:+.4f}, {h.origins[f, 1]:+.4f}), rays {h.n[f].tolist()}')
        for k, foc in enumerate(h.focs):
            red_blue = (h.peak_px[f, 1, k] - h.peak_px[f, 2, k]) if len(wvls) > 2 else np.zeros(2)
            print(f'    foc {foc:+.3f}  Strehl ' + ' / '.join(f'{s:.4f}' for s in h.strehl[f, :, k])
                  + f'  poly {h.poly_strehl[f, k]:.4f}  peak red - blue ({red_blue[0]:+d}, {red_blue[1]:+d}) px'
                  + f'  border ring {h.border_share[f, :, k].max():.3%}')
        print(f'    best focus (polychromatic Strehl): {h.best_focus[f]:+.4f} ({h.best_focus_kind[f]})')
    np.save('huygens_psf_poly.npy', h.poly)
    print('  wrote huygens_psf_poly.npy')


if __name__ == '__main__':
    a = sys.argv[1:4]
    main(*([int(v) for v in a[:2]] + [float(v) for v in a[2:3]]))
