#!/usr/bin/env python3
"""Where the reflected light goes: the two-reflection ghosts of the double Gauss
(analyses.ghost_analysis: every pair of refracting surfaces unfolded into a table of its own,
traced, weighted by rox_surface_thinfilm and reduced by rox_segment_foci where the packets are).
Bare surfaces first, then a quarter wave of MgF2 on every glass-air surface: the ten worst ghosts
of each by flux over patch area, what a 24 x 36 detector collects of them, and the ghost light's
foci inside the lens -- a focus in a glass element or near a surface is where coatings and cement
take the load.  Then the picture: irradiance maps of every ghost on the detector
(rox_weighted_maps: exact weighted histograms), the ghosts ranked by their brightest bin over the
signal's brightest bin, and the sum of all ghosts written as ghosts_total_<coating>.npy
([field, 48, 72], irradiance over signal flux per unit area).  Stand-alone: the table comes from
ray-optics_amd/data.

    python examples/ghosts.py [num_rays] [output directory]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import rayoptics_amd  # noqa: F401
    from rayoptics_amd import analyses, workloads
    from rayoptics_amd.coatings import Coating
    import numpy as np
    num = int(sys.argv[1]) if len(sys.argv) > 1 else 65
    out_dir = sys.argv[2] if len(sys.argv) > 2 else '.'
    model = workloads.TableModel('dblgauss_c2')
    table = model.workload.table
    wvls = list(table.wvls)
    mgf2 = Coating.quarter_wave(1.38, 550.0, name='MgF2 quarter wave')
    for name, tag, coat in (('bare surfaces', 'bare', None), ('MgF2 quarter waves', 'mgf2', mgf2)):
        g = analyses.ghost_analysis(model, flds=model.fields, wvls=wvls, num_rays=num, coatings=coat,
                                    detector=(12.0, 18.0), maps=(48, 72))
        print(f'double Gauss, {name}: {len(g.pairs)} ghosts, {len(g.skipped)} skipped, {num}^2 rays per field and '
              f'wavelength; total ghost flux over signal per field '
              + ' '.join(f'{v:.3e}' for v in g.poly_ratio.sum(axis=0)))
        print(g.table(10))
        glass = [f for f in g.internal_foci if table.n_table[0][f['gap']] != 1.0]
        print(f'  {len(g.internal_foci)} internal foci of the ghost light over all items, {len(glass)} of them in glass; '
              f'the tightest:')
        for f in sorted(g.internal_foci, key=lambda f: f['rms_min'])[:5]:
            medium = 'air' if table.n_table[0][f['gap']] == 1.0 else f'glass n = {table.n_table[0][f["gap"]]:.3f}'
            print(f'    ghost {f["pair"]} field {f["field"]} {wvls[f["wvl"]]:6.1f} nm: after interface {f["source"]} on pass '
                  f'{f["pass_"]}, in gap {f["gap"]} ({medium}), z = {f["zeta"]:8.3f} from its vertex, RMS {f["rms_min"]:.4f}')
        print('  by peak irradiance over the signal\'s peak (0.5 x 0.5 bins):')
        print('   pair (j, i)   field   peak/signal peak   rays in the brightest bin')
        for p, fig in g.ranking(by='peak')[:10]:
            f = int(np.argmax(np.where(np.isnan(g.peak_over_signal[p]), -np.inf, g.peak_over_signal[p])))
            j, i = g.pairs[p]
            print(f'   ({j:3d}, {i:3d})   {f:5d}   {fig:16.3e}   {int(g.ray_counts[p, f].flat[np.argmax(g.irradiance[p, f])]):8d}')
        with np.errstate(divide='ignore'):
            total_peak = g.irradiance_total.max(axis=(1, 2)) / g.signal_irradiance.max(axis=(1, 2))
        print('  all ghosts together, brightest bin over the signal\'s per field (inf: the image point is off the detector): '
              + ' '.join(f'{v:.3e}' for v in total_peak))
        path = os.path.join(out_dir, f'ghosts_total_{tag}.npy')
        np.save(path, g.irradiance_total)
        print(f'  total ghost irradiance map {g.irradiance_total.shape} -> {path}')


if __name__ == '__main__':
    main()
