#!/usr/bin/env python3
"""rox_varying_blur and rox_image_warp (csrc/imgsim.hip) on geometric double Gauss PSFs: 5 x 5
nodes spanning the picture, tap counts in `--taps`, square scenes in `--sizes`, 1 and 3 channels,
every array in HBM.  The PSF stack is real -- analyses.image_simulation on the TableModel's three
prebuilt fields at 5 um pixels -- and is laid on the 5 x 5 grid by the node's distance from the
centre (the nearest of the three fields): the kernel's time does not depend on the taps' values.

A figure is the median over `--trials` windows of back-to-back calls between HIP events after a
warm-up call, with the windows' range beside it.  fp64_tflops counts 2 * S^2 operations per pixel
and per node whose box meets the pixel's tile (the kernel's own rule, restated here), against the
78.6 TFLOP/s vector peak of an MI355X; the arithmetic is unfused (one multiply, one add), so half
of that peak is the ceiling.  image_simulation_ms is the whole analysis call (3 x 1 node column,
three wavelengths, 128 x 128 rays per item) on a scene of the case's size.  host_route_ms is, in
the same run, what the device entry replaces: the PSF stack copied to the host,
scipy.signal.convolve2d per node on the weighted scene and the picture copied back -- run where it
takes under a minute (H*W*S^2*nodes <= 1e10), else null.

    python tools/image_simulation_bench.py [--taps 9 33 65] [--sizes 256 1024 4096] [--json out.json]"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TFLOPS = 78.6
TILE_H, TILE_W = 32, 64                                  # csrc/imgsim.hip


def window_ms(torch, fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def timed(torch, fn, reps, trials):
    fn()
    torch.cuda.synchronize()
    w = [window_ms(torch, fn, reps) for _ in range(trials)]
    return float(np.median(w)), [float(min(w)), float(max(w))]


def nodes_per_pixel(hat_cells, H, W, S, node_y, node_x):
    """the mean number of nodes the kernel walks per pixel: per tile the box [k(first halo row),
    k(last halo row) + 1] x the same in x, clipped to the grid"""
    r = (S - 1) // 2

    def per_tile(n, tile, node):
        lo = np.arange(0, n, tile)
        k_lo, _t = hat_cells(np.maximum(lo - r, 0).astype(np.float64), node)
        k_hi, _t = hat_cells(np.minimum(lo + tile - 1 + r, n - 1).astype(np.float64), node)
        return np.minimum(k_hi + 1, len(node) - 1) - k_lo + 1, np.minimum(lo + tile, n) - lo
    ny, hy = per_tile(H, TILE_H, node_y)
    nx, wx = per_tile(W, TILE_W, node_x)
    return float((ny * hy).sum() * (nx * wx).sum()) / (H * W)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--taps', nargs='+', type=int, default=[9, 33, 65])
    ap.add_argument('--sizes', nargs='+', type=int, default=[256, 1024, 4096])
    ap.add_argument('--channels', nargs='+', type=int, default=[1, 3])
    ap.add_argument('--model', default='dblgauss_c2')
    ap.add_argument('--pitch', type=float, default=0.005)
    ap.add_argument('--trials', type=int, default=5)
    ap.add_argument('--json')
    args = ap.parse_args()
    import torch
    from scipy.signal import convolve2d
    import rayoptics_amd  # noqa: F401
    from rayoptics_amd import analyses, session, workloads
    model = workloads.TableModel(args.model)
    wvls = list(model.workload.table.wvls)
    heights = np.array([np.hypot(*p) for p in model.workload.image_pts])
    eng = session.engine_for(model)
    rng = np.random.default_rng(1)
    results = []
    for S in args.taps:
        for n in args.sizes:
            H = W = n
            scene1 = rng.uniform(0.0, 1.0, (H, W))
            sim_kw = dict(flds=model.fields, node_px=(np.linspace(0.0, H - 1.0, 3), [(W - 1) / 2.0]), wvls=wvls,
                          num_rays=128, psf_size=S, on_device=True)
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                sim = analyses.image_simulation(model, scene1, args.pitch, **sim_kw)
                t_sim = timed(torch, lambda: analyses.image_simulation(model, scene1, args.pitch, **sim_kw), 1,
                              args.trials)
            # the three fields' PSFs on 5 x 5 nodes, by distance from the centre
            node_y, node_x = np.linspace(0.0, H - 1.0, 5), np.linspace(0.0, W - 1.0, 5)
            rad = np.hypot(*np.meshgrid(node_y - (H - 1) / 2.0, node_x - (W - 1) / 2.0, indexing='ij'))
            pick = np.abs(rad[..., None] / rad.max() * heights.max() - heights).argmin(axis=-1)
            stack1 = sim.psfs[0, :, 0][torch.from_numpy(pick).to(eng.device)].contiguous()      # [5, 5, S, S]
            disp = 0.01 * np.stack(np.meshgrid(node_y - (H - 1) / 2.0, node_x - (W - 1) / 2.0, indexing='ij'), axis=-1)
            per_px = nodes_per_pixel(analyses.hat_cells, H, W, S, node_y, node_x)
            for C in args.channels:
                scene = torch.from_numpy(rng.uniform(0.0, 1.0, (C, H, W))).to(eng.device)
                stack = stack1.expand(C, 5, 5, S, S).contiguous()
                flop = 2.0 * C * H * W * S * S * per_px
                reps = int(max(1, min(50, 2e11 // flop)))
                t_blur = timed(torch, lambda: eng.varying_blur(scene, stack, node_y, node_x, on_device=True), reps,
                               args.trials)
                blurred = eng.varying_blur(scene, stack, node_y, node_x, on_device=True)
                t_warp = timed(torch, lambda: eng.image_warp(blurred, node_y, node_x, disp, on_device=True),
                               max(reps, 10), args.trials)
                r = {'case': args.model, 'taps': S, 'scene': [C, H, W], 'nodes': [5, 5], 'pixel_pitch': args.pitch,
                     'nodes_per_pixel': per_px, 'reps': reps, 'trials': args.trials,
                     'varying_blur_ms': t_blur[0], 'varying_blur_ms_range': t_blur[1],
                     'fp64_tflops': flop / (t_blur[0] * 1e-3) / 1e12,
                     'share_of_vector_peak': flop / (t_blur[0] * 1e-3) / 1e12 / PEAK_TFLOPS,
                     'image_warp_ms': t_warp[0], 'image_warp_ms_range': t_warp[1],
                     'warp_gbps': 16.0 * C * H * W / (t_warp[0] * 1e-3) / 1e9,
                     'image_simulation_ms': t_sim[0] if C == 1 else None,
                     'image_simulation_ms_range': t_sim[1] if C == 1 else None,
                     'host_route_ms': None, 'host_route_vs_device': None, 'max_abs_diff_from_host': None}
                if C == 1 and float(H) * W * S * S * 25 <= 1e10:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    h_psf = stack.cpu().numpy()
                    h_scene = scene.cpu().numpy()
                    ky, ty = analyses.hat_cells(np.arange(H, dtype=np.float64), node_y)
                    kx, tx = analyses.hat_cells(np.arange(W, dtype=np.float64), node_x)
                    host = np.zeros((H, W))
                    for a in range(5):
                        wy = np.where(ky == a, 1.0 - ty, np.where(ky + 1 == a, ty, 0.0))
                        for b in range(5):
                            wx = np.where(kx == b, 1.0 - tx, np.where(kx + 1 == b, tx, 0.0))
                            host += convolve2d(h_scene[0] * (wy[:, None] * wx[None, :]), h_psf[0, a, b], mode='same')
                    back = torch.from_numpy(host).to(eng.device)
                    torch.cuda.synchronize()
                    t_host = (time.perf_counter() - t0) * 1e3
                    r.update(host_route_ms=t_host, host_route_vs_device=t_host / t_blur[0],
                             max_abs_diff_from_host=float((back - blurred[0]).abs().max()))
                print(json.dumps(r), flush=True)
                results.append(r)
                del scene, stack, blurred
            del sim, stack1
            torch.cuda.empty_cache()
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(results, fh, indent=1)


if __name__ == '__main__':
    main()
