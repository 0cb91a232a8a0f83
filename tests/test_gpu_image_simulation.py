"""rox_varying_blur and rox_image_warp on the device against their NumPy restatement
(tests/imgsim_ref.py) with ==: the header fixes every operation and its order and the build
contracts nothing, so there is no tolerance -- only the sign of a zero is free.  Seeded random
scenes with negative values, random non-negative PSFs; picture sizes of one pixel, of less than
and of several 32 x 64 tiles; tap counts from 1 to the largest, below and above the 33 tap rows a
staged halo holds at S = 65; node grids of one node, one row, cells wider and narrower than a
tile, nodes outside the picture; both edge rules.  Then analyses.image_simulation on the double
Gauss against the pipeline assembled by hand."""
import warnings

import numpy as np
import pytest

import imgsim_ref as IR
from packets_fixture import torch  # noqa: F401 (the fixture)
from rayoptics_amd import abi, workloads

pytestmark = pytest.mark.gpu


def grid(name, H, W):
    if name == '1x1':
        return [H / 2.0], [W / 2.0]
    if name == '1x3':
        return [3.0], np.linspace(0.0, W - 1.0, 3) if W > 1 else [-1.0, 0.0, 2.5]
    if name == '3x2':
        return np.linspace(0.0, max(H - 1.0, 1.0), 3), [W * 0.25, W * 0.8]
    if name == '4x5':                                    # non-uniform, nodes outside the frame, one on a pixel
        return [-4.5, np.floor(0.3 * H), 0.55 * H, H + 6.0], [-10.0, 0.2 * W, 0.5 * W + 0.25, 0.9 * W, W + 3.5]
    assert name == '9x9'                                 # cells of 4.5 and 8.6 px: many nodes meet one tile
    return np.linspace(0.0, H - 1.0, 9), np.linspace(0.0, W - 1.0, 9)


# (H, W, S, node grid, C, edge)
BLUR_CASES = [(1, 1, 1, '1x1', 1, 'zero'), (1, 1, 9, '1x3', 1, 'replicate'), (1, 1, 65, '3x2', 1, 'zero'),
              (37, 70, 1, '3x2', 3, 'zero'), (37, 70, 3, '4x5', 1, 'replicate'), (37, 70, 9, '9x9', 3, 'zero'),
              (37, 70, 9, '9x9', 1, 'replicate'), (37, 70, 33, '1x3', 1, 'zero'), (37, 70, 65, '4x5', 1, 'replicate'),
              (130, 67, 3, '1x1', 3, 'replicate'), (130, 67, 9, '4x5', 1, 'zero'), (130, 67, 33, '3x2', 1, 'zero'),
              (130, 67, 33, '1x1', 1, 'replicate'), (130, 67, 65, '1x3', 1, 'replicate'),
              (130, 67, 65, '1x1', 1, 'zero')]


def blur_inputs(H, W, S, name, C):
    rng = np.random.default_rng(1000 * H + 10 * S + C + len(name))
    node_y, node_x = (np.asarray(a, dtype=np.float64) for a in grid(name, H, W))
    scene = rng.normal(size=(C, H, W))
    psf = rng.uniform(0.0, 1.0, size=(C, len(node_y), len(node_x), S, S))
    psf[rng.random(psf.shape) < 0.1] = 0.0
    return scene, psf, node_y, node_x


@pytest.fixture(scope='module')
def eng(torch):
    from rayoptics_amd.engine import TraceEngine
    e = TraceEngine(workloads.load('singlet_c1').table)
    yield e
    e.close()


@pytest.mark.parametrize('H,W,S,name,C,edge', BLUR_CASES)
def test_blur_equals_the_restatement(eng, H, W, S, name, C, edge):
    scene, psf, node_y, node_x = blur_inputs(H, W, S, name, C)
    ref = IR.varying_blur(scene, psf, node_y, node_x, IR.EDGE_REPLICATE if edge == 'replicate' else IR.EDGE_ZERO)
    got = eng.varying_blur(scene, psf, node_y, node_x, edge=edge)
    assert got.shape == ref.shape and np.isfinite(got).all()
    bad = np.argwhere(got != ref)
    assert len(bad) == 0, (len(bad), bad[:4], got[tuple(bad[0])], ref[tuple(bad[0])])


def test_blur_host_and_device_arrays_and_two_calls_give_the_same_bits(eng, torch):
    scene, psf, node_y, node_x = blur_inputs(37, 70, 9, '4x5', 3)
    host = eng.varying_blur(scene, psf, node_y, node_x)
    d_scene, d_psf = torch.from_numpy(scene).to(eng.device), torch.from_numpy(psf).to(eng.device)
    dev = eng.varying_blur(d_scene, d_psf, node_y, node_x, on_device=True)
    again = eng.varying_blur(d_scene, d_psf, node_y, node_x, on_device=True)
    mixed = eng.varying_blur(d_scene, psf, node_y, node_x)
    assert dev.is_cuda and dev.shape == (3, 37, 70)
    assert host.tobytes() == dev.cpu().numpy().tobytes() == again.cpu().numpy().tobytes() == mixed.tobytes()
    one = eng.varying_blur(scene[1], psf[1], node_y, node_x)            # without the channel axis
    assert one.shape == (37, 70) and one.tobytes() == host[1].tobytes()
    from rayoptics_amd.engine import EngineError
    with pytest.raises(EngineError, match='S 4 is even'):
        eng.varying_blur(scene, np.zeros((3, 4, 5, 4, 4)), node_y, node_x)
    with pytest.raises(EngineError, match='psf'):
        eng.varying_blur(scene, psf[:2], node_y, node_x)


def test_blur_conserves_light_with_the_zero_edge(eng):
    rng = np.random.default_rng(5)
    scene = np.zeros((40, 90))
    scene[6:34, 6:84] = rng.uniform(0.0, 1.0, (28, 78))
    psf = rng.uniform(0.0, 1.0, (3, 4, 9, 9))
    psf *= 0.6 / psf.sum(axis=(2, 3), keepdims=True)
    out = eng.varying_blur(scene, psf, [2.0, 17.0, 39.0], [0.0, 30.0, 31.0, 89.0])
    assert abs(out.sum() - 0.6 * scene.sum()) < 1e-12 * scene.sum() and out.min() >= 0.0


WARP_SHAPES = [(1, 1, 1), (3, 37, 70), (1, 130, 67)]


@pytest.mark.parametrize('C,H,W', WARP_SHAPES)
def test_warp(eng, torch, C, H, W):
    rng = np.random.default_rng(H)
    img = rng.normal(size=(C, H, W))
    node_y, node_x = (np.asarray(a, dtype=np.float64) for a in grid('4x5', H, W))
    # zero displacement: the input's bits
    same = eng.image_warp(img, node_y, node_x, np.zeros((4, 5, 2)))
    assert same.tobytes() == img.tobytes()
    # an integer displacement: an exact shift, zero where the source lies outside
    disp = np.zeros((4, 5, 2))
    disp[..., 0], disp[..., 1] = 2.0, -3.0
    want = np.zeros_like(img)
    if H > 2 and W > 3:
        want[:, :H - 2, 3:] = img[:, 2:, :W - 3]
    # one node blends nothing (ty = tx = 0): dy = 1*(1*2 + 0*2) + 0 is 2 exactly
    assert np.array_equal(eng.image_warp(img, [5.0], [1.5], disp[:1, :1]), want)
    # between nodes (1 - t)*2 + t*2 may round to the number below 2: the sample then falls one ulp
    # short of the pixel and the blend is the pixel's value to a few roundings -- and the restatement's
    shifted = eng.image_warp(img, node_y, node_x, disp)
    assert np.array_equal(shifted, IR.image_warp(img, node_y, node_x, disp))
    assert np.abs(shifted - want).max() <= 8 * 2.0 ** -53 * np.abs(img).max()
    # a random displacement, host and device arrays
    disp = rng.normal(scale=3.0, size=(4, 5, 2))
    ref = IR.image_warp(img, node_y, node_x, disp)
    got = eng.image_warp(img, node_y, node_x, disp)
    dev = eng.image_warp(torch.from_numpy(img).to(eng.device), node_y, node_x, disp, on_device=True)
    assert np.array_equal(got, ref) and got.tobytes() == dev.cpu().numpy().tobytes()
    one = eng.image_warp(img, [7.0], [2.0], [[[0.5, -0.25]]])          # one node: a uniform sub-pixel shift
    assert np.array_equal(one, IR.image_warp(img, [7.0], [2.0], [[[0.5, -0.25]]]))


@pytest.fixture(scope='module')
def simulated(torch):
    """the double-Gauss TableModel, its three prebuilt fields a 3 x 1 node column, two wavelengths,
    32 x 32 rays, 9 x 9 taps of 10 um on a 48 x 32 scene -- computed once, read by the tests"""
    from rayoptics_amd import analyses
    model = workloads.TableModel('dblgauss_c2')
    wvls = [587.6, 486.1]
    rng = np.random.default_rng(3)
    scene = rng.uniform(0.0, 1.0, (48, 32))
    kw = dict(flds=model.fields, node_px=([4.0, 20.0, 40.0], [15.5]), wvls=wvls, num_rays=32, psf_size=9)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        sim = analyses.image_simulation(model, scene, 0.01, **kw)
        flat = analyses.image_simulation(model, np.ones((48, 32)), 0.01, edge='replicate', **kw)
    return model, wvls, scene, kw, sim, flat, [w for w in caught if 'image_simulation' in str(w.message)]


def test_analysis_psfs_are_the_weighted_maps_normalised(simulated):
    from rayoptics_amd import analyses
    from rayoptics_amd.engine import make_grid
    from rayoptics_amd.trace import _launch_setup
    model, wvls, scene, kw, sim, _flat, caught = simulated
    fs, wis, opts = [], [], []
    for fld in model.fields:
        for wvl in wvls:
            kw_trace = dict(check_apertures=True, apply_vignetting=True)
            e, f, wi, o = _launch_setup(model, fld, wvl, kw_trace, abi.OUT_FULL)
            fs.append(f), wis.append(wi), opts.append(o)
    results = e.trace_pupil_grids(fs, wis, make_grid((-1., -1.), (1., 1.), 32), opts, want_pupil=False)
    assert sim.image_pts.shape == (3, 2, 2)
    # the workload's image points are the chief rays at its reference wavelength, 587.6 nm
    print('chief rays against the workload:', np.abs(sim.image_pts[:, 0] - np.array(model.workload.image_pts)).max())
    assert np.abs(sim.image_pts[:, 0] - np.array(model.workload.image_pts)).max() < 1e-6
    assert np.abs(sim.image_pts[2, 1, 1] - sim.image_pts[2, 0, 1]) > 1e-4          # lateral colour
    window = np.concatenate([sim.image_pts[:, 0], np.full((3, 2), 9 * 0.01 / 2.0)], axis=1)
    # the prebuilt fields' vignetting factors (0, 0.2 and 0.4, above and below) leave this much pupil
    area = [(2.0 - f.vlx - f.vux) / 2.0 * ((2.0 - f.vly - f.vuy) / 2.0) for f in model.fields]
    assert np.allclose(area, [1.0, 0.8, 0.6])
    maps, _cnt, exp, item = e.weighted_maps(results, int(opts[0].flags), item_factor=np.repeat(area, 2),
                                            item_map=[0, 0, 1, 1, 2, 2], n_maps=3, window=window, bins=9)
    q_in = item['q_in'].reshape(3, 2).sum(axis=1)
    q_all = q_in + item['q_out'].reshape(3, 2).sum(axis=1)
    flux = np.ldexp(q_all.astype(np.float64), -exp)
    want = np.ascontiguousarray(maps.transpose(0, 2, 1)) * (1.0 / flux.max())
    psfs = sim.psfs.cpu().numpy()
    assert psfs.shape == (1, 3, 1, 9, 9) and psfs.tobytes() == want.reshape(1, 3, 1, 9, 9).tobytes()
    assert np.array_equal(sim.gain[0], np.ldexp(q_in.astype(np.float64), -exp) / flux.max())
    assert np.array_equal(sim.window_share[0], q_in / q_all)
    print('double Gauss, 10 um pixels, 9 x 9 taps: gain', sim.gain[0], 'window share', sim.window_share[0],
          'warnings', [str(w.message) for w in caught])
    assert (sim.gain <= 1.0).all() and (sim.gain > 0.0).all()
    top = int(np.argmax(flux))
    if sim.window_share[0, top] == 1.0:
        assert sim.gain[0, top] == 1.0
    assert sim.gain[0, 2] < sim.gain[0, 0]                                       # vignetting darkens the corner
    assert all('psf_size' in str(w.message) for w in caught)
    assert (len(caught) > 0) == bool((sim.window_share < 0.99).any())
    assert isinstance(sim, analyses.SimulatedImage) and sim.distortion_px is None and sim.image is sim.blurred


def test_analysis_blur_is_the_restatement_on_its_psfs(simulated):
    _model, _wvls, scene, _kw, sim, _flat, _caught = simulated
    node_y, node_x = sim.node_px
    ref = IR.varying_blur(scene[None], sim.psfs.cpu().numpy(), node_y, node_x)
    assert sim.blurred.shape == (48, 32) and np.array_equal(sim.blurred, ref[0])


def test_analysis_uniform_scene_shows_the_blended_gain(simulated):
    """a uniform scene with the replicate edge: every output is the sum over the taps of the hat
    weight at the tap's SOURCE row times the tap -- the nodes' PSF sums blended; where the weights
    do not change within the PSF's reach (beyond the outermost nodes) that is the node's gain"""
    _model, _wvls, _scene, _kw, _sim, flat, _caught = simulated
    psf = flat.psfs.cpu().numpy()[0, :, 0]                                       # [3, 9, 9]
    wy = IR.hat_weights(48, flat.node_px[0])
    rows = np.clip(np.arange(48)[:, None] - (np.arange(9)[None, :] - 4), 0, 47)  # [i, a]
    want = sum((wy[n][rows] * psf[n].sum(axis=1)[None, :]).sum(axis=1) for n in range(3))
    # at most 162 non-negative terms (two nodes), each product rounded once, summed in another order
    tol = 2 * 162 * 2.0 ** -53 * want
    assert (np.abs(flat.image - want[:, None]) <= tol[:, None]).all()
    assert (np.abs(flat.image[0] - flat.gain[0, 0]) <= tol[0]).all()
    assert (np.abs(flat.image[44:] - flat.gain[0, 2]) <= tol[44:, None]).all()


def test_analysis_with_ideal_points_warps(simulated):
    from rayoptics_amd import analyses
    model, _wvls, scene, kw, sim, _flat, _caught = simulated
    # ideal points 1.5 and -2 pixels from the real ones at the outer nodes
    ideal = sim.image_pts[:, 0] - 0.01 * np.array([[0.0, 0.0], [0.25, 1.5], [-0.5, -2.0]])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        w = analyses.image_simulation(model, scene, 0.01, ideal_pts=ideal, on_device=True, **kw)
        off = analyses.image_simulation(model, scene, 0.01, ideal_pts=ideal, distortion=False, **kw)
    assert w.image.is_cuda and np.array_equal(w.blurred.cpu().numpy(), sim.blurred)
    want_err = ((sim.image_pts[:, 0] - ideal) / 0.01)[:, ::-1].reshape(3, 1, 2)
    assert np.array_equal(w.distortion_px, want_err) and np.abs(want_err[1, 0] - [1.5, 0.25]).max() < 1e-9
    assert np.array_equal(w.displacement, analyses.distortion_displacement(*sim.node_px, want_err))
    ref = IR.image_warp(sim.blurred[None], *sim.node_px, w.displacement)[0]
    assert np.array_equal(w.image.cpu().numpy(), ref) and not np.array_equal(ref, sim.blurred)
    assert off.displacement is None and np.array_equal(off.image, sim.blurred) and off.distortion_px is not None


def test_analysis_channels(simulated):
    """an RGB-like matrix of spectral factors: one PSF stack per channel, a grey scene seen by all"""
    from rayoptics_amd import analyses
    model, _wvls, scene, kw, sim, _flat, _caught = simulated
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        rgb = analyses.image_simulation(model, scene, 0.01, channels=[[1.0, 1.0], [1.0, 0.0], [0.0, 2.0]], **kw)
    assert rgb.image.shape == (3, 48, 32) and rgb.psfs.shape == (3, 3, 1, 9, 9)
    assert np.array_equal(rgb.image[0], sim.image)                               # the factors of the one-channel run
    psfs = rgb.psfs.cpu().numpy()
    # a power-of-two factor scales a map exactly: channel 2 is the blue PSF whatever its factor
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        only_blue = analyses.image_simulation(model, scene, 0.01, channels=[[0.0, 1.0]], **kw)
    assert np.array_equal(psfs[2], only_blue.psfs.cpu().numpy()[0])
    assert not np.array_equal(psfs[1], psfs[2])
    ref = IR.varying_blur(np.broadcast_to(scene, (3, 48, 32)), psfs, *sim.node_px)
    assert np.array_equal(rgb.image, ref)
