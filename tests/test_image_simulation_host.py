"""Image simulation without a GPU: the NumPy restatement of rox_varying_blur (tests/imgsim_ref.py)
against a per-pixel loop that skips what a kernel skips and against scipy's convolution, the hat
weights at their corner cases, the displacement solve of analyses.distortion_displacement on a
known radial distortion, and the argument errors of both C entries, which are reported before a
device is touched."""
import os

import numpy as np
import pytest

import imgsim_ref as IR
from rayoptics_amd import abi, analyses


def random_case(seed, C, H, W, GY, GX, S):
    rng = np.random.default_rng(seed)
    scene = rng.normal(size=(C, H, W))
    psf = rng.uniform(0.0, 1.0, size=(C, GY, GX, S, S))
    node_y = np.sort(rng.uniform(-3.0, H + 2.0, GY))
    node_x = np.sort(rng.uniform(-3.0, W + 2.0, GX))
    return scene, psf, node_y, node_x


def test_the_exports_and_the_header():
    from rayoptics_amd.engine import load_library
    lib = load_library()
    for name in ('rox_varying_blur', 'rox_image_warp'):
        assert hasattr(lib, name) and name in abi.EXPORTS
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, 'include', 'roxtrace.h')).read()
    assert 'int rox_varying_blur(int32_t C, int32_t H, int32_t W, const double *scene,' in src
    assert 'int rox_image_warp(int32_t C, int32_t H, int32_t W, const double *in,' in src
    assert '#define ROX_BLUR_EDGE_REPLICATE 1u' in src and abi.BLUR_EDGE_REPLICATE == 1 and abi.ABI_VERSION == 8


@pytest.mark.parametrize('edge', [IR.EDGE_ZERO, IR.EDGE_REPLICATE])
def test_vectorised_restatement_equals_the_per_pixel_loop(edge):
    """13 x 17, 3 x 2 nodes, S = 5: one product and one sum per node and tap over whole pictures
    against the loop that skips zero-weight terms and outside sources -- equal under =="""
    scene, psf, node_y, node_x = random_case(7, 2, 13, 17, 3, 2, 5)
    node_y[0], node_x[1] = 4.0, 20.5                     # a node on a pixel, one outside the picture
    a = IR.varying_blur(scene, psf, node_y, node_x, edge)
    b = IR.varying_blur_loop(scene, psf, node_y, node_x, edge)
    assert np.array_equal(a, b)
    assert np.abs(a).max() > 1.0


def test_one_node_is_scipy_convolve2d():
    from scipy.signal import convolve2d
    scene, psf, node_y, node_x = random_case(11, 1, 19, 14, 1, 1, 7)
    got = IR.varying_blur(scene, psf, node_y, node_x)[0]
    ref = convolve2d(scene[0], psf[0, 0, 0], mode='same')
    # scipy sums the same 49 products in another order: |sum of products| <= 49 * max|scene| * 1, each
    # sum rounding by at most 2^-53 of the running magnitude
    assert np.abs(got - ref).max() <= 49 * 49 * np.abs(scene).max() * 2.0 ** -53
    print('one node against scipy.signal.convolve2d: max difference', np.abs(got - ref).max())


def test_a_single_tap_of_one_returns_the_scene():
    scene, _psf, node_y, node_x = random_case(13, 3, 9, 11, 2, 3, 1)
    out = IR.varying_blur(scene, np.ones((3, 2, 3, 1, 1)), node_y, node_x)
    # the hat weights of a pixel sum to 1 in two terms (1 - t) + t; each term is scene * w, rounded
    assert np.abs(out - scene).max() <= 4 * 2.0 ** -53 * np.abs(scene).max()
    on = IR.varying_blur(scene, np.ones((3, 1, 1, 1, 1)), [4.0], [5.0])
    assert np.array_equal(on, scene)


def test_light_is_conserved_with_the_zero_edge():
    """every node sums to g: the picture holds g times the scene's light, all of it where the
    scene's light lies S // 2 or more from the frame"""
    rng = np.random.default_rng(17)
    S, g = 5, 0.75
    scene = np.zeros((1, 16, 18))
    scene[0, 2:14, 2:16] = rng.uniform(0.0, 1.0, (12, 14))
    psf = rng.uniform(0.0, 1.0, (1, 3, 3, S, S))
    psf *= g / psf.sum(axis=(3, 4), keepdims=True)
    out = IR.varying_blur(scene, psf, [1.0, 7.5, 20.0], [-2.0, 8.0, 15.0])
    assert abs(out.sum() - g * scene.sum()) < 1e-12 * scene.sum()


def test_hat_weights():
    node = np.array([-2.5, 3.0, 4.5, 9.25])
    w = IR.hat_weights(8, node)
    assert w.shape == (4, 8) and np.abs(w.sum(axis=0) - 1.0).max() <= 2.0 ** -52 and (w >= 0.0).all()
    assert w[1, 3] == 1.0 and w[0, 3] == 0.0 and w[2, 3] == 0.0          # a node on a pixel
    assert w[0, 0] == 1.0 - 2.5 / 5.5 and w[1, 0] == 2.5 / 5.5           # the first node outside the picture
    assert w[1, 4] == 1.0 - 1.0 / 1.5 and w[2, 4] == 1.0 / 1.5 and w[3, 4] == 0.0
    assert (w[3, :5] == 0.0).all() and w[3, 7] == (7.0 - 4.5) / (9.25 - 4.5) and w[2, 7] == 1.0 - w[3, 7]
    # all pixels before the first node / behind the last one
    assert np.array_equal(IR.hat_weights(5, [7.0, 9.0]), [[1.0] * 5, [0.0] * 5])
    assert np.array_equal(IR.hat_weights(5, [-4.0, -1.0]), [[0.0] * 5, [1.0] * 5])
    assert np.array_equal(IR.hat_weights(5, [2.0]), [[1.0] * 5])          # GY = 1, wherever the node lies
    k, t = IR.hat_cells([-1.0, 3.0, 4.0, 9.25, 11.0], node)
    assert k.tolist() == [0, 1, 1, 3, 3] and t[1] == 0.0 and t[3] == 0.0 and t[4] == 0.0
    k2, t2 = analyses.hat_cells([-1.0, 3.0, 4.0, 9.25, 11.0], node)
    assert np.array_equal(k, k2) and np.array_equal(t, t2)


def test_displacement_solve_inverts_a_radial_distortion():
    """5 x 5 nodes.  A magnification error e(q) = m (q - c) is linear, so its hat blend is exact
    and the inverse is known in closed form: D = -m/(1 + m) (p - c).  A third-order distortion
    e(q) = kappa |q - c|^2 (q - c): the solve satisfies D + e(p + D) = 0 on the blend.  Both to
    1e-9 px after the eight steps."""
    node_y, node_x = np.linspace(0.0, 400.0, 5), np.linspace(0.0, 600.0, 5)
    c = np.array([200.0, 300.0])
    p = np.stack(np.meshgrid(node_y, node_x, indexing='ij'), axis=-1)
    m = 0.02
    d = analyses.distortion_displacement(node_y, node_x, m * (p - c))
    assert np.abs(d - (-m / (1.0 + m)) * (p - c)).max() < 1e-9
    # 1.3 % at the corner, 3.9 px; the blend's steepest cell has a slope L of 3.4 %, and a step
    # shrinks the error by L: 3.9 * L^8 = 7e-12
    kappa = 1e-7
    rel = p - c
    err = kappa * (rel ** 2).sum(axis=-1, keepdims=True) * rel
    assert 3.5 < np.abs(err).max() < 4.0 and np.abs(np.diff(err[..., 0], axis=0)).max() / 100.0 < 0.035
    d = analyses.distortion_displacement(node_y, node_x, err)
    q = p + d
    resid = d + analyses.hat_interp(err, node_y, node_x, q[..., 0], q[..., 1])
    assert np.abs(resid).max() < 1e-9
    assert np.abs(d).max() > 3.0 and (d[2, 2] == 0.0).all()


def call_blur(lib, C=1, H=8, W=9, S=3, GY=2, GX=2, node_y=(0.0, 5.0), node_x=(1.0, 6.0), scene=None, out=None,
              psf=None, flags=0):
    scene = np.zeros((C or 1, H, W)) if scene is None else scene
    out = np.zeros((C or 1, H, W)) if out is None else out
    psf = np.zeros(max(1, (C or 1) * GY * GX * S * S)) if psf is None else psf
    ny, nx = np.asarray(node_y, dtype=np.float64), np.asarray(node_x, dtype=np.float64)
    rc = lib.rox_varying_blur(C, H, W, scene.ctypes.data, S, GY, GX, psf.ctypes.data, ny.ctypes.data, nx.ctypes.data,
                              out.ctypes.data, flags, None)
    return rc, lib.rox_last_error().decode()


def call_warp(lib, C=1, H=8, W=9, GY=2, GX=2, node_y=(0.0, 5.0), node_x=(1.0, 6.0), img=None, out=None, disp=None):
    img = np.zeros((C or 1, H, W)) if img is None else img
    out = np.zeros((C or 1, H, W)) if out is None else out
    disp = np.zeros((GY, GX, 2)) if disp is None else disp
    ny, nx = np.asarray(node_y, dtype=np.float64), np.asarray(node_x, dtype=np.float64)
    rc = lib.rox_image_warp(C, H, W, img.ctypes.data, GY, GX, ny.ctypes.data, nx.ctypes.data, disp.ctypes.data,
                            out.ctypes.data, None)
    return rc, lib.rox_last_error().decode()


def test_both_entries_reject_bad_arguments_without_a_device():
    from rayoptics_amd.engine import load_library
    lib = load_library()
    buf = np.zeros(2 * 8 * 9)
    overlap = dict(scene=buf[:72].reshape(1, 8, 9), out=buf[40:112].reshape(1, 8, 9))
    for kw, word in [(dict(S=4), 'S 4 is even'), (dict(S=67), 'S 67 outside'), (dict(S=0), 'S 0 outside'),
                     (dict(node_y=(5.0, 5.0)), 'node_y[1]'), (dict(node_x=(6.0, 1.0)), 'node_x[1]'),
                     (dict(node_x=(np.nan, 1.0)), 'node_x[0]'), (dict(C=0), 'C 0 outside'), (dict(C=17), 'C 17'),
                     (dict(H=0), 'H 0'), (dict(W=16385), 'W 16385'), (dict(GY=0, node_y=()), 'GY 0'),
                     (dict(GY=40, GX=40, node_y=np.arange(40.0), node_x=np.arange(40.0)), 'GY*GX'),
                     (overlap, 'out overlaps scene'), (dict(flags=2), 'flags')]:
        rc, msg = call_blur(lib, **kw)
        assert rc == -1 and msg.startswith('rox_varying_blur: ') and word in msg, (kw, rc, msg)
    overlap = dict(img=buf[:72].reshape(1, 8, 9), out=buf[71:143].reshape(1, 8, 9))
    bad_disp = np.zeros((2, 2, 2))
    bad_disp[1, 0, 1] = np.inf
    for kw, word in [(dict(node_y=(5.0, 4.0)), 'node_y[1]'), (dict(C=0), 'C 0 outside'), (dict(H=16385), 'H 16385'),
                     (dict(GX=0, node_x=()), 'GX 0'), (overlap, 'out overlaps in'), (dict(disp=bad_disp), 'disp[5]')]:
        rc, msg = call_warp(lib, **kw)
        assert rc == -1 and msg.startswith('rox_image_warp: ') and word in msg, (kw, rc, msg)


def test_simulation_flux_adds_a_nodes_items():
    from rayoptics_amd.engine import WMAP_ITEM_DTYPE
    item = np.zeros(4, WMAP_ITEM_DTYPE)
    item['q_in'], item['q_out'] = [8, 24, 0, 16], [0, 32, 0, 16]
    fin, fall = analyses.simulation_flux(item, np.array([3, 4]), 2)
    assert fin.tolist() == [4.0, 1.0] and fall.tolist() == [8.0, 2.0]


# ---- node placement on the live reference's double Gauss (oracle-backed engine) ------------------
@pytest.mark.needs_reference
def test_nodes_on_the_reference_double_gauss():
    """3 x 5 nodes over a 36 x 24 mm frame of 25 um pixels: the node fields' real chief rays land
    on the ideal grid to the lens's distortion (under 2 %), mirrored in x and y, the centre node on
    the axis; the slope of the ideal map is the focal length of this object-at-infinity lens"""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), 'golden'))
    import refmodels as rm
    from oracle_engine import OracleEngine
    from rayoptics_amd import session
    session._set_engine_factory(OracleEngine)
    try:
        opm = rm.dblgauss()
        H, W, pitch = 960, 1440, 0.025
        flds, node_y, node_x, ideal = analyses._simulation_nodes(opm, (3, 5), H, W, pitch, 'test')
        assert len(flds) == 15 and node_y.tolist() == [0.0, 479.5, 959.0] and node_x[0] == 0.0 and node_x[-1] == 1439.0
        assert np.array_equal(ideal[7], [0.0, 0.0]) and flds[7].x == 0.0 and flds[7].y == 0.0
        assert np.allclose(ideal[0], [-719.5 * pitch, -479.5 * pitch]) and np.allclose(ideal[14], -ideal[0])
        assert all(f.vuy == f.vly == f.vux == f.vlx == 0.0 and f.aim_info is not None for f in flds)
        wvl = opm['osp']['wvls'].central_wvl
        real = analyses._chief_ray_image_pts(opm, flds, [wvl], 'test')[:, 0]
        err = real - ideal
        r = np.hypot(ideal[:, 0], ideal[:, 1])
        print('distortion at the nodes (fraction of the image height):',
              np.array2string(np.hypot(err[:, 0], err[:, 1])[r > 0] / r[r > 0], precision=4))
        assert np.abs(real[7]).max() < 1e-9
        assert (np.hypot(err[:, 0], err[:, 1]) <= 0.02 * r + 1e-9).all()
        assert np.abs(real[::-1] + real).max() < 1e-6                    # point symmetry of the grid
        # node 12 is straight below the centre: image height over the tangent of its field angle
        # is the focal length to the distortion (the fields are relative to 14 degrees)
        efl = opm['analysis_results']['parax_data'].fod.efl
        assert flds[12].x == 0.0 and abs(abs(real[12, 1] / np.tan(np.deg2rad(flds[12].y * 14.0))) / efl - 1.0) < 0.02
    finally:
        session._set_engine_factory(None)
