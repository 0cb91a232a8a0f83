"""rox_huygens_psf on the device against its NumPy restatement (tests/huygens_ref.py): synthetic
rows whose arguments reach 2^10 cycles, with failed rays and amplitudes, in shapes of one tile
and of several (70 x 66 pixels cross the 64-row tiles, 289 rays the 16-ray reduction block), whole
and split by a capped scratch; the closed forms; bits that do not depend on the call, the
destination of the statistics or the split; a defocused plane against a pre-shifted phase; an item
without rays.  Then analyses.huygens_psf and image_simulation(psf='huygens') on the double Gauss
of tests/golden/through_focus_map.npz.

The bound per component of U is (2 R + 32) 2^-53 sum |a_r|: the any-order bound of a sum of 2 R
products, plus the operands' rounding (two roundings of a correctly rounded sine or cosine times
a_r) and a few ulp of sincospi.  psf is held to twice that, relative to sum |a_r|^2."""
import numpy as np
import pytest

import huygens_ref as HR
from packets_fixture import torch  # noqa: F401 (the fixture)
from rayoptics_amd import abi, workloads
from test_huygens_host import lattice_case, synthetic

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53


@pytest.fixture(scope='module')
def eng(torch):
    from rayoptics_amd.engine import TraceEngine
    e = TraceEngine(workloads.load('singlet_c1').table)
    yield e
    e.close()


def on_device(eng, rows, amp, status):
    t = eng.torch
    d = lambda a: None if a is None else t.from_numpy(np.ascontiguousarray(a)).to(eng.device)  # noqa: E731
    return d(rows), d(amp), d(status)


GIVEN = object()


def run(eng, case, amp=GIVEN, **kw):
    rows, a, status, planes, px, py, nx, ny, R = case
    d_rows, d_amp, d_status = on_device(eng, rows, a if amp is GIVEN else amp, status)
    psf, field, stats = eng.huygens_psf(d_rows, d_status, planes, nx, ny, px, py, n_rays=R, amp=d_amp,
                                        want_field=True, **kw)
    return psf.cpu().numpy(), field.cpu().numpy(), stats


def make_case(seed, n_items, K, R, nx, ny):
    rows, amp, status, planes, px, py = synthetic(np.random.default_rng(seed), n_items, K, R, nx, ny)
    return rows, amp, status, planes, px, py, nx, ny, R


@pytest.fixture(scope='module')
def cases():
    """the two shapes of the issue and one of two ray slices, each with its restatement, computed once"""
    out = {}
    # 'slices': more than the 8192 rays of one GEMM problem (csrc/huygens.hip kSliceRays)
    for name, shape in (('small', (2, 3, 49, 5, 3)), ('tiles', (2, 3, 289, 70, 66)), ('slices', (1, 2, 8200, 5, 3))):
        case = make_case(len(name), *shape)
        rows, amp, status, planes, px, py, nx, ny, R = case
        out[name] = (case, HR.huygens_psf(rows, amp, status, planes, nx, ny, px, py, n_rays=R))
    return out


def check_against(case, ref, psf, field, stats):
    _rows, _amp, _status, planes, _px, _py, nx, ny, R = case
    U, ref_psf, st = ref
    n_items, K = planes.shape[:2]
    assert psf.shape == (n_items, K, nx, ny) and field.shape == (n_items, K, nx, ny, 2)
    for i in range(n_items):
        tol = (2 * R + 32) * U53 * st['sum_abs'][i]
        err = max(np.abs(field[i, ..., 0] - U[i].real).max(), np.abs(field[i, ..., 1] - U[i].imag).max())
        sq = HR.operands(*[a[i] for a in case[:3]], planes[i], nx, ny, case[4], case[5], R)[2]
        tol_psf = 2 * (2 * R + 32) * U53 * (sq ** 2).sum()
        err_psf = np.abs(psf[i] - ref_psf[i]).max()
        print(f'item {i}: |dU| {err:.3g} (bound {tol:.3g}), |dpsf| {err_psf:.3g} (bound {tol_psf:.3g})')
        assert err <= tol and err_psf <= tol_psf
        # psf is re^2 + im^2 of the field the call wrote, unfused
        assert np.array_equal(psf[i], field[i, ..., 0] * field[i, ..., 0] + field[i, ..., 1] * field[i, ..., 1])
    assert np.array_equal(stats['n'], st['n'])
    assert np.abs(stats['norm'] - st['norm']).max() <= 4 * R * U53 * st['norm'].max()
    assert np.abs(stats['sum'] - psf.sum(axis=(2, 3))).max() <= 4 * nx * ny * U53 * stats['sum'].max()
    assert np.array_equal(stats['peak'], psf.max(axis=(2, 3)))
    at = psf.reshape(n_items, K, -1).argmax(axis=2)
    assert np.array_equal(stats['peak_ix'], at // ny) and np.array_equal(stats['peak_iy'], at % ny)
    for i in range(n_items):
        for k in range(K):
            a0 = HR.origin_pixel(planes[i, k, 0], case[4], nx)
            b0 = HR.origin_pixel(planes[i, k, 1], case[5], ny)
            assert stats['strehl'][i, k] == psf[i, k, a0, b0] / stats['norm'][i, k]


@pytest.mark.parametrize('name', ['small', 'tiles', 'slices'])
def test_device_equals_the_restatement(eng, cases, name):
    case, ref = cases[name]
    check_against(case, ref, *run(eng, case))


# the 'tiles' shape takes 757 760 bytes of scratch per plane and 622 592 per item: 2.9 MB an item
@pytest.mark.parametrize('cap', [3000000, 1500000], ids=['items', 'planes'])
def test_a_capped_scratch_splits_the_job_with_the_same_bits(eng, cases, monkeypatch, cap):
    case, ref = cases['tiles']
    whole = run(eng, case)
    monkeypatch.setenv('ROX_HUYGENS_SCRATCH_BYTES', str(cap))
    split = run(eng, case)
    monkeypatch.delenv('ROX_HUYGENS_SCRATCH_BYTES')
    check_against(case, ref, *split)
    assert whole[0].tobytes() == split[0].tobytes() and whole[1].tobytes() == split[1].tobytes()
    assert whole[2].tobytes() == split[2].tobytes()


def test_both_tile_shapes_give_the_same_bits(eng, monkeypatch):
    """2 items x 4 planes of 512 x 512 pixels are 512 workgroup tiles of 64 x 64: the whole job
    takes the 64 x 64 instance of the GEMM.  Capped at 18 MB (an item is 17.4 MB) a launch holds one
    item, 256 tiles, and takes the 32 x 32 instance.  The bits are the same."""
    case = make_case(21, 2, 4, 16, 512, 512)
    whole = run(eng, case)
    monkeypatch.setenv('ROX_HUYGENS_SCRATCH_BYTES', '18000000')
    split = run(eng, case)
    monkeypatch.delenv('ROX_HUYGENS_SCRATCH_BYTES')
    assert all(x.tobytes() == y.tobytes() for x, y in zip(whole, split)) and (whole[0] > 0.0).any()


def test_identical_calls_host_and_device_stats_and_null_amplitudes(eng, cases):
    from rayoptics_amd.engine import HUYGENS_STATS_DTYPE, records_view
    case, _ref = cases['tiles']
    a, b = run(eng, case), run(eng, case)
    dev = run(eng, case, stats_on_device=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert records_view(dev[2], HUYGENS_STATS_DTYPE).tobytes() == a[2].tobytes() and a[0].tobytes() == dev[0].tobytes()
    # amp NULL is amp of ones, bit for bit
    ones = np.ones_like(case[1])
    none, one = run(eng, case, amp=None), run(eng, case, amp=ones)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(none, one))
    assert none[0].tobytes() != a[0].tobytes()
    # stats alone, psf alone
    rows, amp, status, planes, px, py, nx, ny, R = case
    d_rows, d_amp, d_status = on_device(eng, rows, amp, status)
    _p, _f, only = eng.huygens_psf(d_rows, d_status, planes, nx, ny, px, py, n_rays=R, amp=d_amp, want_psf=False)
    assert _p is None and _f is None and only.tobytes() == a[2].tobytes()


def test_closed_forms_on_the_device(eng):
    rows, planes, nx, ny, px, py, want = lattice_case()
    n2 = rows.shape[2]
    psf, _field, stats = run(eng, (rows, None, np.zeros((1, n2), np.uint8), planes, px, py, nx, ny, n2), amp=None)
    assert np.abs(psf[0, 0] - want).max() <= 1e-11 * n2 ** 2
    assert stats['peak_ix'][0, 0] == nx // 2 and stats['peak_iy'][0, 0] == ny // 2
    assert abs(stats['strehl'][0, 0] - 1.0) < 1e-12 and stats['norm'][0, 0] == n2 ** 2 and stats['n'][0, 0] == n2
    # one ray: a^2 at every pixel of every plane
    one = np.array([[0.3], [17.25], [-4.5], [1700.0]]).reshape(1, 4, 1)
    pl = np.array([[[-0.01, 0.02, 0.0], [0.003, 0.0, -0.05]]])
    psf, _f, stats = run(eng, (one, np.array([[1.75]]), np.zeros((1, 1), np.uint8), pl, 0.0013, 0.0021, 7, 5, 1))
    assert np.abs(psf - 1.75 ** 2).max() <= 8 * U53 * 1.75 ** 2 and (stats['n'] == 1).all()
    assert np.array_equal(stats['norm'], np.full((1, 2), 1.75 ** 2))


def test_a_defocused_plane_is_the_pre_shifted_phase(eng, cases):
    case, _ref = cases['tiles']
    rows, amp, status, planes, px, py, nx, ny, R = case
    whole = run(eng, case)
    k = 2
    assert (planes[:, k, 2] != 0.0).all()
    shifted = rows.copy()
    for i in range(rows.shape[0]):
        shifted[i, 0] = rows[i, 0] + rows[i, 3] * planes[i, k, 2]          # fl(phi + fl(zeta dz))
    flat = planes[:, k:k + 1].copy()
    flat[:, :, 2] = 0.0
    one = run(eng, (shifted, amp, status, flat, px, py, nx, ny, R))
    assert one[0][:, 0].tobytes() == whole[0][:, k].tobytes() and one[1][:, 0].tobytes() == whole[1][:, k].tobytes()
    assert one[2][:, 0].tobytes() == whole[2][:, k].tobytes()


def test_an_item_without_rays(eng):
    case = list(make_case(9, 2, 2, 49, 5, 3))
    case[2] = case[2].copy()
    case[2][1, :] = abi.BLOCKED
    psf, field, stats = run(eng, tuple(case))
    assert (stats['n'][1] == 0).all() and (stats['n'][0] > 0).all()
    for name in ('norm', 'sum', 'peak', 'strehl'):
        assert np.isnan(stats[name][1]).all() and np.isfinite(stats[name][0]).all()
    assert (stats['peak_ix'][1] == -1).all() and (stats['peak_iy'][1] == -1).all()
    assert (psf[1] == 0.0).all() and (field[1] == 0.0).all() and (psf[0] > 0.0).any()


def test_wrapper_errors(eng):
    from rayoptics_amd.engine import EngineError
    rows, amp, status, planes, px, py, nx, ny, R = make_case(1, 1, 1, 8, 4, 4)
    d_rows, d_amp, d_status = on_device(eng, rows, amp, status)
    with pytest.raises(EngineError, match='pitch_x'):
        eng.huygens_psf(d_rows, d_status, planes, nx, ny, 0.0, py)
    with pytest.raises(EngineError, match='n_rays'):
        eng.huygens_psf(d_rows, d_status, planes, nx, ny, px, py, n_rays=rows.shape[2] + 1)
    with pytest.raises(EngineError, match='rows'):
        eng.huygens_psf(rows, d_status, planes, nx, ny, px, py)
    with pytest.raises(EngineError, match='planes'):
        eng.huygens_psf(d_rows, d_status, planes[0], nx, ny, px, py)


# ---- end to end ----------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def dblgauss(torch):
    import focus_map_fixture as fm
    model = fm.FocusMapFixtureModel(fm.load(), 'dblgauss')
    return model, model.focs[7]                     # a focus the fixture has a reference sphere for


def test_analysis_on_the_double_gauss(dblgauss):
    """2 fields x 3 wavelengths, 16 x 16 rays, 24 x 24 pixels of 2 um, two planes"""
    from rayoptics_amd import analyses
    model, foc = dblgauss
    flds, wvls = [model.fields[0], model.fields[2]], model.wvls
    focs = [foc, foc + 0.05]
    kw = dict(flds=flds, wvls=wvls, num_rays=16, ref_foc=foc)
    h = analyses.huygens_psf(model, 0.002, size=24, focs=focs, **kw)
    assert isinstance(h, analyses.HuygensPSF) and h.psf.shape == (2, 3, 2, 24, 24) and h.poly.shape == (2, 2, 24, 24)
    hr = analyses.trace_huygens_rows(model, **kw)
    assert hr.n_rays == 256 and hr.ref == 0
    planes = analyses.huygens_planes(hr.centres, h.origins, focs, 3)
    rows, status = hr.rows.cpu().numpy(), hr.status.cpu().numpy()
    _U, ref, st = HR.huygens_psf(rows, None, status, planes, 24, 24, 0.002, 0.002, n_rays=256)
    tol = 2 * (2 * 256 + 32) * U53 * st['n'].reshape(2, 3, 2).max()
    print('analysis against the restatement:', np.abs(h.psf.reshape(6, 2, 24, 24) - ref).max(), 'bound', tol)
    assert np.abs(h.psf.reshape(6, 2, 24, 24) - ref).max() <= tol
    assert np.array_equal(h.n, st['n'][:, 0].reshape(2, 3)) and (h.n > 100).all()
    # the window: pixel 12 lies on the chief ray of the first wavelength given
    assert np.allclose(h.origins + 12 * 0.002, h.centres[:, 0, :2], atol=1e-15)
    assert np.array_equal(h.peak_px.shape, (2, 3, 2, 2)) and (h.strehl > 0).all() and (h.strehl <= 1.0 + 1e-12).all()
    # lateral colour off axis: the centres differ by wavelength, the window does not
    assert abs(h.centres[1, 2, 1] - h.centres[1, 0, 1]) > 1e-4
    # the polychromatic PSF is the plain weighted sum of the normalised PSFs
    wts = np.ones(3)                                                   # no osp: every spectral weight is 1
    want = sum(wts[w] * h.psf[:, w] / h.norm[:, w, :, None, None] for w in range(3))
    assert np.abs(h.poly - want).max() <= 8 * U53 * want.max()
    assert h.border_share.shape == (2, 3, 2) and (h.border_share >= 0).all() and (h.border_share < 1).all()
    assert h.best_focus.shape == (2,) and h.poly_strehl.shape == (2, 2)
    dev = analyses.huygens_psf(model, 0.002, size=24, focs=focs, on_device=True, **kw)
    assert dev.psf.is_cuda and dev.psf.cpu().numpy().tobytes() == h.psf.tobytes()


def test_image_simulation_with_huygens_psfs(dblgauss):
    import warnings
    import imgsim_ref as IR
    from rayoptics_amd import analyses
    model, foc = dblgauss
    rng = np.random.default_rng(4)
    scene = np.zeros((32, 32))
    scene[8:24, 8:24] = rng.uniform(0.0, 1.0, (16, 16))
    kw = dict(flds=model.fields, node_px=([4.0, 16.0, 28.0], [15.5]), wvls=model.wvls, num_rays=32, psf_size=9)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        geo = analyses.image_simulation(model, scene, 0.01, **kw)
        geo2 = analyses.image_simulation(model, scene, 0.01, psf='geometric', **kw)
        hu = analyses.image_simulation(model, scene, 0.01, psf='huygens', psf_oversample=3, psf_ref_foc=foc, **kw)
    assert np.array_equal(geo.image, geo2.image) and geo.psfs.cpu().numpy().tobytes() == geo2.psfs.cpu().numpy().tobytes()
    psfs = hu.psfs.cpu().numpy()
    assert psfs.shape == (1, 3, 1, 9, 9) and (psfs >= 0.0).all()
    # a node's PSF sums to its relative transmission: the usable flux over the brightest node's
    assert np.abs(psfs.sum(axis=(3, 4))[:, :, 0] - hu.gain).max() <= 200 * U53
    assert hu.gain.max() == 1.0 and (hu.gain > 0.0).all() and hu.gain[0, 2] < hu.gain[0, 0]
    # the same usable flux as the geometric stack counts, inside its window or not
    assert np.abs(hu.gain - geo.gain / geo.window_share).max() < 1e-9
    assert np.array_equal(hu.blurred, IR.varying_blur(scene[None], psfs, *hu.node_px)[0])
    # light: the scene's support lies 8 pixels from the frame, the taps reach 4 -- nothing leaves
    wy = IR.hat_weights(32, hu.node_px[0])
    want = sum((wy[n][:, None] * scene).sum() * hu.gain[0, n] for n in range(3))
    assert abs(hu.image.sum() - want) <= 1e-12 * want
    assert not np.array_equal(hu.image, geo.image) and np.abs(hu.image - geo.image).max() > 1e-3
    with pytest.raises(ValueError, match='psf is'):
        analyses.image_simulation(model, scene, 0.01, psf='fft', **kw)
