"""rox_focus_psf on the device: each plane's PSF is bit-identical to rox_calc_psf of that plane's
OPD grid, the Strehl ratio matches NumPy and is reproducible, argument errors are refused before
anything is enqueued, and analyses.through_focus_psf agrees with through_focus + calc_psf."""
import ctypes as C

import numpy as np
import pytest

from rayoptics_amd import abi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch


@pytest.fixture(scope='module')
def lib(torch):
    from rayoptics_amd.engine import load_library
    return load_library()


def synthetic_rows(torch, n_items, K, ndim, seed, zero_opd=False, fail_frac=0.1):
    """device rows [n_items][K][3][ld] and status [n_items][ld] in the through-focus layouts"""
    from rayoptics_amd.engine import padded_ld
    rng = np.random.default_rng(seed)
    R = ndim * ndim
    ld = padded_ld(R)
    rows = np.full((n_items, K, 3, ld), np.nan)
    rows[:, :, :2, :R] = rng.normal(size=(n_items, K, 2, R))
    rows[:, :, 2, :R] = 0.0 if zero_opd else rng.normal(scale=1e-4, size=(n_items, K, R))
    status = np.zeros((n_items, ld), dtype=np.uint8)
    status[:, :R] = np.where(rng.random((n_items, R)) < fail_frac, abi.BLOCKED, abi.OK)
    scale = 1.0 / (rng.uniform(4e-4, 7e-4, size=n_items))           # 1 / wavelength in mm
    return (torch.from_numpy(rows).cuda(), torch.from_numpy(status).cuda(), scale, rows, status)


def host_opd(rows, status, scale, i, k, ndim):
    R = ndim * ndim
    return np.where(status[i, :R] == abi.OK, scale[i] * rows[i, k, 2, :R], np.nan).reshape(ndim, ndim)


def call(lib, torch, d_rows, d_status, scale, ndim, maxdim, want_psf=True, dev_stats=False):
    n_items, K, _, ld = d_rows.shape
    psf = torch.empty((n_items, K, maxdim, maxdim), dtype=torch.float64, device='cuda') if want_psf else None
    if dev_stats:
        dst = torch.empty((n_items, K, 4), dtype=torch.float64, device='cuda')
        ptr = dst.data_ptr()
    else:
        from rayoptics_amd.engine import FOCUS_PSF_STATS_DTYPE
        dst = np.empty((n_items, K), dtype=FOCUS_PSF_STATS_DTYPE)
        ptr = dst.ctypes.data
    sc = np.ascontiguousarray(scale, dtype=np.float64)
    rc = lib.rox_focus_psf(n_items, K, d_rows.data_ptr(), ld, d_status.data_ptr(), sc.ctypes.data, ndim, maxdim,
                           psf.data_ptr() if psf is not None else None, ptr,
                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.rox_last_error()
    torch.cuda.synchronize()
    if dev_stats:
        from rayoptics_amd.engine import FOCUS_PSF_STATS_DTYPE
        dst = dst.cpu().numpy().view(FOCUS_PSF_STATS_DTYPE).reshape(n_items, K)
    return psf, dst


def numpy_strehl(opd):
    ok = ~np.isnan(opd)
    n = int(ok.sum())
    if n == 0:
        return n, float('nan')
    ph = np.exp(1j * 2 * np.pi * opd[ok])
    return n, float(abs(ph.sum()) ** 2 / n ** 2)


def check_against_single_calls(torch, lib, n_items, K, ndim, maxdim, seed, planes=None):
    from rayoptics_amd.engine import calc_psf
    d_rows, d_status, scale, rows, status = synthetic_rows(torch, n_items, K, ndim, seed)
    psf, stats = call(lib, torch, d_rows, d_status, scale, ndim, maxdim)
    todo = planes if planes is not None else [(i, k) for i in range(n_items) for k in range(K)]
    for i, k in todo:
        opd = host_opd(rows, status, scale, i, k, ndim)
        one = calc_psf(torch.from_numpy(opd).cuda(), ndim, maxdim)
        assert torch.equal(psf[i, k], one), (ndim, maxdim, i, k)
        n, s = numpy_strehl(opd)
        assert stats[i, k]['n'] == n
        assert abs(stats[i, k]['strehl'] - s) <= 1e-12, (i, k)
    return psf, stats, (d_rows, d_status, scale, rows, status)


@pytest.mark.parametrize('ndim,maxdim,K', [(8, 20, 1), (8, 20, 7), (8, 20, 21), (8, 20, 256), (32, 128, 7),
                                           (32, 128, 21), (64, 256, 7), (128, 512, 3), (128, 1000, 2)])
def test_planes_equal_single_calls(torch, lib, ndim, maxdim, K):
    check_against_single_calls(torch, lib, 1, K, ndim, maxdim, seed=ndim + K)


def test_items_with_their_own_wave_scale(torch, lib):
    check_against_single_calls(torch, lib, 3, 5, 32, 128, seed=11)


def test_split_into_several_launches(torch, lib):
    """(128, 512) takes 1.3 MB of scratch per plane: 256 planes run as two launches; without a
    PSF destination (its scratch counted too) as four -- the same statistics either way"""
    K = 256
    planes = [(0, k) for k in (0, 1, 100, 203, 204, 205, 255)]
    psf, stats, (d_rows, d_status, scale, _r, _s) = check_against_single_calls(torch, lib, 1, K, 128, 512, seed=5,
                                                                               planes=planes)
    _none, stats2 = call(lib, torch, d_rows, d_status, scale, 128, 512, want_psf=False)
    assert stats.tobytes() == stats2.tobytes()
    # each plane's normalised centre times its maximum is |sum phase|^2 (no OPD entry is 0)
    M = 512
    centre = psf[0, :, M // 2, M // 2].cpu().numpy()
    np.testing.assert_allclose(centre * stats['psf_peak'][0], stats['strehl'][0] * stats['n'][0] ** 2, rtol=1e-12)


def test_strehl_of_a_perfect_wavefront_is_one(torch, lib):
    d_rows, d_status, scale, _rows, status = synthetic_rows(torch, 2, 3, 32, seed=3, zero_opd=True)
    _psf, stats = call(lib, torch, d_rows, d_status, scale, 32, 64, want_psf=False)
    assert (stats['strehl'] == 1.0).all()
    assert (stats['n'] == (status[:, :32 * 32] == abi.OK).sum(axis=1)[:, None]).all()


def test_no_ray_gives_nan(torch, lib):
    d_rows, d_status, scale, _rows, _status = synthetic_rows(torch, 1, 2, 8, seed=4, fail_frac=2.0)
    _psf, stats = call(lib, torch, d_rows, d_status, scale, 8, 20, want_psf=False)
    assert (stats['n'] == 0).all() and np.isnan(stats['strehl']).all()


def test_stats_are_reproducible_host_or_device(torch, lib):
    d_rows, d_status, scale, _rows, _status = synthetic_rows(torch, 2, 21, 64, seed=9)
    _p1, s1 = call(lib, torch, d_rows, d_status, scale, 64, 256)
    _p2, s2 = call(lib, torch, d_rows, d_status, scale, 64, 256)
    _p3, s3 = call(lib, torch, d_rows, d_status, scale, 64, 256, dev_stats=True)
    assert s1.tobytes() == s2.tobytes() == s3.tobytes()


def test_argument_errors_enqueue_nothing(torch, lib):
    d_rows, d_status, scale, _rows, _status = synthetic_rows(torch, 1, 2, 8, seed=1)
    ld = d_rows.shape[-1]
    psf = torch.full((1, 2, 20, 20), -7.0, dtype=torch.float64, device='cuda')
    sc = np.ascontiguousarray(scale)
    bad_scale = np.array([np.inf])
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    R, S, P = d_rows.data_ptr(), d_status.data_ptr(), psf.data_ptr()
    cases = [((0, 2, R, ld, S, sc.ctypes.data, 8, 20, P, None), b'n_items'),
             ((abi.MAX_FOCUS_ITEMS + 1, 2, R, ld, S, sc.ctypes.data, 8, 20, P, None), b'n_items'),
             ((1, 0, R, ld, S, sc.ctypes.data, 8, 20, P, None), b'n_planes'),
             ((1, abi.MAX_FOCUS_PLANES + 1, R, ld, S, sc.ctypes.data, 8, 20, P, None), b'n_planes'),
             ((1, 2, R, ld, S, sc.ctypes.data, 7, 20, P, None), b'ndim'),
             ((1, 2, R, ld, S, sc.ctypes.data, 8, 8, P, None), b'maxdim'),
             ((1, 2, R, 63, S, sc.ctypes.data, 8, 20, P, None), b'ld'),
             ((1, 2, None, ld, S, sc.ctypes.data, 8, 20, P, None), b'rows'),
             ((1, 2, R, ld, None, sc.ctypes.data, 8, 20, P, None), b'status'),
             ((1, 2, R, ld, S, None, 8, 20, P, None), b'wave_scale'),
             ((1, 2, R, ld, S, bad_scale.ctypes.data, 8, 20, P, None), b'wave_scale'),
             ((1, 2, R, ld, S, sc.ctypes.data, 8, 20, None, None), b'psf and stats')]
    for args, name in cases:
        assert lib.rox_focus_psf(*args, st) == -1         # ROX_E_ARG
        msg = lib.rox_last_error()
        assert b'rox_focus_psf' in msg and name in msg, (args, msg)
    torch.cuda.synchronize()
    assert (psf == -7.0).all()


def _fixture_model():
    import sys
    import os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import focus_fixture
    z = focus_fixture.load()
    return focus_fixture.FocusFixtureModel(z, 'dblgauss')


def test_through_focus_psf_equals_through_focus_and_calc_psf(torch):
    """end to end: the drop-in's statistics are through_focus's bit for bit, and each plane's PSF
    is calc_psf of the OPD grid through_focus's rows give"""
    from rayoptics_amd import analyses
    from rayoptics_amd.engine import calc_psf
    m = _fixture_model()
    fld, wvl, focs = m.fields[0], m.wvl, m.focs
    ndim, maxdim = 32, 64
    tf = analyses.through_focus(m, fld, wvl, focs, num_rays=ndim, rows=True)
    res = analyses.through_focus_psf(m, fld, wvl, focs, num_rays=ndim, maxdim=maxdim)
    assert res.stats.tobytes() == tf.stats.tobytes()
    assert res.psf.shape == (len(focs), maxdim, maxdim)
    assert res.delta_x is None and res.delta_xp is None          # a table model has no paraxial data
    for k in range(len(focs)):
        opd = np.where(tf.status == abi.OK, tf.rows[k, 2], np.nan).reshape(ndim, ndim)
        assert np.array_equal(res.psf[k], calc_psf(opd, ndim, maxdim)), k
        n, s = numpy_strehl(opd)
        assert res.n[k] == n and abs(res.strehl[k] - s) <= 1e-12
    best = analyses.best_focus(focs, -res.strehl)
    assert (res.best_focus_strehl, res.best_focus_strehl_kind) == best
    dev = analyses.through_focus_psf(m, fld, wvl, focs, num_rays=ndim, maxdim=maxdim, on_device=True)
    assert isinstance(dev.psf, torch.Tensor) and dev.psf.is_cuda
    assert np.array_equal(dev.psf.cpu().numpy(), res.psf)
    none = analyses.through_focus_psf(m, fld, wvl, focs, num_rays=ndim, maxdim=maxdim, psf=False)
    assert none.psf is None and none.strehl.tobytes() == res.strehl.tobytes()


@pytest.mark.parametrize('field', ['f0', 'f1'])
def test_through_focus_psf_against_the_stored_reference(torch, field):
    """end to end against tests/golden/through_focus_psf.npz (the reference's focus_wavefront,
    calc_psf and calc_psf_scaling of the double Gauss at 7 foci, on axis and at full field): the
    OPD grids within 1e-10 relative to convert_to_opd, the PSFs within 1e-9 (both maxdims, one
    not a power of two), delta_x / delta_xp exactly, the Strehl ratio as NumPy gives it on the
    reference's grid, and the geometric statistics through_focus's bit for bit"""
    import focus_psf_fixture as PF
    from rayoptics_amd import analyses
    m = PF.FocusPsfFixtureModel(PF.load(), field)
    z, focs, fld = m.z, m.focs, m.fields[0]
    ndim, convert = int(z['ndim']), float(z['convert_to_opd'])
    tf = analyses.through_focus(m, fld, m.wvl, focs, num_rays=ndim, rows=True)
    for k in range(len(focs)):
        opd = np.where(tf.status == abi.OK, tf.rows[k, 2], np.nan).reshape(ndim, ndim)
        ref = z['opd'][k]
        assert np.array_equal(np.isnan(opd), np.isnan(ref)) and np.isfinite(ref).sum() > 500
        assert np.nanmax(np.abs(opd - ref)) <= 1e-10 * convert, k
    for j, M in enumerate(int(v) for v in z['maxdims']):
        res = analyses.through_focus_psf(m, fld, m.wvl, focs, num_rays=ndim, maxdim=M)
        assert res.stats.tobytes() == tf.stats.tobytes()
        assert np.array_equal(res.delta_x, z['psf_scaling'][:, j, 0])
        assert np.array_equal(res.delta_xp, z['psf_scaling'][:, j, 1])
        for k in range(len(focs)):
            n, s = numpy_strehl(z['opd'][k])
            assert res.n[k] == n and abs(res.strehl[k] - s) <= 1e-9, k
        if M == int(z['psf_maxdim']):
            for i, k in enumerate(z['psf_focs']):
                assert np.max(np.abs(res.psf[k] - z['psf'][i])) <= 1e-9, k
