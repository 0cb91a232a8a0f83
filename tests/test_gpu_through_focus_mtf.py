"""rox_focus_mtf on the device: the line OTFs match the NumPy restatement (tests/line_otf.py),
nu = 0 gives exactly (1, 0), over-Nyquist and empty planes give NaN, repeated calls and host /
device destinations are bit-identical, argument errors are refused before anything is enqueued,
and analyses.through_focus_mtf on the double Gauss agrees with the reference's stored PSFs, the
pupil autocorrelation of its OPD grids and its spot centroid (tests/golden/through_focus_mtf.npz)."""
import ctypes as C
import os

import numpy as np
import pytest

import line_otf as LO
from rayoptics_amd import abi

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'through_focus_mtf.npz')


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


def synthetic_psf(n_items, K, M, seed, empty=()):
    """smooth non-negative blobs, off centre, with a little noise; planes in ``empty`` are NaN
    (what rox_focus_psf writes for a plane no ray reached)"""
    rng = np.random.default_rng(seed)
    j = np.arange(M) - M // 2
    out = np.empty((n_items, K, M, M))
    for i in range(n_items):
        for k in range(K):
            cx, cy = rng.uniform(-M / 8, M / 8, 2)
            sx, sy = rng.uniform(M / 40, M / 10, 2)
            out[i, k] = np.exp(-((j[:, None] - cx) / sx) ** 2 - ((j[None, :] - cy) / sy) ** 2)
            out[i, k] += 1e-3 * rng.random((M, M))
    for i, k in empty:
        out[i, k] = np.nan
    return out


def call(lib, torch, d_psf, pitch, freqs, dev_out=False):
    n_items, K, M, _M = d_psf.shape
    Q = len(freqs)
    p = np.ascontiguousarray(np.broadcast_to(pitch, (n_items, K)), dtype=np.float64)
    f = np.ascontiguousarray(freqs, dtype=np.float64)
    if dev_out:
        out = torch.empty((n_items, K, 2, Q, 2), dtype=torch.float64, device='cuda')
        ptr = out.data_ptr()
    else:
        out = np.empty((n_items, K, 2, Q, 2))
        ptr = out.ctypes.data
    rc = lib.rox_focus_mtf(n_items, K, d_psf.data_ptr(), M, p.ctypes.data, Q, f.ctypes.data, ptr,
                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.rox_last_error()
    torch.cuda.synchronize()
    if dev_out:
        out = out.cpu().numpy()
    return out


def as_complex(out):
    return out[..., 0] + 1j * out[..., 1]


@pytest.mark.parametrize('M', [64, 128, 256, 512])
def test_matches_the_numpy_line_otf(torch, lib, M):
    """odd Q, mixed pitches (some frequencies above some planes' Nyquist), within 1e-12"""
    n_items, K = 3, 5
    psf = synthetic_psf(n_items, K, M, seed=M)
    rng = np.random.default_rng(M + 1)
    pitch = rng.uniform(0.5e-3, 2e-3, size=(n_items, K))
    freqs = np.array([0.0, 3.0, 17.5, 60.0, 130.0, 260.0, 420.0])
    got = as_complex(call(lib, torch, torch.from_numpy(psf).cuda(), pitch, freqs))
    exp = LO.line_otf(psf, pitch, freqs)
    assert np.array_equal(np.isnan(got), np.isnan(exp))
    assert np.isnan(got).any() and (~np.isnan(got)).sum() > 100
    ok = ~np.isnan(exp)
    assert np.max(np.abs(got[ok] - exp[ok])) <= 1e-12


def test_zero_frequency_nyquist_and_empty_planes(torch, lib):
    M = 96
    psf = synthetic_psf(2, 3, M, seed=3, empty=[(1, 2)])
    psf[0, 1] = 0.0                                     # no light at all
    pitch = np.full((2, 3), 1e-3)
    freqs = np.array([0.0, 499.0, 499.9, 500.5, 1e4])   # nu p = 0, 0.499, 0.4999, 0.5005, 10
    out = call(lib, torch, torch.from_numpy(psf).cuda(), pitch, freqs)
    lit = [(0, 0), (0, 2), (1, 0), (1, 1)]
    for i, k in lit:
        assert (out[i, k, :, 0, 0] == 1.0).all() and (out[i, k, :, 0, 1] == 0.0).all()
        assert not np.signbit(out[i, k, :, 0, 1]).any()
        assert np.isfinite(out[i, k, :, 1:3]).all()
        assert np.isnan(out[i, k, :, 3:]).all()
    assert np.isnan(out[0, 1]).all() and np.isnan(out[1, 2]).all()


def test_reproducible_host_or_device_and_across_launch_splits(torch, lib):
    """identical calls, host and device destinations, and one-plane calls give the same bytes"""
    M, K = 512, 21
    psf = synthetic_psf(1, K, M, seed=9)
    d = torch.from_numpy(psf).cuda()
    pitch = np.linspace(0.8e-3, 1.2e-3, K)
    freqs = np.linspace(0.0, 400.0, 9)
    a = call(lib, torch, d, pitch, freqs)
    b = call(lib, torch, d, pitch, freqs)
    c = call(lib, torch, d, pitch, freqs, dev_out=True)
    assert a.tobytes() == b.tobytes() == c.tobytes()
    for k in (0, 7, 20):
        one = call(lib, torch, d[:, k:k + 1].contiguous(), pitch[k:k + 1], freqs)
        assert one.tobytes() == a[:, k:k + 1].tobytes()


def test_argument_errors_enqueue_nothing(torch, lib):
    M = 32
    d = torch.from_numpy(synthetic_psf(1, 2, M, seed=1)).cuda()
    out = torch.full((1, 2, 2, 3, 2), -7.0, dtype=torch.float64, device='cuda')
    pitch = np.full(2, 1e-3)
    freqs = np.array([0.0, 10.0, 20.0])
    bad_p = np.array([1e-3, -1.0])
    bad_f = np.array([0.0, np.nan, 1.0])
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P, PI, FR, O = d.data_ptr(), pitch.ctypes.data, freqs.ctypes.data, out.data_ptr()
    cases = [((0, 2, P, M, PI, 3, FR, O), b'n_items'),
             ((abi.MAX_FOCUS_ITEMS + 1, 2, P, M, PI, 3, FR, O), b'n_items'),
             ((1, 0, P, M, PI, 3, FR, O), b'n_planes'),
             ((1, abi.MAX_FOCUS_PLANES + 1, P, M, PI, 3, FR, O), b'n_planes'),
             ((1, 2, P, 1, PI, 3, FR, O), b'maxdim'),
             ((1, 2, P, M, PI, 0, FR, O), b'n_freq'),
             ((1, 2, P, M, PI, abi.MAX_MTF_FREQS + 1, FR, O), b'n_freq'),
             ((1, 2, None, M, PI, 3, FR, O), b'psf'),
             ((1, 2, P, M, None, 3, FR, O), b'pitch'),
             ((1, 2, P, M, PI, 3, None, O), b'freqs'),
             ((1, 2, P, M, PI, 3, FR, None), b'otf'),
             ((1, 2, P, M, bad_p.ctypes.data, 3, FR, O), b'pitch[1]'),
             ((1, 2, P, M, PI, 3, bad_f.ctypes.data, O), b'freqs[1]')]
    for args, name in cases:
        assert lib.rox_focus_mtf(*args, st) == -1           # ROX_E_ARG
        msg = lib.rox_last_error()
        assert b'rox_focus_mtf' in msg and name in msg, (args, msg)
    torch.cuda.synchronize()
    assert (out == -7.0).all()


def test_engine_wrapper(torch):
    from rayoptics_amd.engine import TraceEngine
    from rayoptics_amd import SurfaceTable
    tbl = SurfaceTable.from_prescription([dict(cv=0, thi=10.0), dict(cv=0.02, thi=3.0, n=1.5), dict(cv=0, thi=0)])
    eng = TraceEngine(tbl)
    psf = synthetic_psf(2, 3, 64, seed=5)
    d = torch.from_numpy(psf).cuda()
    freqs = [0.0, 50.0, 120.0]
    host = eng.focus_mtf(d, 1e-3, freqs)
    dev = eng.focus_mtf(d, 1e-3, freqs, on_device=True)
    assert host.shape == (2, 3, 2, 3) and host.dtype == np.complex128
    assert dev.is_cuda and dev.dtype == torch.complex128
    assert np.array_equal(dev.cpu().numpy(), host)
    exp = LO.line_otf(psf, 1e-3, freqs)
    assert np.max(np.abs(host - exp)) <= 1e-12


# ---- the double Gauss against the stored reference --------------------------------------------
def _model():
    import focus_map_fixture as FM
    return FM.FocusMapFixtureModel(np.load(GOLDEN), 'dblgauss')


def _run(m, nu=None, **kw):
    from rayoptics_amd import analyses
    z = m.z
    ndim, M = int(z['ndim']), int(z['maxdims'][0])
    pitch = z['psf_scaling'][:, :, :, 0, 1]
    nu = np.array([0.0, 5.0, 20.0, 45.0, 80.0, 140.0, 250.0, 400.0]) if nu is None else nu
    args = dict(m.map_kwargs(), num_rays=ndim, maxdim=M, pitch=pitch)
    args.update(kw)
    return analyses.through_focus_mtf(m, m.focs, nu, **args), nu, pitch


def _one(m, f, w, pitch, **kw):
    """item (f, w) alone"""
    return _run(m, flds=[m.fields[f]], wvls=[m.wvls[w]], field_wts=[1.0], spectral_wts=[1.0], ref_wvl=m.wvls[w],
                pitch=pitch, **kw)[0]


def test_double_gauss_against_the_stored_reference(torch):
    """on axis and off axis (a field with an x component), at every wavelength: the OTFs are the
    NumPy line OTF of the device's PSFs within 1e-11; the PSFs are the reference's calc_psf
    within 1e-9 (as test_gpu_through_focus_psf.py holds them), the OTFs the line OTF of the
    reference's PSFs within 1e-9, and at lattice frequencies the pupil autocorrelation of the
    reference's OPD grids; the F W batch is bit-identical to single-item calls and to a forced
    small PSF bound"""
    from rayoptics_amd import analyses
    m = _model()
    z = m.z
    F, W, K = z['opd'].shape[:3]
    ndim, M = int(z['ndim']), int(z['maxdims'][0])
    res, nu, pitch = _run(m, psf=True)
    assert res.otf.shape == (F, W, K, 2, nu.size) and res.psf.shape == (F, W, K, M, M)
    exp = LO.line_otf(res.psf, pitch, nu)
    assert np.array_equal(np.isnan(exp), np.isnan(res.otf))
    ok = ~np.isnan(exp)
    assert np.max(np.abs(res.otf[ok] - exp[ok])) <= 1e-11
    for f in range(F):
        for w in range(W):
            k = K // 2
            ref = LO.line_otf(z['psf'][f, w], pitch[f, w, k], nu)
            assert np.array_equal(np.isnan(ref), np.isnan(res.otf[f, w, k]))
            assert np.max(np.abs(res.psf[f, w, k] - z['psf'][f, w])) <= 1e-9, (f, w)
            assert np.nanmax(np.abs(res.otf[f, w, k] - ref)) <= 1e-9, (f, w)
            # lattice frequencies: the autocorrelation of the reference's OPD grid
            mm = np.arange(M // 2)
            lat = _one(m, f, w, np.full((1, 1, K), pitch[f, w, k]), nu=mm / (M * pitch[f, w, k]))
            ac = LO.autocorrelation_otf(z['opd'][f, w, k], ndim, M, mm)
            assert np.max(np.abs(lat.otf[0, 0, k] - ac)) <= 1e-9, (f, w)
            assert np.array_equal(lat.poly_otf[0], lat.otf[0, 0])      # one wavelength: itself
    # single-item calls and a PSF bound of one item give the same bytes
    for f in range(F):
        for w in range(W):
            one = _one(m, f, w, pitch[f:f + 1, w:w + 1])
            assert one.otf.tobytes() == res.otf[f:f + 1, w:w + 1].tobytes()
    old = analyses.MTF_PSF_CHUNK_BYTES
    analyses.MTF_PSF_CHUNK_BYTES = K * M * M * 8
    try:
        small, _nu, _p = _run(m)
    finally:
        analyses.MTF_PSF_CHUNK_BYTES = old
    assert small.otf.tobytes() == res.otf.tobytes() and small.poly_otf.tobytes() == res.poly_otf.tobytes()
    assert list(res.meridional) == [True, False]
    assert np.isnan(res.tangential[1]).all() and np.isfinite(res.tangential[0][:, :3]).all()
    dev, _nu, _p = _run(m, psf=True, on_device=True)
    assert dev.psf.is_cuda and np.array_equal(dev.psf.cpu().numpy(), res.psf)


def test_orientation_against_the_reference_spot_centroid(torch):
    """off axis (a field with x and y components, centroid 4 and 5.6 pitches from the image point)
    on the fine grid, where the PSF does not alias: the PSF's centroid in image coordinates is the
    reference's geometric spot centroid within 5 %, in both directions, and the OTF's phase at
    low frequency is -2 pi nu times it.  (The diffraction centroid of a sampled pupil and the
    mean of its rays agree to about 2 % here; the reference's own calc_psf gives the same, see
    test_through_focus_mtf_reference.py.)"""
    m = _model()
    z = m.z
    n = int(z['ndim_fine'])
    c = list(m.wvls).index(m.central_wvl)
    pitch = z['psf_scaling_fine'][1, :, 1]
    K = len(m.focs)
    nu = np.array([0.0, 0.02 / (2 * n * pitch.mean())])
    res = _one(m, 1, c, pitch.reshape(1, 1, K), nu=nu, num_rays=n, maxdim=2 * n, psf=True, on_device=True)
    geo = z['centroid_fine'][1]                                         # [K, 2]
    psf = res.psf[0, 0].cpu().numpy()
    got = LO.psf_centroid(psf, pitch)
    assert np.all(np.abs(geo) > 3 * pitch[:, None])
    assert np.all(np.sign(got) == np.sign(geo))
    assert np.all(np.abs(got - geo) <= 0.05 * np.abs(geo)), (got / pitch[:, None], geo / pitch[:, None])
    phase = np.angle(res.otf[0, 0, :, :, 1])                           # [K, 2]
    np.testing.assert_allclose(phase, -2 * np.pi * nu[1] * got, rtol=0.05)
