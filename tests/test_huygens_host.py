"""Huygens PSFs without a GPU: the NumPy restatement of rox_huygens_psf (tests/huygens_ref.py)
against closed forms and against the unfactorised sum, the row construction of
analyses.trace_huygens_rows on packets from the CPU oracle (tests/oracle_engine.py), its agreement
with the reference's FFT PSF (tests/golden/psf.npz, through_focus_psf.npz), the sign of the OPD in
the phase (the PSF's centroid lies where the geometric spot's does), the argument errors of the C
entry, which come before a device is touched, and header against ctypes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import huygens_ref as HR
from rayoptics_amd import abi, analyses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement against closed forms ---------------------------------------------------------
def test_one_ray_is_a_squared_everywhere():
    rows = np.array([[0.3], [17.25], [-4.5], [1700.0]]).reshape(1, 4, 1)
    amp = np.array([[1.75]])
    planes = np.array([[[-0.01, 0.02, 0.0], [0.003, 0.0, -0.05]]])
    U, psf, st = HR.huygens_psf(rows, amp, np.zeros((1, 1), np.uint8), planes, 7, 5, 0.0013, 0.0021)
    # |a (c + i s)|^2 with c^2 + s^2 = 1 to two roundings of the correctly rounded c, s, then the square's
    assert np.abs(psf - 1.75 ** 2).max() <= 8 * 2.0 ** -53 * 1.75 ** 2
    assert (st['n'] == 1).all() and np.array_equal(st['norm'], np.full((1, 2), 1.75 ** 2))
    assert np.abs(st['strehl'] - 1.0).max() <= 8 * 2.0 ** -53


def dirichlet(n, x):
    """|sum_{j < n} exp(2 pi i j x)| = |sin(pi n x) / sin(pi x)|, n where x is an integer"""
    x = np.asarray(x, dtype=np.longdouble)
    pi = np.arccos(np.longdouble(-1.0))
    s = np.sin(pi * x)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(np.abs(s) < 1e-15, float(n), np.abs(np.sin(pi * n * x) / s)).astype(np.float64)


def lattice_case(n=6, step=12.5, xi0=-31.25, nx=33, ny=29, px=0.0011, py=0.0017):
    """a flat phase over an n x n lattice of (xi, eta) = xi0 + step * (i, j): the PSF is the product
    of two Dirichlet kernels of X step and Y step"""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
    rows = np.zeros((1, 4, n * n))
    rows[0, 0] = 0.125
    rows[0, 1], rows[0, 2] = (xi0 + step * i).reshape(-1), (xi0 + step * j).reshape(-1)
    rows[0, 3] = 1500.0
    planes = np.array([[[-px * (nx // 2), -py * (ny // 2), 0.0]]])
    X = planes[0, 0, 0] + np.arange(nx) * px
    Y = planes[0, 0, 1] + np.arange(ny) * py
    want = (dirichlet(n, step * X)[:, None] * dirichlet(n, step * Y)[None, :]) ** 2
    return rows, planes, nx, ny, px, py, want


def test_a_flat_phase_over_a_lattice_is_two_dirichlet_kernels():
    rows, planes, nx, ny, px, py, want = lattice_case()
    n2 = rows.shape[2]
    U, psf, st = HR.huygens_psf(rows, None, np.zeros((1, n2), np.uint8), planes, nx, ny, px, py)
    # |U| <= 36; each of the 36 terms carries the rounding of its argument (|t| < 2^6: 2^-47 absolute,
    # times 2 pi) and of the sum: a few 1e-13 of the peak 36^2
    assert np.abs(psf[0, 0] - want).max() <= 1e-11 * n2 ** 2
    assert st['peak_ix'][0, 0] == nx // 2 and st['peak_iy'][0, 0] == ny // 2
    assert abs(st['strehl'][0, 0] - 1.0) < 1e-12 and st['norm'][0, 0] == n2 ** 2


def test_the_factorised_sum_is_the_direct_sum():
    """random rows with |t| up to 2^10, failed rays, amplitudes: U = A B^T against the unfactorised
    long double sum to the bound of the device tests"""
    rng = np.random.default_rng(2)
    R, nx, ny = 49, 5, 3
    rows, amp, status, planes, px, py = synthetic(rng, 1, 2, R, nx, ny)
    U, _psf, st = HR.huygens_psf(rows, amp, status, planes, nx, ny, px, py)
    for k in range(2):
        ref = HR.direct_sum(rows[0, :, :R], amp[0, :R], status[0, :R], planes[0, k], nx, ny, px, py)
        # the direct sum adds its four argument terms in another order: up to 2^10 * 2^-52 cycles each
        tol = ((2 * R + 32) * 2.0 ** -53 + 2 * np.pi * 4 * 2.0 ** -43) * st['sum_abs'][0]
        assert max(np.abs(U[0, k].real - ref.real).max(), np.abs(U[0, k].imag - ref.imag).max()) <= tol


def synthetic(rng, n_items, K, R, nx, ny, ld=None):
    """rows whose every argument stays within 2^10 cycles, a third of the rays failed (their rows
    NaN: never read), amplitudes in [0.5, 1.5)"""
    ld = R + 3 if ld is None else ld
    px, py = 0.0021, 0.0013
    planes = np.empty((n_items, K, 3))
    planes[..., 0] = -px * (nx // 2) + rng.uniform(-px, px, (n_items, K))
    planes[..., 1] = -py * (ny // 2) + rng.uniform(-py, py, (n_items, K))
    planes[..., 2] = rng.uniform(-0.1, 0.1, (n_items, K))
    planes[:, 0, 2] = 0.0
    rows = np.full((n_items, 4, ld), np.nan)
    span_x, span_y = px * (nx + 1), py * (ny + 1)
    rows[:, 0, :R] = rng.uniform(-200.0, 200.0, (n_items, R))
    rows[:, 1, :R] = rng.uniform(-1.0, 1.0, (n_items, R)) * min(400.0, 200.0 / span_x)
    rows[:, 2, :R] = rng.uniform(-1.0, 1.0, (n_items, R)) * min(400.0, 200.0 / span_y)
    rows[:, 3, :R] = rng.uniform(1500.0, 1700.0, (n_items, R))          # zeta * dz <= 170
    status = np.full((n_items, ld), abi.BLOCKED, dtype=np.uint8)
    status[:, :R] = np.where(rng.random((n_items, R)) < 0.33, rng.integers(1, 5, (n_items, R)), 0)
    for c in range(4):
        rows[:, c, :R] = np.where(status[:, :R] == 0, rows[:, c, :R], np.nan)
    amp = np.full((n_items, ld), np.nan)
    amp[:, :R] = rng.uniform(0.5, 1.5, (n_items, R))
    return rows, amp, status, planes, px, py


# ---- rows from the CPU oracle, and the FFT PSF ----------------------------------------------------
def on_axis_rows():
    """the double Gauss on axis (tests/golden/through_focus_psf.npz f0), 32 x 32 rays over the
    pupil, traced by the CPU oracle: the Huygens rows about the reference sphere of every focus
    that has a golden PSF"""
    import focus_psf_fixture as fp
    from oracle_engine import OracleEngine
    from rayoptics_amd import session
    z = fp.load()
    model = fp.FocusPsfFixtureModel(z, 'f0')
    session._set_engine_factory(OracleEngine)
    try:
        rows = {int(k): analyses.trace_huygens_rows(model, flds=model.fields, wvls=[model.wvl], num_rays=32,
                                                    ref_foc=model.focs[int(k)]) for k in model.z['psf_focs']}
    finally:
        session._set_engine_factory(None)
    return model, rows


@pytest.fixture(scope='module')
def on_axis():
    return on_axis_rows()


def test_rows_are_the_opd_and_the_directions(on_axis):
    model, rows = on_axis
    d = model.z
    for k, hr in rows.items():
        r, st = hr.rows.numpy()[0, :, :1024], hr.status.numpy()[0, :1024]
        W = d['opd'][k].reshape(-1)                              # waves; NaN where no ray passes
        assert np.array_equal(st == 0, ~np.isnan(W)) and hr.n_rays == 1024 and (hr.status.numpy()[0, 1024:] != 0).all()
        ok = st == 0
        lam = model.nm_to_sys_units(model.wvl)
        # phi = -W - n q / (sqrt(R^2 - q) + R) / lambda: the second term is not negative, a fraction
        # of a wave, and zero for the chief ray
        corr = -(r[0, ok] + W[ok])
        print('focus', k, ': sphere-to-plane term, waves: max', corr.max(), 'min', corr.min())
        assert corr.min() > -1e-9 and 0.01 < corr.max() < 0.5
        # (xi, eta, zeta) lambda is a unit vector (n = 1) that points at +z
        nrm = np.sqrt((r[1:4, ok] ** 2).sum(axis=0)) * lam
        assert np.abs(nrm - 1.0).max() < 1e-12 and (r[3, ok] > 0).all()
        assert abs(hr.radii[0] - float(d['ref_radius'][k])) < 1e-9 * abs(hr.radii[0])
        assert hr.centres[0, 2] == model.focs[k] and np.allclose(hr.centres[0, :2], d['image_pt'][k])


def fft_grid(model, k, M):
    """calc_psf's pixels: image coordinates -p (j - M/2) about the image point, p = delta_xp; as an
    ascending grid that is x0 = -p (M/2 - 1), pixel a = M - 1 - j"""
    d = model.z
    mi = list(d['maxdims']).index(M)
    p = float(d['psf_scaling'][k, mi, 1])
    return p, -p * (M / 2 - 1)


def recorded_fft_differences():
    """what tools/huygens_psf_bench.py measured and wrote into the profile: the last record of
    profiles/r21_huygens_psf_bench.json (DESIGN.md 3.22 quotes it); the test allows twice each figure"""
    import json
    with open(os.path.join(ROOT, 'profiles', 'r21_huygens_psf_bench.json')) as f:
        return [r for r in json.load(f) if 'fft_psf_comparison' in r][-1]['fft_psf_comparison']


def huygens_on_fft_grid(hr, p, x0, M, dz=0.0, scale_opd=None):
    rows = hr.rows.numpy()
    if scale_opd is not None:
        rows = rows.copy()
        rows[0, 0, :1024] = scale_opd * rows[0, 0, :1024]        # the OPD and its sphere-to-plane term alike
    _U, psf, _st = HR.huygens_psf(rows, None, hr.status.numpy(), np.array([[[x0, x0, dz]]]), M, M, p, p,
                                  n_rays=hr.n_rays)
    h = psf[0, 0][::-1, ::-1]
    return h / h.max()


def fft_differences(model, rows):
    """largest absolute differences of peak-normalised PSFs, Huygens at calc_psf's pixels against
    the reference's FFT PSF: at focus 0 and at the defocused plane (maxdim 64), that plane again
    from the sphere of focus 0 displaced by dz, focus 0 at maxdim 128 (tests/golden/psf.npz), and
    focus 0 with the wavefront scaled to 2 % against the NumPy restatement of calc_psf"""
    from test_through_focus_psf_host import numpy_calc_psf
    d = model.z
    M = int(d['psf_maxdim'])
    p, x0 = fft_grid(model, 3, M)
    p6, x06 = fft_grid(model, 6, M)
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'psf.npz'))
    assert np.array_equal(np.nan_to_num(g['dblgauss_f0/opd']), np.nan_to_num(d['opd'][3]))
    _dx, p128 = analyses.psf_scaling(model, model.wvl, 32, 128, float(d['ref_radius'][3]))
    diff = lambda a, b: float(np.abs(a - b).max())  # noqa: E731
    return {'focus_0': diff(huygens_on_fft_grid(rows[3], p, x0, M), d['psf'][1]),
            'defocused': diff(huygens_on_fft_grid(rows[6], p6, x06, M), d['psf'][2]),
            'defocused_through_dz': diff(huygens_on_fft_grid(rows[3], p6, x06, M, dz=model.focs[6] - model.focs[3]),
                                         d['psf'][2]),
            'focus_0_maxdim_128': diff(huygens_on_fft_grid(rows[3], p128, -p128 * 63, 128), g['dblgauss_f0/psf']),
            'wavefront_at_2_percent': diff(huygens_on_fft_grid(rows[3], p, x0, M, scale_opd=0.02),
                                           numpy_calc_psf(0.02 * d['opd'][3], 32, M))}


def test_agreement_with_the_fft_psf(on_axis):
    """Peak-normalised Huygens PSF at calc_psf's pixels against the reference's FFT PSF, each
    difference within twice what the profile records.  At the paraxial focus this lens carries 18
    waves peak to valley on axis (5.8 rms): 32 rays across undersample it, the FFT aliases and the
    Huygens sum, with the rays' real directions, aliases differently -- the two differ by more than
    half the peak, and twice that bounds nothing: against the stored PSFs, whose grid is 32 x 32
    rays, this test can only fail by an error.  What it can tell is in the last figure: the same
    rays with the wavefront scaled to 2 % (0.37 waves peak to valley), where both are well sampled,
    agree to 0.024 of the peak, the paraxial pitch against real directions; no stored PSF exists
    for that wavefront, so the FFT side is the suite's NumPy restatement of calc_psf."""
    model, rows = on_axis
    got, recorded = fft_differences(model, rows), recorded_fft_differences()
    print('Huygens against the FFT PSF:', got, 'recorded:', recorded)
    assert sorted(got) == sorted(recorded)
    for name, v in got.items():
        assert v <= 2 * recorded[name], name


def test_the_psf_centroid_is_the_geometric_centroid():
    """Full field (f1), 64 x 64 rays of which the inner half of the pupil counts, at the plane of
    the smallest geometric spot: the centroid of |U|^2 is the mean transverse aberration of the
    rays (the centroid theorem) -- and with the other sign of the OPD, the PSF of the conjugate
    wavefront, it is not.  This pins HUYGENS_OPD_SIGN.  (The case named for this was a tilt added
    to W.  A tilt tau * L added to W shifts the PSF by -HUYGENS_OPD_SIGN * tau / n by construction;
    which way the geometric spot of such a wavefront moves is the very convention in question, so
    the test takes rays whose transverse aberrations and OPDs both come from the trace.)"""
    import focus_psf_fixture as fp
    from oracle_engine import OracleEngine
    from rayoptics_amd import session
    from rayoptics_amd.engine import make_grid
    from rayoptics_amd.trace import _launch_setup
    model = fp.FocusPsfFixtureModel(fp.load(), 'f1')
    N = 64
    session._set_engine_factory(OracleEngine)
    try:
        hr = analyses.trace_huygens_rows(model, flds=model.fields, wvls=[model.wvl], num_rays=N, ref_foc=0.0)
        _e, f, wi, o = _launch_setup(model, model.fields[0], model.wvl,
                                     dict(check_apertures=True, apply_vignetting=True), abi.OUT_LAST)
        seg = hr.eng.trace_pupil_grids([f], [wi], make_grid((-1., -1.), (1., 1.), N), [o])[0].seg.numpy()
    finally:
        session._set_engine_factory(None)
    g = np.arange(N) / (N - 1) * 2 - 1
    status = hr.status.numpy().copy()
    status[0, :N * N][(g[:, None] ** 2 + g[None, :] ** 2).reshape(-1) > 0.25] = abi.BLOCKED
    ok = status[0, :N * N] == 0
    c = hr.centres[0]

    def spot(dz):
        P = seg[0:3][:, ok] + ((dz - seg[2, ok]) / seg[5, ok]) * seg[3:6][:, ok]
        return P[:2] - c[:2, None]
    dzs = np.linspace(-1.0, 1.0, 201)
    dz = float(dzs[np.argmin([spot(z).std(axis=1).sum() for z in dzs])])
    ta = spot(dz)
    geo = ta.mean(axis=1)
    half = np.abs(ta - geo[:, None]).max()
    S, p = 128, 0.001
    origin = np.round(geo / p) * p - (S // 2) * p
    planes = np.array([[[origin[0], origin[1], dz]]])
    X, Y = origin[0] + np.arange(S) * p, origin[1] + np.arange(S) * p
    got = {}
    for sign in (-1.0, 1.0):
        rows = hr.rows.numpy().copy()
        if sign != analyses.HUYGENS_OPD_SIGN:                    # phi = sign W - term: flip the OPD's part
            rows[0, 0] = flip_opd(rows[0, 0], seg, c, hr.radii[0], model.nm_to_sys_units(model.wvl), N * N)
        _U, psf, st = HR.huygens_psf(rows, None, status, planes, S, S, p, p, n_rays=N * N)
        h = psf[0, 0]
        got[sign] = np.array([(h.sum(axis=1) * X).sum(), (h.sum(axis=0) * Y).sum()]) / h.sum()
        ring = (h[0].sum() + h[-1].sum() + h[1:-1, 0].sum() + h[1:-1, -1].sum()) / h.sum()
        print('OPD sign', sign, 'plane dz', dz, 'geometric centroid', geo, 'spot half width', half, 'PSF centroid',
              got[sign], 'border ring share', ring, 'rays', int(ok.sum()))
    right, wrong = got[analyses.HUYGENS_OPD_SIGN], got[-analyses.HUYGENS_OPD_SIGN]
    # The plane's shift along the chief ray moves both alike; what the sign turns over is the part
    # the aberrations add.  Measured: 0.09 um with the sign of waveabr.py, 0.9 um with the other, on
    # 1 um pixels with 0.4 % of the light in the border ring.  A quarter pixel separates them.
    assert np.hypot(*(right - geo)) < 0.25 * p
    assert np.hypot(*(wrong - geo)) > 0.5 * p


def flip_opd(phi, seg, c, radius, lam, R):
    """phi = s W / lambda - term / lambda -> -s W / lambda - term / lambda, the term recomputed from the packet"""
    ta = seg[0:3, :R] - c[:, None]
    d = seg[3:6, :R]
    dta = (d * ta).sum(axis=0)
    q = (ta * ta).sum(axis=0) - dta * dta
    term = q / (np.sqrt(radius * radius - q) + abs(radius)) / lam
    out = phi.copy()
    out[:R] = -(phi[:R] + term) - term
    return out


def test_an_infinite_reference_sphere_is_refused():
    import focus_psf_fixture as fp
    from oracle_engine import OracleEngine
    from rayoptics_amd import session
    from rayoptics_amd.table import wavefront_to_array

    class Telecentric(fp.FocusPsfFixtureModel):
        def setup_pupil_coords(self, fld, wvl, foc, image_pt=None, image_delta=None):
            out = super().setup_pupil_coords(fld, wvl, foc, image_pt, image_delta)
            w = fld.rox_wavefront
            w.ref_radius = 1e12
            w.kind = abi.WF_INF_FULL
            assert len(wavefront_to_array(w))
            return out
    model = Telecentric(fp.load(), 'f0')
    session._set_engine_factory(OracleEngine)
    try:
        with pytest.raises(ValueError, match='reference sphere'):
            analyses.trace_huygens_rows(model, flds=model.fields, wvls=[model.wvl], num_rays=8)
    finally:
        session._set_engine_factory(None)


def test_window_and_planes():
    o = analyses.huygens_window((0.25, -1.0), 24, 0.01)
    assert np.allclose(o, [0.25 - 0.12, -1.0 - 0.12])
    centres = np.array([[0.25, -1.0, 0.0], [0.26, -1.0, 0.0]])
    pl = analyses.huygens_planes(centres, [o], [-0.1, 0.0, 0.2], 2)
    assert pl.shape == (2, 3, 3) and np.array_equal(pl[0, :, 2], [-0.1, 0.0, 0.2])
    assert HR.origin_pixel(pl[0, 0, 0], 0.01, 24) == 12 and HR.origin_pixel(pl[1, 1, 0], 0.01, 24) == 13
    with pytest.raises(ValueError, match='pixel_pitch'):
        analyses.huygens_psf(None, 0.0)
    with pytest.raises(ValueError, match='size'):
        analyses.huygens_psf(None, 0.01, size=5000)


# ---- the C entry --------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from rayoptics_amd.engine import load_library
    return load_library()


def call(lib, n_items=1, n_planes=1, n_rays=8, ld=8, nx=4, ny=4, pitch_x=0.01, pitch_y=0.01, planes=None,
         rows=1, status=1, outs=(1, 0, 0)):
    planes = np.zeros((max(n_items, 1), max(n_planes, 1), 3)) if planes is None else planes
    buf = np.zeros(64)                  # stands for a device pointer: no check dereferences it
    rc = lib.rox_huygens_psf(n_items, n_planes, n_rays, buf.ctypes.data if rows else None, ld, None,
                             buf.ctypes.data if status else None,
                             planes.ctypes.data if planes is not False else None, nx, ny, pitch_x, pitch_y,
                             *[buf.ctypes.data if o else None for o in outs], None)
    return rc, lib.rox_last_error().decode()


def test_argument_errors_come_before_a_device(lib):
    errors = json_errors()
    bad = np.zeros((1, 2, 3))
    bad[0, 1, 2] = np.inf
    cases = {'n_items 0': dict(n_items=0), 'n_items 1025': dict(n_items=1025), 'n_planes 0': dict(n_planes=0),
             'n_planes 257': dict(n_planes=257), 'nx 0': dict(nx=0), 'ny 4097': dict(ny=4097),
             'n_rays 0': dict(n_rays=0), 'n_rays > ld': dict(n_rays=9), 'ld 0': dict(ld=0, n_rays=1),
             'pitch_x 0': dict(pitch_x=0.0), 'pitch_x nan': dict(pitch_x=float('nan')),
             'pitch_y negative': dict(pitch_y=-0.01), 'pitch_y inf': dict(pitch_y=float('inf')),
             'rows null': dict(rows=0), 'status null': dict(status=0), 'planes null': dict(planes=False),
             'planes not finite': dict(n_planes=2, planes=bad), 'outputs all null': dict(outs=(0, 0, 0)),
             # 16 * 2^28 * (4096 + 4096) bytes for one plane: beyond the scratch bound
             'one plane beyond the scratch': dict(n_rays=1 << 28, ld=1 << 28, nx=4096, ny=4096)}
    assert list(cases) == [c[0] for c in errors]
    for (name, kw), (_n, want_rc, want_msg) in zip(cases.items(), errors):
        rc, msg = call(lib, **kw)
        assert (rc, msg) == (want_rc, want_msg) and msg.startswith('rox_huygens_psf: '), (name, rc, msg)


def json_errors():
    """tests/golden/huygens_entry_errors.json: [name, return code, rox_last_error() text] per call, in order"""
    import json
    with open(os.path.join(ROOT, 'tests', 'golden', 'huygens_entry_errors.json')) as f:
        return json.load(f)['calls']


def test_header_binding_and_struct_agree(tmp_path, lib):
    src = open(os.path.join(ROOT, 'include', 'roxtrace.h')).read()
    assert 'int rox_huygens_psf(int32_t n_items, int32_t n_planes, int64_t n_rays,' in src
    assert 'rox_huygens_psf' in abi.EXPORTS and hasattr(lib, 'rox_huygens_psf')
    assert len(lib.rox_huygens_psf.argtypes) == 16 and abi.ABI_VERSION == 8
    from rayoptics_amd.engine import HUYGENS_STATS_DTYPE
    names = [n for n, _t in abi.HuygensStats._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/roxtrace.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(rox_huygens_stats));']
    lines += [f'printf("{n} %zu\\n", offsetof(rox_huygens_stats, {n}));' for n in names] + ['return 0; }']
    (tmp_path / 'layout.c').write_text('\n'.join(lines))
    subprocess.check_call(['gcc', '-o', str(tmp_path / 'layout'), str(tmp_path / 'layout.c')])
    got = dict(line.split() for line in subprocess.check_output([str(tmp_path / 'layout')], text=True).splitlines())
    assert int(got['size']) == C.sizeof(abi.HuygensStats) == HUYGENS_STATS_DTYPE.itemsize == 48
    for n in names:
        assert int(got[n]) == getattr(abi.HuygensStats, n).offset == HUYGENS_STATS_DTYPE.fields[n][1], n
