"""CPU-side checks of diffraction through focus (rox_focus_psf, analyses.through_focus_psf): the
struct against the header, argument errors without a device, the Strehl best-focus rule, and the
result object assembled from an engine double that serves focus_psf with NumPy."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from rayoptics_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        'rox_build', os.path.join(ROOT, 'ray-optics_amd', 'build.py'))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return abi.declare(C.CDLL(b.build()))


def test_focus_psf_stats_layout_matches_header(tmp_path):
    st = abi.FocusPsfStats
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/roxtrace.h"',
             'int main(void) {', 'printf("size %zu\\n", sizeof(rox_focus_psf_stats));']
    for fname, _t in st._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(rox_focus_psf_stats, {fname}));')
    lines += ['return 0; }']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-o', str(exe), str(src)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got['size']) == C.sizeof(st) == 32
    for fname, _t in st._fields_:
        assert int(got[fname]) == getattr(st, fname).offset, fname
    assert 'rox_focus_psf' in abi.EXPORTS
    from rayoptics_amd.engine import FOCUS_PSF_STATS_DTYPE
    assert FOCUS_PSF_STATS_DTYPE.names == ('n', 'strehl', 'psf_peak', 'reserved')


def test_c_argument_errors_without_a_device(lib):
    """every check of rox_focus_psf comes before it touches a device: each returns ROX_E_ARG and
    names its parameter"""
    rows = np.zeros(3 * 64 * 2)
    status = np.zeros(64, dtype=np.uint8)
    sc = np.array([2.0])
    out = np.zeros(2 * 20 * 20)
    R, S, P, W = rows.ctypes.data, status.ctypes.data, out.ctypes.data, sc.ctypes.data
    nan = np.array([np.nan])
    cases = [((0, 2, R, 64, S, W, 8, 20, P, None), b'n_items'),
             ((abi.MAX_FOCUS_ITEMS + 1, 2, R, 64, S, W, 8, 20, P, None), b'n_items'),
             ((1, 0, R, 64, S, W, 8, 20, P, None), b'n_planes'),
             ((1, abi.MAX_FOCUS_PLANES + 1, R, 64, S, W, 8, 20, P, None), b'n_planes'),
             ((1, 2, R, 64, S, W, 9, 20, P, None), b'ndim'),
             ((1, 2, R, 64, S, W, 0, 20, P, None), b'ndim'),
             ((1, 2, R, 64, S, W, 8, 8, P, None), b'maxdim'),
             ((1, 2, R, 63, S, W, 8, 20, P, None), b'ld'),
             ((1, 2, None, 64, S, W, 8, 20, P, None), b'rows'),
             ((1, 2, R, 64, None, W, 8, 20, P, None), b'status'),
             ((1, 2, R, 64, S, None, 8, 20, P, None), b'wave_scale'),
             ((1, 2, R, 64, S, nan.ctypes.data, 8, 20, P, None), b'wave_scale[0]'),
             ((1, 2, R, 64, S, W, 8, 20, None, None), b'psf and stats')]
    for args, name in cases:
        assert lib.rox_focus_psf(*args, None) == -1, args
        msg = lib.rox_last_error()
        assert msg.startswith(b'rox_focus_psf') and name in msg, (args, msg)


def test_python_argument_errors_before_any_launch():
    """odd num_rays, a maxdim the grid does not fit in and K outside [1, 256] raise ValueError
    before the model is touched (the model here has nothing to trace)"""
    from rayoptics_amd import analyses
    model, fld = object(), object()
    with pytest.raises(ValueError, match='even'):
        analyses.through_focus_psf(model, fld, 550.0, [0.0], num_rays=31, maxdim=128)
    with pytest.raises(ValueError, match='does not fit'):
        analyses.through_focus_psf(model, fld, 550.0, [0.0], num_rays=32, maxdim=32)
    with pytest.raises(ValueError, match='focus values'):
        analyses.through_focus_psf(model, fld, 550.0, [], num_rays=32, maxdim=128)
    with pytest.raises(ValueError, match='focus values'):
        analyses.through_focus_psf(model, fld, 550.0, np.zeros(abi.MAX_FOCUS_PLANES + 1), num_rays=32)


def _psf_stats(strehl, n=100, peak=None):
    from rayoptics_amd.engine import FOCUS_PSF_STATS_DTYPE
    s = np.zeros(len(strehl), dtype=FOCUS_PSF_STATS_DTYPE)
    s['n'], s['strehl'] = n, strehl
    s['psf_peak'] = peak if peak is not None else np.asarray(strehl) * n * n
    return s


def test_best_focus_strehl_is_the_peak():
    from rayoptics_amd import analyses
    from rayoptics_amd.engine import FOCUS_STATS_DTYPE
    focs = np.linspace(-0.03, 0.03, 7)
    strehl = 0.9 * np.exp(-((focs - 0.004) / 0.012) ** 2)
    geo = np.zeros(7, dtype=FOCUS_STATS_DTYPE)
    r = analyses.ThroughFocusPSF(focs, geo, _psf_stats(strehl), None)
    i = int(np.argmax(strehl))
    assert r.best_focus_strehl_kind == 'vertex'
    assert focs[i - 1] <= r.best_focus_strehl <= focs[i + 1]
    assert abs(r.best_focus_strehl - 0.004) < 0.002
    # the maximum at the end of the scan
    r = analyses.ThroughFocusPSF(focs, geo, _psf_stats(np.linspace(0.1, 0.8, 7)), None)
    assert (r.best_focus_strehl, r.best_focus_strehl_kind) == (focs[-1], 'end')
    r = analyses.ThroughFocusPSF(focs, geo, _psf_stats(np.full(7, np.nan), n=0), None)
    assert r.best_focus_strehl_kind == 'none'


class _Rows:
    def __init__(self, rows, status):
        self.rows, self.status = rows, status


class _NumpyFocusEngine:
    """the two device entries through_focus_psf uses, served on the host: rows from a synthetic
    wavefront per plane, focus_psf as the reference's calc_psf arithmetic (NumPy FFT) + Strehl"""

    def __init__(self, num, K):
        rng = np.random.default_rng(0)
        self.R = num * num
        self.opd = rng.normal(scale=2e-4, size=(K, self.R))
        self.status = np.where(rng.random(self.R) < 0.2, abi.BLOCKED, abi.OK).astype(np.uint8)
        self.calls = []

    def trace_pupil_grid_focus(self, fld, grid, wvl_idx, opts, planes, want_rows=False, want_stats=True):
        from rayoptics_amd.engine import FOCUS_STATS_DTYPE
        K = len(planes)
        self.calls.append(('trace', K, want_rows, want_stats))
        rows = np.full((K, 3, self.R), np.nan)
        rows[:, 2] = self.opd
        stats = np.zeros(K, dtype=FOCUS_STATS_DTYPE)
        stats['n'] = (self.status == abi.OK).sum()
        stats['opd_rms'] = np.arange(K)
        return stats, _Rows(rows, self.status)

    def focus_psf(self, focus_rows, ndim, maxdim, wave_scale, want_psf=True):
        import torch
        self.calls.append(('psf', ndim, maxdim, wave_scale, want_psf))
        K = focus_rows.rows.shape[0]
        psf = np.empty((1, K, maxdim, maxdim))
        st = _psf_stats(np.zeros(K))
        for k in range(K):
            w = np.where(focus_rows.status == abi.OK, wave_scale * focus_rows.rows[k, 2], np.nan)
            w = w.reshape(ndim, ndim)
            psf[0, k] = numpy_calc_psf(w, ndim, maxdim)
            ok = ~np.isnan(w)
            ph = np.exp(1j * 2 * np.pi * w[ok])
            st['n'][k] = ok.sum()
            st['strehl'][k] = abs(ph.sum()) ** 2 / ok.sum() ** 2
        return (torch.from_numpy(psf) if want_psf else None), st[None]


def numpy_calc_psf(wavefront, ndim, maxdim):
    """analyses.calc_psf's arithmetic (rayoptics/raytr/analyses.py:848-875) in NumPy"""
    h = maxdim // 2
    W = np.zeros([maxdim, maxdim])
    nd2 = ndim // 2
    W[h - (nd2 - 1):h + (nd2 + 1), h - (nd2 - 1):h + (nd2 + 1)] = np.nan_to_num(wavefront)
    phase = np.exp(1j * 2 * np.pi * W)
    phase[phase == 1] = 0
    AP = abs(np.fft.fftshift(np.fft.fft2(np.fft.fftshift(phase)))) ** 2
    return AP / np.nanmax(AP)


def test_result_assembled_from_an_engine_double(monkeypatch):
    pytest.importorskip('torch')
    import focus_fixture as FF
    from rayoptics_amd import analyses
    m = FF.FocusFixtureModel(FF.load(), 'dblgauss')
    focs = m.focs
    K, num, M = len(focs), 16, 40
    eng = _NumpyFocusEngine(num, K)
    seen = {}

    def setup(opt_model, fld, wvl, kw, out_mode):       # the double stands in for the device engine
        seen.update(kw=dict(kw), out_mode=out_mode)
        return eng, None, 0, None
    monkeypatch.setattr(analyses, '_launch_setup', setup)
    res = analyses.through_focus_psf(m, m.fields[0], m.wvl, focs, num_rays=num, maxdim=M)
    assert seen['out_mode'] == abi.OUT_FAN and seen['kw']['check_apertures'] is True
    convert = 1 / m.nm_to_sys_units(m.wvl)
    assert eng.calls[0] == ('trace', K, True, True)
    assert eng.calls[1][:3] == ('psf', num, M) and eng.calls[1][3] == convert and eng.calls[1][4] is True
    assert res.psf.shape == (K, M, M) and isinstance(res.psf, np.ndarray)
    assert np.array_equal(res.stats['opd_rms'], convert * np.arange(K))     # in waves, as through_focus
    assert res.strehl.shape == res.psf_peak.shape == res.n.shape == (K,)
    assert (res.best_focus_strehl, res.best_focus_strehl_kind) == analyses.best_focus(focs, -res.strehl)
    assert res.delta_x is None and res.delta_xp is None


@pytest.mark.parametrize('field', ['f0', 'f1'])
def test_scaling_per_focus_equals_the_references_calc_psf_scaling(monkeypatch, field):
    """delta_x / delta_xp of every focus against the reference's calc_psf_scaling stored in
    tests/golden/through_focus_psf.npz: each focus brings its own reference-sphere radius (the
    sphere moves with foc), and the arithmetic is the reference's, bit for bit"""
    pytest.importorskip('torch')
    import focus_psf_fixture as PF
    from rayoptics_amd import analyses
    m = PF.FocusPsfFixtureModel(PF.load(), field)
    K, ndim = len(m.focs), int(m.z['ndim'])
    assert len(set(m.z['ref_radius'])) == K
    eng = _NumpyFocusEngine(ndim, K)
    monkeypatch.setattr(analyses, '_launch_setup', lambda *a: (eng, None, 0, None))
    for j, M in enumerate(m.z['maxdims']):
        res = analyses.through_focus_psf(m, m.fields[0], m.wvl, m.focs, num_rays=ndim, maxdim=int(M), psf=False)
        assert res.psf is None
        assert np.array_equal(res.delta_x, m.z['psf_scaling'][:, j, 0])
        assert np.array_equal(res.delta_xp, m.z['psf_scaling'][:, j, 1])
