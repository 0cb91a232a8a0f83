"""rox_focus_gmtf on the device: the geometric OTF and line spread of through-focus rows against
the NumPy restatement (tests/gmtf_ref.py) -- the device's own rows of the double Gauss, the .zmx
zoom (exact and ROX_FAST_FP64) and the on-axis paraboloid, and the reference's own transverse
aberrations (tests/golden/through_focus_ee.npz) --, the sign and the centroid phase from a series
that does not use the restatement, edge cases, chunk boundaries, bit-identical repeats and
destinations, jobs split over several launches, exact histograms, argument errors and
analyses.through_focus_gmtf end to end.

The tolerance of every OTF comparison, per (re, im) entry (gmtf_ref.tol):

    tol = (n_ok + 8) 2^-52 + 2 pi nu max|u| 2^-51

Derivation.  The entry and the restatement form the same u (two products and a sum, no FMA), the
same t = fl(nu u) and the same r = t - rint(t), which is exact; so both sum the same n terms
cos(2 pi r), sin(2 pi r) up to the rounding of the sine and cosine themselves (below 2 ulp of a
value <= 1 each on either side: 4 of the 8 ulp, the rest for the division by n and the final
negation).  Any order of summing n terms of magnitude <= 1 has partial sums <= n, so n - 1
additions each round by at most n 2^-53 / n after the division by n: two different orders differ
by at most (n - 1) 2^-52 relative to the mean's scale 1.  That is the first term.  The second is
for comparisons against a value that did not round t the same way (an 80-bit or exp(-2 pi i nu u)
evaluation): one rounding of t = nu u is |t| 2^-53, a phase error 2 pi |t| 2^-53 <=
2 pi nu max|u| 2^-53, and a unit-modulus term moves by at most its phase error; the factor 4 covers
the rounding of 2 pi nu u in the other evaluation.  The bound is not fitted to the device's
output.

End to end the device rows are the reference's rays only to the agreement the earlier
through-focus tests pin (test_gpu_through_focus_ee: 1e-9 relative of the spot), so that test adds
the phase of such a displacement, 2 pi nu 1e-9 max|u|, to tol."""
import ctypes as C
import os

import numpy as np
import pytest

import gmtf_ref as GR
from rayoptics_amd import abi
from test_gpu_through_focus_ee import _Rows, _engine, device_rows, traced
from test_through_focus_gmtf_host import c_error_cases, call_gmtf

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FREQS = np.array([0.0, 1.0, 5.0, 10.0, 37.5, 100.0, 400.0])
DIRS = np.array([(1.0, 0.0), (0.0, 1.0), (0.6, 0.8), (np.cos(0.3), np.sin(0.3))])
LENSES = [('dblgauss_c2', False), ('zmx_evenasph_c3', False), ('zmx_evenasph_c3', True), ('tt_paraboloid', False)]


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


@pytest.fixture(scope='module')
def traced_rows(torch):
    """(name, fast) -> (engine, stats, FocusRows, host rows, host status, restatement): 6 items,
    64^2 rays, K = 5, traced and restated once per lens and left unchanged"""
    cache = {}

    def get(name, fast):
        if (name, fast) not in cache:
            eng, stats, fr = traced(name, 6, 64, fast=fast, seed=3, K=5)
            rows, status = fr.rows.cpu().numpy(), fr.status.cpu().numpy()
            ref = GR.focus_gmtf(rows, status, rows.shape[-1], DIRS, FREQS)
            cache[(name, fast)] = (eng, stats, fr, rows, status, ref)
        return cache[(name, fast)]

    yield get
    for entry in cache.values():
        entry[0].close()


@pytest.fixture(scope='module')
def random_rows(torch):
    """2 items x 2 planes, R = 5000 in rows of pitch 5120; every third ray failed (item 0 from ray
    2, item 1 from ray 0)"""
    rng = np.random.default_rng(11)
    rows = rng.normal(scale=0.02, size=(2, 2, 3, 5120))
    status = np.full((2, 5120), abi.OK, dtype=np.uint8)
    status[0, 2::3] = abi.BLOCKED
    status[1, ::3] = abi.MISSED_SURFACE
    full = device_rows(torch, rows, status)
    return _Rows(full.rows[..., :5000], full.status[:, :5000]), rows[..., :5000], status[:, :5000]


def same_bytes(a, b):
    return all((x is None and y is None) or x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- 1. traced rows --------------------------------------------------------------------------
@pytest.mark.parametrize('name,fast', LENSES)
def test_traced_rows_equal_the_restatement(torch, traced_rows, name, fast):
    eng, stats, fr, rows, status, (e_otf, _l, e_n, umax) = traced_rows(name, fast)
    R = rows.shape[-1]
    assert (status == abi.OK).sum() > 1000
    otf, lsf, n_ok = eng.focus_gmtf(fr, R, DIRS, FREQS)
    assert lsf is None and np.array_equal(n_ok, e_n)
    worst = GR.assert_otf_close(otf, e_otf, n_ok, FREQS, umax, f'{name} fast={fast}')
    print(f'{name} fast={fast}: largest error / tol = {worst:.3g}')
    lit = n_ok > 0
    assert lit.any() and (otf[lit][..., 0].real == 1.0).all() and (otf[lit][..., 0].imag == 0.0).all()
    assert not np.signbit(otf[lit][..., 0].imag).any()
    # the first R - 17 rays
    o2, _l, n2 = eng.focus_gmtf(fr, R - 17, DIRS, FREQS)
    e2, _l, en2, um2 = GR.focus_gmtf(rows, status, R - 17, DIRS, FREQS)
    assert np.array_equal(n2, en2)
    GR.assert_otf_close(o2, e2, n2, FREQS, um2, f'{name} fast={fast} first rays')
    # the rows of failed rays are never read: garbage there changes nothing
    K = rows.shape[1]
    full = torch.zeros(rows.shape[:3] + (int(fr.rows.stride(2)),), dtype=torch.float64, device='cuda')
    full[..., :R] = fr.rows                              # a copy at the same row pitch
    dirty = _Rows(full[..., :R], fr.status)
    bad = (fr.status != abi.OK)[:, None, None, :].expand(-1, K, 2, -1)
    dirty.rows[:, :, :2].masked_fill_(bad, 1e300)
    edges = np.linspace(-0.2, 0.2, 33)
    a = eng.focus_gmtf(fr, R, DIRS, FREQS, edges=edges)
    b = eng.focus_gmtf(dirty, R, DIRS, FREQS, edges=edges)
    assert same_bytes(a, b) and a[0].tobytes() == otf.tobytes()


# ---- 2. the reference's own rays -------------------------------------------------------------
def golden_rows():
    z = np.load(os.path.join(GOLDEN, 'through_focus_ee.npz'))
    a = z['dblgauss/abr']                                # [F, W, K, n, n, 2]
    F, W, K, n, _n, _two = a.shape
    rows = np.zeros((F * W, K, 3, n * n))
    rows[:, :, :2] = np.moveaxis(a.reshape(F * W, K, n * n, 2), -1, 2)
    bad = np.isnan(a[:, :, 0, ..., 0]).reshape(F * W, n * n)
    status = np.where(bad, abi.BLOCKED, abi.OK).astype(np.uint8)
    return np.where(bad[:, None, None], 0.0, rows), status


def test_the_reference_rays(torch):
    """the reference's transverse aberrations in HBM: within tol of mean(exp(-2 pi i nu u))"""
    rows, status = golden_rows()
    fr = device_rows(torch, rows, status)
    eng = _engine()
    otf, _l, n_ok = eng.focus_gmtf(fr, rows.shape[-1], DIRS, FREQS)
    exp = np.empty_like(otf)
    umax = np.empty(otf.shape[:3])
    for i in range(rows.shape[0]):
        ok = status[i] == abi.OK
        assert n_ok[i, 0] == ok.sum() and (n_ok[i] == n_ok[i, 0]).all()
        for k in range(rows.shape[1]):
            for d, (ex, ey) in enumerate(DIRS):
                u = ex * rows[i, k, 0] + ey * rows[i, k, 1]
                umax[i, k, d] = np.abs(u[ok]).max()
                for q, nu in enumerate(FREQS):
                    exp[i, k, d, q] = np.exp(-2j * np.pi * nu * u)[ok].mean()
    assert n_ok.min() > 500
    worst = GR.assert_otf_close(otf, exp, n_ok, FREQS, umax, 'reference rays')
    print(f'reference rays: largest error / tol = {worst:.3g}')
    eng.close()


# ---- 3. sign and centroid ----------------------------------------------------------------------
def test_sign_and_centroid_phase(torch, traced_rows):
    """independent of the restatement: with eps = 2 pi nu0 max|u - c| <= 1e-3 about the centroid c
    of the launch's own statistics, mean(exp(-i theta)) = exp(-i mean) (1 + O(eps^2)) and
    |arg(OTF) + 2 pi nu0 c| <= eps^3 / 6 / (1 - eps^2 / 2) + 1e-12"""
    eng, stats, fr, rows, status, _ref = traced_rows('dblgauss_c2', False)
    R = rows.shape[-1]
    n_items, K = stats.shape
    spread = np.zeros((n_items, K, 2))
    cen = np.nan_to_num(np.stack([stats['cx'], stats['cy']], axis=-1))
    lit = np.zeros((n_items, K), dtype=bool)
    for i in range(n_items):
        ok = status[i] == abi.OK
        lit[i] = ok.any()
        for k in range(K):
            for d in range(2):
                if ok.any():
                    spread[i, k, d] = np.abs(rows[i, k, d, ok] - cen[i, k, d]).max()
    nu0 = 1e-3 / (2 * np.pi * spread.max())
    otf, _l, n_ok = eng.focus_gmtf(fr, R, DIRS[:2], [nu0])
    eps = 2 * np.pi * nu0 * spread
    assert lit.sum() >= 20 and np.array_equal(n_ok > 0, lit) and eps.max() <= 1e-3 * (1 + 1e-15)
    err = np.abs(np.angle(otf[..., 0]) + 2 * np.pi * nu0 * cen)
    assert (err[lit] <= (eps ** 3 / 6 / (1 - eps ** 2 / 2) + 1e-12)[lit]).all()
    # the phases are not all below the bound by themselves: the centroid term is what is checked
    assert np.abs(np.angle(otf[..., 0][lit])).max() > 1e-9


# ---- 4. edge cases -------------------------------------------------------------------------------
def test_edge_cases(torch):
    eng = _engine()
    R, K = 300, 5
    rng = np.random.default_rng(7)
    rows = rng.normal(size=(3, K, 3, R))
    status = np.full((3, R), abi.OK, dtype=np.uint8)
    status[0] = abi.BLOCKED                              # item 0: no ray on any plane
    status[1] = abi.MISSED_SURFACE
    status[1, 123] = abi.OK                              # item 1: a single ray
    u0 = (0.25, -0.125)
    rows[2, 1, 0], rows[2, 1, 1] = u0                    # item 2 plane 1: every ray on one point
    fr = device_rows(torch, rows, status)
    dirs = np.array([(1.0, 0.0), (0.0, 1.0), (0.0, -1.0), (0.6, 0.8)])
    edges = np.linspace(-4.0, 4.0, 17)
    otf, lsf, n_ok = eng.focus_gmtf(fr, R, dirs, FREQS, edges=edges)
    e_otf, e_lsf, e_n, umax = GR.focus_gmtf(rows, status, R, dirs, FREQS, edges)
    assert np.array_equal(n_ok, e_n) and np.array_equal(lsf, e_lsf)
    GR.assert_otf_close(otf, e_otf, n_ok, FREQS, umax, 'edge cases')
    assert (n_ok[0] == 0).all() and np.isnan(otf[0].real).all() and np.isnan(otf[0].imag).all() and (lsf[0] == 0).all()
    assert (n_ok[1] == 1).all() and np.max(np.abs(np.abs(otf[1]) - 1.0)) <= 4 * 2.0 ** -52
    for d, (ex, ey) in enumerate(dirs):
        u = ex * u0[0] + ey * u0[1]
        exp = np.exp(-2j * np.pi * FREQS * u)
        t = GR.tol(R, FREQS, abs(u))
        assert (np.abs(otf[2, 1, d].real - exp.real) <= t).all() and (np.abs(otf[2, 1, d].imag - exp.imag) <= t).all()
    # (0, -1) against (0, 1): the conjugate, bit for bit
    lit = n_ok > 0
    up, down = otf[lit][:, 1], otf[lit][:, 2]
    assert np.abs(up).tobytes() == np.abs(down).tobytes()
    assert np.array_equal(up.real, down.real) and np.array_equal(up.imag, -down.imag)
    eng.close()


# ---- 5. chunk boundaries and determinism ---------------------------------------------------------
@pytest.mark.parametrize('n_rays', [1, 63, 64, 65, 2047, 2048, 2049, 4999, 5000])
def test_chunk_boundaries_and_determinism(torch, random_rows, n_rays):
    fr, rows, status = random_rows
    eng = _engine()
    edges = np.linspace(-0.1, 0.1, 41)
    a = eng.focus_gmtf(fr, n_rays, DIRS, FREQS, edges=edges)
    e_otf, e_lsf, e_n, umax = GR.focus_gmtf(rows, status, n_rays, DIRS, FREQS, edges)
    assert np.array_equal(a[2], e_n) and np.array_equal(a[1], e_lsf)
    GR.assert_otf_close(a[0], e_otf, e_n, FREQS, umax, f'n_rays {n_rays}')
    b = eng.focus_gmtf(fr, n_rays, DIRS, FREQS, edges=edges)
    d = eng.focus_gmtf(fr, n_rays, DIRS, FREQS, edges=edges, on_device=True)
    assert same_bytes(a, b)
    assert same_bytes(a, [x.cpu().numpy() for x in d])
    eng.close()


# ---- 6. consecutive launches -------------------------------------------------------------------
def seeded_entries_close(eng, rows_t, status_t, R, dirs, freqs, otf_t, n_entries, seed, what):
    rng = np.random.default_rng(seed)
    n_items, K = rows_t.shape[:2]
    for _ in range(n_entries):
        i, k, d, q = (int(rng.integers(n)) for n in (n_items, K, len(dirs), len(freqs)))
        x, y = rows_t[i, k, 0, :R].cpu().numpy(), rows_t[i, k, 1, :R].cpu().numpy()
        ok = status_t[i, :R].cpu().numpy() == abi.OK
        u = GR.project(dirs[d][0], dirs[d][1], x[ok], y[ok])
        exp = GR.otf_of(u, [freqs[q]])[0]
        got = complex(otf_t[i, k, d, q].cpu())
        t = GR.tol(ok.sum(), [freqs[q]], np.abs(u).max())[0]
        assert abs(got.real - exp.real) <= t and abs(got.imag - exp.imag) <= t, (what, i, k, d, q)


def test_consecutive_launches_over_planes(torch):
    """8 items x 256 planes x 2100 rays (two ray chunks), 8 directions and 1024 frequencies: the
    partial records of all planes take 2048 x 2 x 128 KiB = 512 MiB, four times the scratch of a
    launch.  The bytes equal those of 8 one-item calls; 16 seeded entries against the restatement"""
    eng = _engine()
    n_items, K, R, ld = 8, 256, 2100, 2112
    g = torch.Generator(device='cuda').manual_seed(5)
    rows = torch.randn((n_items, K, 3, ld), dtype=torch.float64, device='cuda', generator=g) * 0.01
    status = torch.full((n_items, ld), abi.OK, dtype=torch.uint8, device='cuda')
    status[:, ::29] = abi.BLOCKED
    th = np.linspace(0.0, np.pi, 8, endpoint=False)
    dirs = np.stack([np.cos(th), np.sin(th)], axis=-1)
    freqs = np.linspace(0.0, 400.0, 1024)
    fr = _Rows(rows[..., :R], status[:, :R])
    otf, _l, n_ok = eng.focus_gmtf(fr, R, dirs, freqs, on_device=True)
    for i in range(n_items):
        one, _l, n1 = eng.focus_gmtf(_Rows(rows[i:i + 1, ..., :R], status[i:i + 1, :R]), R, dirs, freqs, on_device=True)
        assert torch.equal(torch.view_as_real(one), torch.view_as_real(otf[i:i + 1])) and torch.equal(n1, n_ok[i:i + 1])
    seeded_entries_close(eng, rows, status, R, dirs, freqs, otf, 16, 9, 'planes')
    eng.close()


def test_consecutive_launches_over_frequencies(torch):
    """one plane of 2 200 000 rays (1075 ray chunks), 8 directions and 1024 frequencies: the
    plane's records of every frequency take 134 MiB, more than half a launch's scratch, so the
    frequencies run in groups.  The bytes equal those of four 256-frequency calls"""
    eng = _engine()
    R = 2_200_000
    g = torch.Generator(device='cuda').manual_seed(6)
    rows = torch.randn((1, 1, 3, R), dtype=torch.float64, device='cuda', generator=g) * 0.01
    status = torch.full((1, R), abi.OK, dtype=torch.uint8, device='cuda')
    status[:, ::7] = abi.BLOCKED
    th = np.linspace(0.0, np.pi, 8, endpoint=False)
    dirs = np.stack([np.cos(th), np.sin(th)], axis=-1)
    freqs = np.linspace(0.0, 400.0, 1024)
    fr = _Rows(rows, status)
    otf, _l, n_ok = eng.focus_gmtf(fr, R, dirs, freqs, on_device=True)
    for q0 in range(0, 1024, 256):
        part, _l, n1 = eng.focus_gmtf(fr, R, dirs, freqs[q0:q0 + 256], on_device=True)
        assert torch.equal(torch.view_as_real(part), torch.view_as_real(otf[..., q0:q0 + 256])) and torch.equal(n1, n_ok)
    seeded_entries_close(eng, rows, status, R, dirs, freqs, otf, 16, 10, 'frequencies')
    eng.close()


# ---- 7. the line spread ------------------------------------------------------------------------
def spot_edges(rows, status, n_rays, dirs, B, seed):
    """strictly increasing random edges per (item, plane, direction) across each projected spot:
    one inner edge exactly on a ray and the last edge exactly on the largest u"""
    rng = np.random.default_rng(seed)
    n_items, K = rows.shape[:2]
    out = np.empty((n_items, K, len(dirs), B + 1))
    for i in range(n_items):
        ok = status[i, :n_rays] == abi.OK
        for k in range(K):
            for d, (ex, ey) in enumerate(dirs):
                u = np.unique(GR.project(ex, ey, rows[i, k, 0, :n_rays][ok], rows[i, k, 1, :n_rays][ok]))
                if u.size < 3:
                    out[i, k, d] = np.linspace(-1.0, 1.0, B + 1)
                    continue
                lo, hi = u[0] + 0.1 * (u[-1] - u[0]), u[-1]
                on_ray = u[u.size // 2]
                out[i, k, d] = np.linspace(-1.0, 1.0, B + 1)     # (kept for a spot a few ulp wide)
                for _ in range(20):
                    e = np.sort(np.concatenate([[lo, on_ray, hi], rng.uniform(lo, hi, B - 2)]))
                    if (np.diff(e) > 0).all():
                        out[i, k, d] = e
                        break
    return out


def check_lsf(eng, fr, rows, status, n_rays, what):
    from rayoptics_amd import analyses
    dirs = DIRS[:3]
    n_items, K = rows.shape[:2]
    rnd = spot_edges(rows, status, n_rays, dirs, 37, seed=4)
    _o, _l, _n, umax = GR.focus_gmtf(rows, status, n_rays, dirs, None)
    lin = analyses.lsf_edges(np.zeros((n_items, K, 3)), np.maximum(0.7 * umax, 1e-6), 64)
    for edges in (rnd, lin):
        otf, lsf, n_ok = eng.focus_gmtf(fr, n_rays, dirs, FREQS, edges=edges)
        _e, e_lsf, e_n, _u = GR.focus_gmtf(rows, status, n_rays, dirs, None, edges)
        assert np.array_equal(lsf, e_lsf) and np.array_equal(n_ok, e_n), what
        assert lsf.dtype == np.int64 and 0 < lsf.sum() <= n_ok.sum() * 3
        only_l = eng.focus_gmtf(fr, n_rays, dirs, None, edges=edges)
        only_o = eng.focus_gmtf(fr, n_rays, dirs, FREQS)
        assert only_l[0] is None and only_o[1] is None
        assert same_bytes((lsf, n_ok), only_l[1:]) and same_bytes((otf, n_ok), (only_o[0], only_o[2])), what


@pytest.mark.parametrize('name,fast', LENSES)
def test_lsf_is_numpy_histogram_on_traced_rows(torch, traced_rows, name, fast):
    eng, _stats, fr, rows, status, _ref = traced_rows(name, fast)
    check_lsf(eng, fr, rows, status, rows.shape[-1], f'{name} fast={fast}')


@pytest.mark.parametrize('n_rays', [65, 5000])
def test_lsf_is_numpy_histogram_on_random_rows(torch, random_rows, n_rays):
    fr, rows, status = random_rows
    eng = _engine()
    check_lsf(eng, fr, rows, status, n_rays, f'random rows, n_rays {n_rays}')
    eng.close()


def test_lsf_limits(torch, random_rows):
    """4096 bins and 8 directions, the largest histogram of a call"""
    fr, rows, status = random_rows
    eng = _engine()
    th = np.linspace(0.0, np.pi, 8, endpoint=False)
    dirs = np.stack([np.cos(th), np.sin(th)], axis=-1)
    edges = np.linspace(-0.05, 0.05, abi.MAX_LSF_BINS + 1)
    _o, lsf, n_ok = eng.focus_gmtf(fr, 5000, dirs, None, edges=edges)
    _e, e_lsf, e_n, _u = GR.focus_gmtf(rows, status, 5000, dirs, None, edges)
    assert np.array_equal(lsf, e_lsf) and np.array_equal(n_ok, e_n)
    eng.close()


# ---- 8. argument errors ------------------------------------------------------------------------
def test_argument_errors_enqueue_nothing(torch, lib, random_rows):
    """every limit returns ROX_E_ARG with the parameter's name, and device outputs keep their
    bytes; the same arguments without the error run"""
    fr, _rows, _status = random_rows
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    otf = torch.full((2, 3, 2, 3, 2), -7.0, dtype=torch.float64, device='cuda')
    lsf = torch.full((2, 3, 2, 4), -7, dtype=torch.int64, device='cuda')
    n_ok = torch.full((2, 3), -7, dtype=torch.int64, device='cuda')
    rows = torch.zeros((2, 3, 3, 320), dtype=torch.float64, device='cuda')
    status = torch.zeros((2, 320), dtype=torch.uint8, device='cuda')
    outs = (otf.data_ptr(), lsf.data_ptr(), n_ok.data_ptr())
    for name, over, word in c_error_cases():
        rc = call_gmtf(lib, dict(over), rows.data_ptr(), status.data_ptr(), outs, st)
        msg = lib.rox_last_error().decode()
        assert rc == -1 and msg.startswith('rox_focus_gmtf: ') and word in msg, (name, rc, msg)
    torch.cuda.synchronize()
    assert (otf == -7.0).all() and (lsf == -7).all() and (n_ok == -7).all()
    assert call_gmtf(lib, {}, rows.data_ptr(), status.data_ptr(), outs, st) == 0
    torch.cuda.synchronize()
    assert (n_ok == 300).all() and (otf[..., 0] == 1.0).all() and (otf[..., 1] == 0.0).all()
    assert (lsf.sum(dim=-1) == 300).all() and (lsf[..., 2] == 300).all()     # u = 0: the bin [0, 0.5)


# ---- 9. end to end -----------------------------------------------------------------------------
def test_through_focus_gmtf_double_gauss_against_the_reference(torch):
    import focus_map_fixture as FM
    from rayoptics_amd import analyses
    z = np.load(os.path.join(GOLDEN, 'through_focus_ee.npz'))
    m = FM.FocusMapFixtureModel(z, 'dblgauss')
    a = m.z['abr']                                       # [F, W, K, n, n, 2]
    F, W, K, n = a.shape[:4]
    res = analyses.through_focus_gmtf(m, m.focs, FREQS, num_rays=n, lsf_bins=32, **m.map_kwargs())
    D, Q = 4, FREQS.size
    assert res.directions == ['x', 'y', 't', 's'] and res.otf.shape == (F, W, K, D, Q)
    ref = m.wvls.index(m.central_wvl)
    ip = m.z['image_pt'][:, ref, 1]
    assert np.array_equal(res.dirs[0], [(1, 0), (0, 1), (0, 1), (1, 0)])               # the axial field
    t = ip[1] / np.hypot(*ip[1])
    assert np.array_equal(res.dirs[1, 2], t) and np.array_equal(res.dirs[1, 3], (t[1], -t[0])) and t[0] > 0.5
    for f in range(F):
        for w in range(W):
            for k in range(K):
                x, y = a[f, w, k, ..., 0].reshape(-1), a[f, w, k, ..., 1].reshape(-1)
                ok = ~np.isnan(x)
                assert res.n_ok[f, w, k] == ok.sum()
                for d in range(D):
                    u = GR.project(res.dirs[f, d, 0], res.dirs[f, d, 1], x[ok], y[ok])
                    exp = GR.otf_of(u, FREQS)
                    um = np.abs(u).max()
                    tol = GR.tol(ok.sum(), FREQS, um) + 2 * np.pi * FREQS * 1e-9 * um
                    got = res.otf[f, w, k, d]
                    assert (np.abs(got.real - exp.real) <= tol).all() and (np.abs(got.imag - exp.imag) <= tol).all()
    for f in range(F):
        merged = analyses.poly_otf_merge(res.otf[f], res.image_pts[f], m.spectral_wts, ref, FREQS, dirs=res.dirs[f])
        assert merged.tobytes() == res.poly_otf[f].tobytes()
    # the axial field: tangential is y and sagittal is x; the oblique field has both, finite
    assert res.tangential[0].tobytes() == np.ascontiguousarray(res.poly_mtf[0, :, 1]).tobytes()
    assert res.sagittal[0].tobytes() == np.ascontiguousarray(res.poly_mtf[0, :, 0]).tobytes()
    assert np.isfinite(res.tangential[1]).all() and np.isfinite(res.sagittal[1]).all()
    assert res.best_focus.shape == (F, D, Q) and res.best_focus_all.shape == (Q,)
    assert (res.poly_mtf[..., 0] == 1.0).all() and (res.poly_mtf <= 1.0 + 1e-12).all()
    # the line spread: the rays inside +- 3 RMS about the polychromatic centroid.  Chebyshev's
    # inequality leaves at most 1/9 outside for the mixture the RMS weights (s_w n_w); poly_lsf
    # weights s_w, and the ray counts of a field's wavelengths differ by under 3 %: 1 - 1.03 / 9
    assert res.lsf.shape == (F, W, K, D, 32) and res.lsf_edges.shape == (F, K, D, 33)
    assert (res.lsf.sum(axis=-1) <= res.n_ok[..., None]).all()
    assert (res.lsf_inside >= 0.885).all() and (res.lsf_inside <= 1 + 1e-15).all()
    assert np.array_equal(res.esf[..., -1], np.cumsum(res.poly_lsf, axis=-1)[..., -1])
    # given half widths, one per field, along one direction
    one = analyses.through_focus_gmtf(m, m.focs, FREQS[:2], num_rays=n, directions=('t',), lsf_bins=8,
                                      lsf_half_width=[0.1, 0.2], **m.map_kwargs())
    assert one.lsf.shape == (F, W, K, 1, 8) and one.sagittal is None
    assert one.otf.tobytes() == np.ascontiguousarray(res.otf[..., 2:3, :2]).tobytes()
    width = one.lsf_edges[..., -1] - one.lsf_edges[..., 0]
    assert np.max(np.abs(width[0] - 0.2)) <= 1e-15 and np.max(np.abs(width[1] - 0.4)) <= 1e-15
    assert np.max(np.abs(one.lsf_edges[..., 4] - res.lsf_edges[:, :, 2:3, 16])) <= 1e-15      # the same centre
