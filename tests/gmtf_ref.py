"""TEST INFRASTRUCTURE for the geometric-MTF-through-focus tests: include/roxtrace.h's
rox_focus_gmtf restated in NumPy.

Over the OK rays of a plane and per direction (ex, ey): u = ex*x + ey*y (two products and one sum,
each one IEEE binary64 operation: NumPy does not contract).  OTF(nu) = mean exp(-2 pi i nu u) with
the entry's steps: t = nu*u, r = t - rint(t) (exact), then cos(2 pi r) and sin(2 pi r); re = mean
cos, im = -mean sin; NaN where no ray is OK.  lsf = numpy.histogram(u, edges)[0].

tol() is the bound every OTF comparison of the tests uses; its derivation is in
tests/test_gpu_through_focus_gmtf.py."""
import numpy as np

OK = 0              # ROX_OK


def project(ex, ey, x, y):
    return np.add(np.multiply(np.float64(ex), x), np.multiply(np.float64(ey), y))


def otf_of(u, freqs):
    """u [n] -> complex [Q]: the restated steps, summed by numpy (pairwise)"""
    nu = np.asarray(freqs, dtype=np.float64).reshape(-1)
    u = np.asarray(u, dtype=np.float64).reshape(-1)
    if u.size == 0:
        return np.full(nu.size, np.nan + 1j * np.nan)
    t = np.multiply(nu[:, None], u[None, :])
    r = np.subtract(t, np.rint(t))
    ang = 2.0 * np.pi * r
    n = np.float64(u.size)
    return np.cos(ang).sum(axis=1) / n + 1j * (-(np.sin(ang).sum(axis=1)) / n + 0.0)


def tol(n_ok, freqs, umax):
    """(n_ok + 8) 2^-52 + 2 pi nu max|u| 2^-51 per (re, im) entry, [Q]"""
    nu = np.asarray(freqs, dtype=np.float64).reshape(-1)
    return (float(n_ok) + 8.0) * 2.0 ** -52 + 2.0 * np.pi * nu * float(umax) * 2.0 ** -51


def plane_gmtf(x, y, ok, dirs, freqs, edges=None):
    """one plane: x, y, ok [R]; dirs [D, 2]; edges [D, B + 1] or None ->
    (otf [D, Q] complex, lsf [D, B] int64 or None, n, umax [D])"""
    ok = np.asarray(ok, dtype=bool)
    x = np.asarray(x, dtype=np.float64)[ok]
    y = np.asarray(y, dtype=np.float64)[ok]
    dirs = np.asarray(dirs, dtype=np.float64).reshape(-1, 2)
    nu = np.asarray(freqs, dtype=np.float64).reshape(-1) if freqs is not None else np.empty(0)
    otf = np.empty((dirs.shape[0], nu.size), dtype=np.complex128)
    umax = np.zeros(dirs.shape[0])
    lsf = None if edges is None else np.empty((dirs.shape[0], np.asarray(edges).shape[-1] - 1), dtype=np.int64)
    for d, (ex, ey) in enumerate(dirs):
        u = project(ex, ey, x, y)
        otf[d] = otf_of(u, nu)
        umax[d] = np.abs(u).max() if u.size else 0.0
        if lsf is not None:
            lsf[d] = np.histogram(u, np.asarray(edges, dtype=np.float64)[d])[0]
    return otf, lsf, int(x.size), umax


def focus_gmtf(rows, status, n_rays, dirs, freqs, edges=None):
    """rows [n_items, K, 3, >= n_rays], status [n_items, >= n_rays]; dirs broadcast to
    [n_items, D, 2]; edges broadcast to [n_items, K, D, B + 1] or None ->
    (otf [n_items, K, D, Q], lsf or None, n_ok [n_items, K], umax [n_items, K, D])"""
    rows = np.asarray(rows, dtype=np.float64)
    n_items, K = rows.shape[:2]
    dirs = np.asarray(dirs, dtype=np.float64)
    D = dirs.shape[-2] if dirs.ndim > 1 else 1
    dirs = np.broadcast_to(dirs, (n_items, D, 2))
    nu = np.asarray(freqs, dtype=np.float64).reshape(-1) if freqs is not None else np.empty(0)
    if edges is not None:
        edges = np.asarray(edges, dtype=np.float64)
        edges = np.broadcast_to(edges, (n_items, K, D, edges.shape[-1]))
    otf = np.empty((n_items, K, D, nu.size), dtype=np.complex128)
    lsf = None if edges is None else np.empty((n_items, K, D, edges.shape[-1] - 1), dtype=np.int64)
    n_ok = np.empty((n_items, K), dtype=np.int64)
    umax = np.empty((n_items, K, D))
    for i in range(n_items):
        ok = np.asarray(status[i][:n_rays]) == OK
        for k in range(K):
            o, l, n, um = plane_gmtf(rows[i, k, 0, :n_rays], rows[i, k, 1, :n_rays], ok, dirs[i], nu,
                                     None if edges is None else edges[i, k])
            otf[i, k], n_ok[i, k], umax[i, k] = o, n, um
            if lsf is not None:
                lsf[i, k] = l
    return otf, lsf, n_ok, umax


def assert_otf_close(got, exp, n_ok, freqs, umax, what=''):
    """got, exp [n_items, K, D, Q]; n_ok [n_items, K]; umax [n_items, K, D]: every (re, im) entry
    within tol(), NaN where and only where n_ok == 0.  Returns the largest error / tol."""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, what
    nu = np.asarray(freqs, dtype=np.float64).reshape(-1)
    worst = 0.0
    for i in range(got.shape[0]):
        for k in range(got.shape[1]):
            if n_ok[i, k] == 0:
                assert np.isnan(got[i, k].real).all() and np.isnan(got[i, k].imag).all(), (what, i, k)
                continue
            for d in range(got.shape[2]):
                t = tol(n_ok[i, k], nu, umax[i, k, d])
                err = np.maximum(np.abs(got[i, k, d].real - exp[i, k, d].real),
                                 np.abs(got[i, k, d].imag - exp[i, k, d].imag))
                assert not np.isnan(err).any(), (what, i, k, d)
                worst = max(worst, float((err / t).max()))
                assert (err <= t).all(), (what, i, k, d, err, t)
    return worst
