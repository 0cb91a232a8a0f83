"""TEST INFRASTRUCTURE: a NumPy restatement of rox_focus_zernike (include/roxtrace.h) -- the pupil
axes by repeated +=, the selection rule, the Zernike basis and a least-squares fit per plane by
numpy.linalg.lstsq (SVD), not by the normal equations."""
import math

import numpy as np

OK = 0


def axes(start, stop, num):
    """the pupil axis x and y of a PRODUCT grid, each by repeated += of (stop - start)/(num - 1)"""
    out = []
    for d in range(2):
        step = (stop[d] - start[d]) / (num - 1)
        v, a = start[d], np.empty(num)
        for k in range(num):
            a[k] = v
            v += step
        out.append(a)
    return out


def select(status, px, py, circle=(0.0, 0.0, 1.0)):
    """ray r = a num + b at (px[a], py[b]) -> (fit, outside, x, y) over the rays, normalised to
    the circle; fit: status OK and x*x + y*y <= 1; outside: OK and not inside"""
    cx, cy, rad = circle
    X, Y = np.meshgrid(px, py, indexing='ij')
    x = ((X - cx) / rad).reshape(-1)
    y = ((Y - cy) / rad).reshape(-1)
    ok = np.asarray(status)[:x.size] == OK
    inside = x * x + y * y <= 1.0
    return ok & inside, ok & ~inside, x, y


def radial(n, m, rho):
    m = abs(m)
    out = np.zeros_like(rho)
    for k in range((n - m) // 2 + 1):
        c = (-1) ** k * math.factorial(n - k) // (math.factorial(k) * math.factorial((n + m) // 2 - k)
                                                 * math.factorial((n - m) // 2 - k))
        out = out + c * rho ** (n - 2 * k)
    return out


def basis(terms, x, y):
    """[R, J]: scale R_n^|m|(rho) {1 | cos m theta | sin |m| theta} with rho, theta from (x, y)"""
    rho = np.hypot(x, y)
    th = np.arctan2(y, x)
    cols = []
    for t in terms:
        n, m = int(t[0]), int(t[1])
        s = float(t[2]) if len(t) > 2 else 1.0
        ang = 1.0 if m == 0 else (np.cos(m * th) if m > 0 else np.sin(-m * th))
        cols.append(s * radial(n, m, rho) * ang)
    return np.stack(cols, axis=-1)


def fit_plane(W, Z):
    """(coef, rms, rms_residual, pv_residual) of one plane: W [n] waves, Z [n, J]"""
    n, J = Z.shape
    if n < J or n == 0:
        return np.full(J, np.nan), (np.sqrt(((W - W.mean()) ** 2).mean()) if n else np.nan), np.nan, np.nan
    c = np.linalg.lstsq(Z, W, rcond=None)[0]
    r = W - Z @ c
    return c, np.sqrt(((W - W.mean()) ** 2).mean()), np.sqrt((r * r).mean()), r.max() - r.min()


def focus_zernike(rows, status, grids, terms, wave_scale, circle=None):
    """rows [n_items, K, 3, >= R], status [n_items, >= R], grids [(start, stop, num)] per item ->
    (coef [n_items, K, J], dict of [n_items, K] arrays n, n_outside, rms, rms_residual,
    pv_residual)"""
    n_items, K = rows.shape[:2]
    J = len(terms)
    coef = np.empty((n_items, K, J))
    st = {k: np.empty((n_items, K)) for k in ('rms', 'rms_residual', 'pv_residual')}
    st['n'] = np.empty((n_items, K), dtype=np.int64)
    st['n_outside'] = np.empty((n_items, K), dtype=np.int64)
    for i in range(n_items):
        start, stop, num = grids[i]
        px, py = axes(start, stop, num)
        c = (0.0, 0.0, 1.0) if circle is None else tuple(circle[i])
        fit, out, x, y = select(status[i], px, py, c)
        Z = basis(terms, x[fit], y[fit])
        for k in range(K):
            W = wave_scale[i] * rows[i, k, 2, :num * num][fit]
            coef[i, k], st['rms'][i, k], st['rms_residual'][i, k], st['pv_residual'][i, k] = fit_plane(W, Z)
            st['n'][i, k], st['n_outside'][i, k] = int(fit.sum()), int(out.sum())
    return coef, st
