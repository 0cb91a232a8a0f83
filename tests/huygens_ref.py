"""TEST INFRASTRUCTURE: the NumPy restatement of rox_huygens_psf (include/roxtrace.h,
ray-optics_amd/csrc/huygens.hip).  It forms the operands with the header's arithmetic -- every
product and sum one IEEE rounding, summed left to right, the arguments reduced by r = t - rint(t)
-- and then takes a plain complex sum over the rays, in whatever order NumPy's matrix product
uses.  The device differs from it by the order of that sum and by the last bits of sincospi; the
tests bound both.

The sine and cosine of 2 pi r are taken in long double where the platform has one wider than
double (x86: 64-bit mantissa), so that the restatement's operands are the correctly rounded ones
to well under one ulp."""
import numpy as np

OK = 0
_LD = np.longdouble
_TWO_PI = 2 * np.arccos(_LD(-1.0))


def wavelet(t):
    """(cos, sin)(2 pi t) with the argument reduced as the kernel reduces it"""
    r = t - np.rint(t)                                   # exact: |r| <= 1/2
    x = _TWO_PI * r.astype(_LD)
    return np.cos(x).astype(np.float64), np.sin(x).astype(np.float64)


def operands(rows, amp, status, planes, nx, ny, pitch_x, pitch_y, n_rays=None):
    """one item: rows [4, ld], amp [ld] or None, status [ld], planes [K, 3] ->
    A [K, nx, R] and B [ny, R] complex128, a failed ray a zero column, and the amplitudes [R] with
    zeros at failed rays"""
    rows = np.asarray(rows, dtype=np.float64)
    R = rows.shape[1] if n_rays is None else int(n_rays)
    phi, xi, eta, zeta = (rows[c, :R] for c in range(4))
    ok = np.asarray(status)[:R] == OK
    a = np.ones(R) if amp is None else np.asarray(amp, dtype=np.float64)[:R]
    planes = np.asarray(planes, dtype=np.float64).reshape(-1, 3)
    safe = [np.where(ok, v, 0.0) for v in (phi, xi, eta, zeta)]      # a failed ray's rows are never read
    phi, xi, eta, zeta = safe
    xg = np.arange(nx, dtype=np.float64) * pitch_x                   # a * pitch_x: one rounding
    yg = np.arange(ny, dtype=np.float64) * pitch_y
    A = np.zeros((planes.shape[0], nx, R), dtype=np.complex128)
    for k, (x0, y0, dz) in enumerate(planes):
        t = phi + zeta * dz
        t = t + xi * x0
        t = t + eta * y0
        t = t[None, :] + xi[None, :] * xg[:, None]
        c, s = wavelet(t)
        A[k] = np.where(ok, a * c, 0.0) + 1j * np.where(ok, a * s, 0.0)
    c, s = wavelet(eta[None, :] * yg[:, None])
    B = np.where(ok, c, 0.0) + 1j * np.where(ok, s, 0.0)
    return A, B, np.where(ok, a, 0.0)


def origin_pixel(x0, pitch, n):
    return int(min(max(np.rint(-x0 / pitch), 0.0), n - 1.0))


def huygens_psf(rows, amp, status, planes, nx, ny, pitch_x, pitch_y, n_rays=None):
    """every item: rows [n_items, 4, ld], amp [n_items, ld] or None, status [n_items, ld], planes
    [n_items, K, 3] -> (U [n_items, K, nx, ny] complex128, psf, stats), stats a dict of [n_items, K]
    arrays n, norm, sum, peak, strehl, peak_ix, peak_iy, and sum_abs [n_items] = sum |a_r| over the
    OK rays (what the error bounds scale with)"""
    rows = np.asarray(rows, dtype=np.float64)
    planes = np.asarray(planes, dtype=np.float64)
    n_items, K = planes.shape[0], planes.shape[1]
    U = np.zeros((n_items, K, nx, ny), dtype=np.complex128)
    st = {k: np.full((n_items, K), np.nan) for k in ('norm', 'sum', 'peak', 'strehl')}
    st.update({k: np.full((n_items, K), -1, dtype=np.int64) for k in ('peak_ix', 'peak_iy')})
    st['n'] = np.zeros((n_items, K), dtype=np.int64)
    st['sum_abs'] = np.zeros(n_items)
    for i in range(n_items):
        A, B, a = operands(rows[i], None if amp is None else amp[i], status[i], planes[i], nx, ny, pitch_x, pitch_y,
                           n_rays)
        U[i] = A @ B.T
        n = int(np.count_nonzero(np.asarray(status[i])[:a.shape[0]] == OK))
        st['n'][i] = n
        st['sum_abs'][i] = np.abs(a).sum()
        if n == 0:
            continue
        for k in range(K):
            p = U[i, k].real ** 2 + U[i, k].imag ** 2
            at = int(np.argmax(p))                                   # the first of equal maxima
            st['norm'][i, k] = a.sum() ** 2
            st['sum'][i, k] = p.sum()
            st['peak'][i, k] = p.flat[at]
            st['peak_ix'][i, k], st['peak_iy'][i, k] = at // ny, at % ny
            a0 = origin_pixel(planes[i, k, 0], pitch_x, nx)
            b0 = origin_pixel(planes[i, k, 1], pitch_y, ny)
            st['strehl'][i, k] = p[a0, b0] / st['norm'][i, k]
    psf = U.real ** 2 + U.imag ** 2
    return U, psf, st


def direct_sum(rows, amp, status, plane, nx, ny, pitch_x, pitch_y):
    """one item, one plane, without the factorisation: U[a][b] = sum_r a_r exp(2 pi i (phi + zeta dz +
    xi X_a + eta Y_b)) in long double -- the physics the factorised sum must equal to rounding"""
    rows = np.asarray(rows, dtype=np.float64)
    ok = np.asarray(status) == OK
    phi, xi, eta, zeta = (rows[c][ok].astype(_LD) for c in range(4))
    a = (np.ones(rows.shape[1]) if amp is None else np.asarray(amp, dtype=np.float64))[ok].astype(_LD)
    x0, y0, dz = (_LD(v) for v in plane)
    X = x0 + np.arange(nx).astype(_LD) * _LD(pitch_x)
    Y = y0 + np.arange(ny).astype(_LD) * _LD(pitch_y)
    t = (phi + zeta * dz)[None, None, :] + xi[None, None, :] * X[:, None, None] + eta[None, None, :] * Y[None, :, None]
    t = t - np.rint(t)
    return ((a * np.cos(_TWO_PI * t)).sum(axis=-1).astype(np.float64)
            + 1j * (a * np.sin(_TWO_PI * t)).sum(axis=-1).astype(np.float64))
