"""TEST INFRASTRUCTURE for the encircled-energy-through-focus tests: include/roxtrace.h's
rox_focus_ee and rox_focus_psf_ee restated in NumPy, and the polychromatic merges of
analyses.through_focus_ee.

Geometric: over the OK rays of a plane, dx = x - cx, dy = y - cy, d2 = dx*dx + dy*dy (each one
IEEE binary64 operation: NumPy does not contract), counts[j] = #(d2 <= r_j * r_j) and
ee_radius[q] = sqrt(D(m)), D the sorted d2, m = clamp(ceil(f_q * n), 1, n); NaN where n == 0.

Diffraction: pixel (j, l) of an M x M PSF sits at (X, Y) = (-p (j - M/2), -p (l - M/2)) (the
orientation of rox_focus_mtf, tests/line_otf.py); ee(r) = sum of the PSF over the pixels whose
centre has d2 <= r * r, over the sum of the whole PSF; NaN where that sum is not positive and
finite.  The centre is given or the PSF's centroid, sum(X PSF) / sum(PSF) and likewise for Y."""
import numpy as np

OK = 0              # ROX_OK


def d2_of(x, y, cx, cy):
    dx = np.subtract(x, cx)
    dy = np.subtract(y, cy)
    return np.add(np.multiply(dx, dx), np.multiply(dy, dy))


def rank_of(fraction, n):
    """m = clamp(ceil(fraction * n), 1, n) with the product one IEEE product"""
    m = np.ceil(np.multiply(np.float64(fraction), np.float64(n)))
    return int(min(max(m, 1.0), float(n)))


def plane_ee(x, y, ok, center, radii, fractions):
    """one plane: x, y, ok [R] -> (counts [Nr] int64, ee_radius [Nf], n)"""
    ok = np.asarray(ok, dtype=bool)
    cx, cy = (0.0, 0.0) if center is None else (float(center[0]), float(center[1]))
    d2 = d2_of(np.asarray(x, dtype=np.float64)[ok], np.asarray(y, dtype=np.float64)[ok], cx, cy)
    n = int(d2.size)
    r = np.asarray(radii, dtype=np.float64).reshape(-1)
    counts = np.array([int(np.count_nonzero(d2 <= np.multiply(rj, rj))) for rj in r], dtype=np.int64)
    # non-negative doubles order as their bit patterns (NaN, never on an OK ray, last)
    srt = np.sort(d2.view(np.uint64)).view(np.float64)
    f = np.asarray(fractions, dtype=np.float64).reshape(-1)
    rad = np.full(f.size, np.nan)
    if n:
        rad = np.array([np.sqrt(srt[rank_of(fq, n) - 1]) for fq in f])
    return counts, rad, n


def focus_ee(rows, status, n_rays, centers, radii, fractions):
    """rows [n_items, K, 3, >= n_rays], status [n_items, >= n_rays]; centers [n_items, K, 2] or
    None; radii broadcast to [n_items, K, Nr]; fractions [Nf] -> (counts, ee_radius, n_ok)"""
    rows = np.asarray(rows, dtype=np.float64)
    n_items, K = rows.shape[:2]
    r = np.asarray(radii, dtype=np.float64)
    r = np.broadcast_to(r, (n_items, K, r.shape[-1] if r.ndim else 1))
    f = np.asarray(fractions, dtype=np.float64).reshape(-1)
    counts = np.empty(r.shape, dtype=np.int64)
    rad = np.empty((n_items, K, f.size))
    n_ok = np.empty((n_items, K), dtype=np.int64)
    for i in range(n_items):
        ok = np.asarray(status[i][:n_rays]) == OK
        for k in range(K):
            c = None if centers is None else centers[i][k]
            counts[i, k], rad[i, k], n_ok[i, k] = plane_ee(rows[i, k, 0, :n_rays], rows[i, k, 1, :n_rays], ok, c,
                                                           r[i, k], f)
    return counts, rad, n_ok


def pixel_coords(M, pitch):
    """[M] image coordinate of pixel index j along either axis: -p (j - M/2)"""
    return -(np.float64(pitch) * (np.arange(M) - M // 2).astype(np.float64))


def psf_centroid(psf, pitch):
    """[2] (X, Y) centroid of one PSF; NaN where its sum is not positive and finite"""
    psf = np.asarray(psf, dtype=np.float64)
    X = pixel_coords(psf.shape[0], pitch)
    tot = psf.sum()
    if not (np.isfinite(tot) and tot > 0):
        return np.array([np.nan, np.nan])
    return np.array([(psf.sum(axis=1) * X).sum() / tot, (psf.sum(axis=0) * X).sum() / tot])


def psf_ee(psf, pitch, center, radii):
    """one PSF [M, M] -> ee [Nr] about ``center`` (None = its centroid)"""
    psf = np.asarray(psf, dtype=np.float64)
    M = psf.shape[0]
    c = psf_centroid(psf, pitch) if center is None else np.asarray(center, dtype=np.float64)
    X = pixel_coords(M, pitch)
    d2 = d2_of(X[:, None], X[None, :], c[0], c[1])
    tot = psf.sum()
    r = np.asarray(radii, dtype=np.float64).reshape(-1)
    if not (np.isfinite(tot) and tot > 0):
        return np.full(r.size, np.nan)
    return np.array([psf[d2 <= np.multiply(rj, rj)].sum() / tot for rj in r])


def focus_psf_ee(psf, pitch, centers, radii):
    """psf [n_items, K, M, M]; pitch broadcast to [n_items, K]; centers [n_items, K, 2] or None;
    radii broadcast to [n_items, K, Nr] -> (ee [n_items, K, Nr], centroid [n_items, K, 2])"""
    psf = np.asarray(psf, dtype=np.float64)
    n_items, K = psf.shape[:2]
    p = np.broadcast_to(np.asarray(pitch, dtype=np.float64), (n_items, K))
    r = np.asarray(radii, dtype=np.float64)
    r = np.broadcast_to(r, (n_items, K, r.shape[-1] if r.ndim else 1))
    ee = np.empty(r.shape)
    cen = np.empty((n_items, K, 2))
    for i in range(n_items):
        for k in range(K):
            cen[i, k] = psf_centroid(psf[i, k], p[i, k])
            ee[i, k] = psf_ee(psf[i, k], p[i, k], None if centers is None else centers[i][k], r[i, k])
    return ee, cen


# ---- polychromatic merges --------------------------------------------------------------------
def poly_counts_ee(counts, n, spectral_wts):
    """geometric: counts [W, ..., Nr], n [W, ...] -> sum_w s_w counts_w / sum_w s_w n_w (NaN where
    the denominator is 0)"""
    s = np.asarray(spectral_wts, dtype=np.float64)
    c = np.asarray(counts, dtype=np.float64)
    n = np.asarray(n, dtype=np.float64)
    sw = s.reshape((-1,) + (1,) * (c.ndim - 1))
    num = (sw * c).sum(axis=0)
    den = (s.reshape((-1,) + (1,) * (n.ndim - 1)) * n).sum(axis=0)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(den[..., None] > 0, num / den[..., None], np.nan)


def poly_psf_ee(ee, spectral_wts):
    """diffraction: ee [W, ..., Nr] of unit-energy PSFs -> sum_w s_w ee_w / sum_w s_w"""
    s = np.asarray(spectral_wts, dtype=np.float64)
    e = np.asarray(ee, dtype=np.float64)
    return (s.reshape((-1,) + (1,) * (e.ndim - 1)) * e).sum(axis=0) / s.sum()


def curve_radius(radii, curve, fraction):
    """the smallest radius at which the piecewise-linear curve through (radii, curve) reaches
    ``fraction``: linear interpolation inside the first segment that crosses it; NaN when the
    curve never does (or is NaN)"""
    r = np.asarray(radii, dtype=np.float64)
    e = np.asarray(curve, dtype=np.float64)
    if np.isnan(e).any():
        return np.nan
    hit = np.nonzero(e >= fraction)[0]
    if not hit.size:
        return np.nan
    j = int(hit[0])
    if j == 0:
        return float(r[0])
    t = (fraction - e[j - 1]) / (e[j] - e[j - 1])
    return float(r[j - 1] + t * (r[j] - r[j - 1]))
