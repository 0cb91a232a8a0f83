"""TEST INFRASTRUCTURE for the MTF-through-focus tests: the line OTF of include/roxtrace.h's
rox_focus_mtf restated in NumPy, and the FFT-free check it is held against -- the normalised
circular autocorrelation of the padded pupil array analyses.calc_psf builds
(rayoptics/raytr/analyses.py:848-875).

A PSF is M x M, axis 0 image x, axis 1 image y, pixel (M/2, M/2) the image point; pixel j sits
at image coordinate SIGN * p * (j - M/2).  OTF_d(nu) = sum_j LSF_d[j] exp(-2 pi i nu x_j) /
sum_j LSF_d[j], LSF_x = PSF.sum(axis=1), LSF_y = PSF.sum(axis=0)."""
import numpy as np

SIGN = -1.0         # image coordinate of pixel j: SIGN * pitch * (j - M/2), both directions


def line_otf(psf, pitch, freqs):
    """[..., M, M] PSFs, pitch broadcast to [...], freqs [Q] -> complex [..., 2, Q]; NaN above
    the Nyquist frequency (nu p > 1/2) and where a projection's sum is not positive and finite"""
    psf = np.asarray(psf, dtype=np.float64)
    M = psf.shape[-1]
    lead = psf.shape[:-2]
    p = np.broadcast_to(np.asarray(pitch, dtype=np.float64), lead)
    nu = np.asarray(freqs, dtype=np.float64).reshape(-1)
    lsf = np.stack([psf.sum(axis=-1), psf.sum(axis=-2)], axis=-2)        # [..., 2, M]
    f = nu * p[..., None]                                                # [..., Q] cycles per pixel
    t = f[..., None] * (np.arange(M) - M // 2)                           # [..., Q, M]
    r = t - np.rint(t)
    kern = np.exp(-2j * np.pi * SIGN * r)                                # exp(-2 pi i nu x_j)
    num = np.einsum('...dm,...qm->...dq', lsf, kern)
    den = lsf.sum(axis=-1)[..., None]
    with np.errstate(invalid='ignore', divide='ignore'):
        out = num / den
    bad = ~(np.isfinite(den) & (den > 0)) | (f > 0.5)[..., None, :]
    return np.where(bad, np.nan + 0j, out)


def padded_pupil(opd, ndim, maxdim):
    """calc_psf's padded pupil array: exp(i 2 pi W) of the zero-padded OPD grid (NaN -> 0) with
    the entries equal to 1 zeroed (analyses.py:856-871)"""
    h, nd2 = maxdim // 2, ndim // 2
    W = np.zeros([maxdim, maxdim])
    W[h - (nd2 - 1):h + (nd2 + 1), h - (nd2 - 1):h + (nd2 + 1)] = np.nan_to_num(opd)
    phase = np.exp(1j * 2 * np.pi * W)
    phase[phase == 1] = 0
    return phase


def autocorrelation_otf(opd, ndim, maxdim, m):
    """the line OTFs at the lattice frequencies nu = m / (maxdim p), m an int array: the
    normalised circular autocorrelation of the padded pupil P along axis 0 (x) and axis 1 (y),
    sum P[i + SIGN' m] conj(P[i]) / sum |P|^2 -> complex [2, len(m)]"""
    P = padded_pupil(opd, ndim, maxdim)
    norm = (np.abs(P) ** 2).sum()
    shift = int(-SIGN)          # pixel offset direction of a positive image coordinate
    out = np.empty((2, len(m)), dtype=np.complex128)
    for d in range(2):
        for i, mm in enumerate(m):
            out[d, i] = (np.roll(P, -shift * int(mm), axis=d) * np.conj(P)).sum() / norm
    return out


def numpy_calc_psf(opd, ndim, maxdim):
    """analyses.calc_psf's arithmetic in NumPy"""
    AP = abs(np.fft.fftshift(np.fft.fft2(np.fft.fftshift(padded_pupil(opd, ndim, maxdim))))) ** 2
    return AP / np.nanmax(AP)


def psf_centroid(psf, pitch):
    """the PSF's centroid in image coordinates [..., 2] (x, y)"""
    psf = np.asarray(psf, dtype=np.float64)
    M = psf.shape[-1]
    x = SIGN * np.asarray(pitch, dtype=np.float64)[..., None] * (np.arange(M) - M // 2)
    tot = psf.sum(axis=(-1, -2))
    return np.stack([(psf.sum(axis=-1) * x).sum(axis=-1) / tot, (psf.sum(axis=-2) * x).sum(axis=-1) / tot], axis=-1)
