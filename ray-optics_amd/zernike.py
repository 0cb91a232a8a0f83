"""Zernike polynomials over the unit disk: the term orders rox_focus_zernike is usually asked for
(Fringe / University of Arizona, Noll 1976), their names, and a NumPy evaluation that rebuilds a
wavefront map from fitted coefficients.

A term is ``(n, m, scale)``: ``scale * R_n^|m|(rho) * {1 | cos(m theta) | sin(|m| theta)}`` for
``m = 0``, ``m > 0``, ``m < 0``, with ``x = rho cos theta`` and ``y = rho sin theta``.
:func:`zernike_eval` evaluates it as rox_focus_zernike does, ``P(rho^2) * Re/Im((x + i y)^|m|)``
with ``P`` the radial polynomial over ``rho^|m|`` (its integer coefficients times ``scale``), by
Horner from the highest power; the same operations in the same order, so the basis matches the
device's to rounding."""
import math

import numpy as np

from . import abi


def _fringe_nm():
    out = []
    for s in range(6):                   # (n + |m|) / 2 = s; |m| from s down to 0, cos before sin
        for mm in range(s, -1, -1):
            n = 2 * s - mm
            out += [(n, mm), (n, -mm)] if mm else [(n, 0)]
    return out + [(12, 0)]               # Z37


_FRINGE = _fringe_nm()


def fringe_terms(n_terms=37):
    """the first ``n_terms`` (1..37) Fringe Zernike terms, scale 1: Z1 piston, Z2/Z3 tilt x/y, Z4
    defocus 2 rho^2 - 1, Z5/Z6 astigmatism 0/45 deg, Z7/Z8 coma x/y, Z9 spherical
    6 rho^4 - 6 rho^2 + 1, ..., Z36 (10, 0), Z37 (12, 0)"""
    n_terms = int(n_terms)
    if not 1 <= n_terms <= 37:
        raise ValueError(f'fringe_terms: n_terms {n_terms} outside [1, 37]')
    return [(n, m, 1.0) for n, m in _FRINGE[:n_terms]]


def noll_terms(n_terms):
    """the first ``n_terms`` (1..91) Noll terms: within an order |m| increases; for m != 0 an
    even index j takes the cosine and an odd j the sine; scale sqrt(n + 1) for m = 0 and
    sqrt(2 (n + 1)) otherwise, so each term has unit RMS over the disk"""
    n_terms = int(n_terms)
    if not 1 <= n_terms <= abi.MAX_ZERNIKE_TERMS:
        raise ValueError(f'noll_terms: n_terms {n_terms} outside [1, {abi.MAX_ZERNIKE_TERMS}]')
    out = []
    n = 0
    while len(out) < n_terms:
        for mm in range(n % 2, n + 1, 2):
            if mm == 0:
                out.append((n, 0, math.sqrt(n + 1)))
            else:
                for _two in range(2):
                    j = len(out) + 1
                    out.append((n, mm if j % 2 == 0 else -mm, math.sqrt(2 * (n + 1))))
        n += 1
    return out[:n_terms]


_NAMES = {(0, 0): 'piston', (1, 1): 'tilt x', (1, -1): 'tilt y', (2, 0): 'defocus',
          (2, 2): 'astigmatism 0', (2, -2): 'astigmatism 45', (3, 1): 'coma x', (3, -1): 'coma y',
          (4, 0): 'spherical', (3, 3): 'trefoil 0', (3, -3): 'trefoil 30',
          (4, 2): 'secondary astigmatism 0', (4, -2): 'secondary astigmatism 45',
          (5, 1): 'secondary coma x', (5, -1): 'secondary coma y', (6, 0): 'secondary spherical',
          (4, 4): 'tetrafoil 0', (4, -4): 'tetrafoil 22.5', (8, 0): 'tertiary spherical'}


def term_name(n, m):
    """the classical name of (n, m) ('defocus', 'coma x', ...), else 'Z(n,m)'"""
    return _NAMES.get((int(n), int(m)), f'Z({int(n)},{int(m)})')


def term_names(terms):
    return [term_name(t[0], t[1]) for t in terms]


def check_terms(terms, count=True):
    """(n, m, scale) triples (a scale may be left out: 1), checked as rox_focus_zernike checks
    them (their number too, with ``count``)"""
    out = []
    for t in terms:
        n, m = int(t[0]), int(t[1])
        s = float(t[2]) if len(t) > 2 else 1.0
        if not (0 <= n <= abi.MAX_ZERNIKE_ORDER and abs(m) <= n and (n - abs(m)) % 2 == 0
                and math.isfinite(s)):
            raise ValueError(f'Zernike term (n, m, scale) = ({n}, {m}, {s}): need 0 <= n <= '
                             f'{abi.MAX_ZERNIKE_ORDER}, |m| <= n, n - |m| even, a finite scale')
        out.append((n, m, s))
    if count and not 1 <= len(out) <= abi.MAX_ZERNIKE_TERMS:
        raise ValueError(f'1 to {abi.MAX_ZERNIKE_TERMS} Zernike terms, got {len(out)}')
    return out


def radial_coefficients(n, m, scale=1.0):
    """the coefficients of P(s) = R_n^|m|(rho) / rho^|m| in s = rho^2, highest power first, each
    the exact integer times ``scale`` (one IEEE product) -- the table rox_focus_zernike builds"""
    mm = abs(m)
    out = []
    for k in range((n - mm) // 2 + 1):
        q = math.factorial(n - k) // (math.factorial(k) * math.factorial((n + mm) // 2 - k)
                                      * math.factorial((n - mm) // 2 - k))
        v = float(q) * scale
        out.append(-v if k % 2 else v)
    return out


def zernike_eval(terms, x, y):
    """the terms at pupil points (x, y) (broadcast together; normalised to the unit circle) ->
    float64 [..., J].  A map is ``zernike_eval(terms, x, y) @ coef``."""
    terms = check_terms(terms, count=False)
    x, y = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
    s = x * x + y * y
    out = np.empty(x.shape + (len(terms),))
    for j, (n, m, sc) in enumerate(terms):
        c = radial_coefficients(n, m, sc)
        q = np.full(x.shape, c[0])
        for v in c[1:]:
            q = q * s + v
        if m == 0:
            out[..., j] = q
            continue
        re, im = np.ones(x.shape), np.zeros(x.shape)
        for _i in range(abs(m)):
            re, im = re * x - im * y, re * y + im * x
        out[..., j] = q * (re if m > 0 else im)
    return out
