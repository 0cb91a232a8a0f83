"""rox_surface_thinfilm restated in NumPy complex128 from host copies of a FULL packet, in a
formulation the product does not use: a stack's amplitude coefficients come from the recursive
Airy summation, layer by layer from the exit side,

    r_j = (r_{j,j+1} + r_{j+1} e^{2 i delta_{j+1}}) / (1 + r_{j,j+1} r_{j+1} e^{2 i delta_{j+1}})
    t_j = t_{j,j+1} t_{j+1} e^{i delta_{j+1}}       / (1 + r_{j,j+1} r_{j+1} e^{2 i delta_{j+1}})

with the single-interface coefficients of two adjacent media (no characteristic matrix; e^{i delta}
of an absorbing layer decays, so nothing overflows), and the field carry of fresnel_ref.py with
complex E.  The device's sincos / exp / sqrt / division are not NumPy's and the two formulations
round differently, so rows are compared within a bound.

``stack`` = dict(first [n_ifcs + 1], thick [L], index [n_wvls, L] complex, sub [n_wvls, n_ifcs]
complex or None) describes the layers as the C entry takes them."""
import math

import numpy as np

import fresnel_ref as FR
from rayoptics_amd import abi

EPS = FR.EPS
# The largest |device row - restatement row| over every case of tests/test_gpu_thinfilm.py
# (test_against_the_restatement prints it per case), rows T, T1, T2, D and the 12 field rows alike,
# was measured on an MI355X at 5.44e-15 (49 * 2^-53: dblgauss_c2 at 33 x 33 rays, item 3; the other
# cases 1.3e-15 to 4.9e-15); the tests assert 10 x that.
ROW_MEASURED = 5.44e-15
ROW_BOUND = 10 * ROW_MEASURED


def stack_dict(first, thick, index, sub=None):
    """from the arrays coatings.stack_tables returns ([W, L, 2] and [W, N, 2] of (re, im))"""
    index = np.asarray(index, dtype=np.float64)
    return dict(first=np.asarray(first), thick=np.asarray(thick, dtype=np.float64),
                index=index[..., 0] + 1j * index[..., 1],
                sub=None if sub is None else np.asarray(sub)[..., 0] + 1j * np.asarray(sub)[..., 1])


def _sqrt_up(z):
    g = np.sqrt(np.asarray(z, dtype=np.complex128))
    return np.where(g.imag < 0.0, -g, g)


def airy(n1, n_exit, layers, thick, wvl, a2, A):
    """(rho_s, rho_p, tau_s, tau_p) of the layers (complex indices, in crossing order) between the
    real n1 and n_exit (complex allowed), for the rays' a2 = n1^2 sin^2 and A = n1 ci"""
    N = [complex(n1)] + [complex(v) for v in layers] + [complex(n_exit)]
    g = [A + 0j] + [_sqrt_up(v * v - a2) for v in N[1:]]
    out = []
    for pol in 'sp':
        y = [gj if pol == 's' else v * v / gj for v, gj in zip(N, g)]
        m = len(N) - 2                                       # layers
        r = (y[m] - y[m + 1]) / (y[m] + y[m + 1])
        t = 2.0 * y[m] / (y[m] + y[m + 1])
        for j in range(m - 1, -1, -1):                       # interface j | j+1, through layer j+1
            rj = (y[j] - y[j + 1]) / (y[j] + y[j + 1])
            tj = 2.0 * y[j] / (y[j] + y[j + 1])
            ph = np.exp(1j * (2.0 * math.pi * thick[j] / wvl) * g[j + 1])
            den = 1.0 + rj * r * ph * ph
            r, t = (rj + r * ph * ph) / den, tj * t * ph / den
        out += [r, t]
    return out[0], out[2], out[1], out[3]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def thinfilm(table, trace_flags, seg, status, wvl_idx, wvl, coat_kind=None, coat_value=None, stack=None, fields=False):
    """-> dict(rows [4 or 16, R] (NaN where status != OK), ok [R], Ts, Tp, ci [n_seg, n_ok]) as
    fresnel_ref.transmission_a, complex inside"""
    seg = np.asarray(seg, dtype=np.float64)
    ok = np.asarray(status) == abi.OK
    R = ok.shape[0]
    si = FR.slot_interfaces(table, trace_flags)
    n_seg = len(si)
    assert seg.shape[0] == n_seg
    kinds = None if coat_kind is None else np.where(np.asarray(coat_kind) == abi.COAT_STACK, abi.COAT_BARE, coat_kind)
    md = FR.models(table, wvl_idx, kinds, coat_value)
    nt = np.asarray(table.n_table)[wvl_idx]
    n = int(ok.sum())
    Ts_all, Tp_all, ci_all = (np.ones((n_seg, n)) for _ in range(3))
    one = np.ones(n)
    ex, ey = np.stack([one, 0 * one, 0 * one]), np.stack([0 * one, one, 0 * one])
    q = one.copy()
    b4 = E1 = E2 = None
    with np.errstate(all='ignore'):
        for k in range(n_seg):
            d, N = seg[k, 3:6][:, ok], seg[k, 7:10][:, ok]
            if k >= 1:
                for i in range(si[k - 1], si[k]):
                    rt = np.array(list(table.rows[i].rt), dtype=np.float64).reshape(3, 3)
                    b4, E1, E2 = rt @ b4, rt @ E1, rt @ E2
            else:
                e = np.stack([d[2], 0 * one, -d[0]])
                e = np.where(_dot(e, e) == 0.0, ex, e)
                E1 = (e / np.sqrt(_dot(e, e))).astype(np.complex128)
                E2 = np.cross(d, E1.real, axis=0).astype(np.complex128)
                b4 = d
            ci = np.abs(_dot(b4, N))
            ci_all[k] = ci
            if 0 < k < n_seg - 1:
                s = si[k]
                m, n1, n2, cTs, cTp = md[s]
                ct = np.abs(_dot(d, N))
                if coat_kind is not None and int(coat_kind[s]) == abi.COAT_STACK:
                    l0, l1 = int(stack['first'][s]), int(stack['first'][s + 1])
                    lay, th = stack['index'][wvl_idx, l0:l1], stack['thick'][l0:l1]
                    n1, n2 = float(nt[s - 1]), float(nt[s])
                    A, a2 = n1 * ci, n1 * n1 * (1.0 - ci * ci)
                    if table.rows[s].mode == abi.REFLECT:
                        rs, rp, _ts, _tp = airy(n1, stack['sub'][wvl_idx, s], lay, th, wvl, a2, A)
                        ts, tp, qs = rs, -rp, one
                    else:
                        _rs, _rp, ts, tp = airy(n1, n2, lay, th, wvl, a2, A)
                        tp = tp * ci / ct
                        qs = n2 * ct / A
                    Ts, Tp = qs * np.abs(ts) ** 2, qs * np.abs(tp) ** 2
                elif m == FR.BARE:
                    A, B = n1 * ci, n2 * ct
                    z = ci == 0.0
                    ts, tp = np.where(z, 0.0, 2 * A / (A + B)), np.where(z, 0.0, 2 * A / (n2 * ci + n1 * ct))
                    qs = np.where(z, 0.0, B / A)
                    Ts, Tp = qs * ts * ts, qs * tp * tp
                else:
                    ts = (-math.sqrt(cTs) if m in (FR.MIRROR, FR.FIXED_MIRROR) else math.sqrt(cTs)) * one
                    tp, qs = math.sqrt(cTp) * one, one
                    Ts, Tp = cTs * one, cTp * one
                c = np.cross(b4, N, axis=0)
                alt = np.where(np.abs(b4[0]) <= np.abs(b4[1]), np.cross(b4, ex, axis=0), np.cross(b4, ey, axis=0))
                c = np.where(_dot(c, c) == 0.0, alt, c)
                sh = c / np.sqrt(_dot(c, c))
                pi, po = np.cross(b4, sh, axis=0), np.cross(d, sh, axis=0)
                E1 = ts * _dot(sh, E1) * sh + tp * _dot(pi, E1) * po
                E2 = ts * _dot(sh, E2) * sh + tp * _dot(pi, E2) * po
                q = q * qs
                Ts_all[k], Tp_all[k] = Ts, Tp
            b4 = d
        g11, g22 = _dot(E1.conj(), E1).real, _dot(E2.conj(), E2).real
        g12 = _dot(E1.conj(), E2)
        m, h = (g11 + g22) / 2.0, (g11 - g22) / 2.0
        r = np.sqrt(h * h + np.abs(g12) ** 2)
        D = np.where(m == 0.0, 0.0, r / m)
    rows = np.full((16 if fields else 4, R), np.nan)
    rows[0, ok], rows[1, ok], rows[2, ok], rows[3, ok] = q * m, q * g11, q * g22, D
    if fields:
        rows[4:7, ok], rows[7:10, ok], rows[10:13, ok], rows[13:16, ok] = E1.real, E2.real, E1.imag, E2.imag
    return dict(rows=rows, ok=ok, Ts=Ts_all, Tp=Tp_all, ci=ci_all)


records = FR.records
