"""rox_surface_transmission restated in NumPy, twice, from host copies of a FULL packet (``seg``
[n_seg, 10, R], ``status`` [R]), the table's rt, modes and indices.

(A) ``transmission_a``: the operation order include/roxtrace.h states, vectorised over the rays --
    every step one float64 operation, so a ray's rows are the device's bit for bit.
(B) ``transmission_b``: an independent formulation, not in that order: the 3 x 3 polarization
    ray-tracing matrices P_s = O_out . diag(ts, tp, 1) . O_in^T multiplied along the ray (frame
    changes as plain matrix products), T and D from numpy.linalg.svd of the 3 x 2 matrix
    P . [e1 e2].

``records`` forms rox_tx_surface / rox_tx_item from (A)'s per-ray values with math.fsum, the exact
sums the device's pairwise sums are bounded against."""
import math

import numpy as np

from rayoptics_amd import abi

IDEAL, BARE, MIRROR, FIXED, FIXED_MIRROR = range(5)

# the bounds of the tests (derived in tests/test_transmission_host.py)
EPS = 2.0 ** -53
CLOSED = 32 * EPS               # a closed form, per surface pair
AB_MEASURED = 2.11e-15          # the largest |A - B| on the golden packets
AB_BOUND = 10 * AB_MEASURED


def slot_interfaces(table, trace_flags):
    N = table.n_ifcs
    filt = bool(trace_flags & abi.FILTER_PHANTOMS)
    return [i for i, row in enumerate(table.rows) if not (filt and row.mode == abi.PHANTOM and 0 < i < N - 1)]


def models(table, wvl_idx, coat_kind=None, coat_value=None):
    """per interface: (model, n1, n2, Ts, Tp) as the entry decides them"""
    nt = np.asarray(table.n_table)[wvl_idx]
    out = []
    for s, row in enumerate(table.rows):
        if not 0 < s < table.n_ifcs - 1:
            out.append((IDEAL, 1.0, 1.0, 1.0, 1.0))
            continue
        kind = abi.COAT_BARE if coat_kind is None else int(coat_kind[s])
        n1, n2 = float(nt[s - 1]), float(nt[s])
        m = IDEAL
        if row.mode == abi.REFLECT:
            m = FIXED_MIRROR if kind == abi.COAT_FIXED else MIRROR
        elif row.mode == abi.TRANSMIT and kind == abi.COAT_FIXED:
            m = FIXED
        elif (row.mode == abi.TRANSMIT and kind == abi.COAT_BARE and row.profile != abi.THINLENS
              and row.ph.kind == abi.PH_NONE and n1 != n2):
            m = BARE
        fixed = m in (FIXED, FIXED_MIRROR)
        out.append((m, n1, n2, float(coat_value[s][0]) if fixed else 1.0, float(coat_value[s][1]) if fixed else 1.0))
    return out


# ---- (A) the stated operation order ---------------------------------------------------------
def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return np.stack([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def _carry(row, v):
    rt = np.array(list(row.rt), dtype=np.float64).reshape(3, 3)
    c0, c1 = (1, 0) if row.rt_order == abi.RT_C_ORDER else (0, 1)
    return np.stack([(rt[a, c0] * v[c0] + rt[a, c1] * v[c1]) + rt[a, 2] * v[2] for a in range(3)])


def _through(E, s, pi, po, ts, tp):
    a, b = ts * _dot(s, E), tp * _dot(pi, E)
    return np.stack([a * s[0] + b * po[0], a * s[1] + b * po[1], a * s[2] + b * po[2]])


def transmission_a(table, trace_flags, seg, status, wvl_idx, coat_kind=None, coat_value=None, fields=False):
    """-> dict(rows [4 or 10, R] (NaN where status != OK), ok [R], and over the OK rays in ray
    order Ts, Tp, ci [n_seg, n_ok])"""
    seg = np.asarray(seg, dtype=np.float64)
    ok = np.asarray(status) == abi.OK
    R = ok.shape[0]
    si = slot_interfaces(table, trace_flags)
    n_seg = len(si)
    assert seg.shape[0] == n_seg
    md = models(table, wvl_idx, coat_kind, coat_value)
    n = int(ok.sum())
    Ts_all, Tp_all, ci_all = (np.ones((n_seg, n)) for _ in range(3))
    one = np.ones(n)
    ex, ey = np.stack([one, 0 * one, 0 * one]), np.stack([0 * one, one, 0 * one])
    b4 = E1 = E2 = None
    q = one.copy()
    with np.errstate(all='ignore'):
        for k in range(n_seg):
            d, N = seg[k, 3:6][:, ok], seg[k, 7:10][:, ok]
            if k >= 1:
                for i in range(si[k - 1], si[k]):
                    b4, E1, E2 = (_carry(table.rows[i], v) for v in (b4, E1, E2))
            else:
                e = np.stack([d[2], 0 * one, -d[0]])
                ee = _dot(e, e)
                e = np.where(ee == 0.0, ex, e)
                ee = _dot(e, e)
                E1 = e / np.sqrt(ee)
                E2 = _cross(d, E1)
                b4 = d
            ci = np.abs(_dot(b4, N))
            ci_all[k] = ci
            if 0 < k < n_seg - 1:
                m, n1, n2, cTs, cTp = md[si[k]]
                if m == BARE:
                    ct = np.abs(_dot(d, N))
                    A, B = n1 * ci, n2 * ct
                    ts = (A + A) / (A + B)
                    tp = (A + A) / (n2 * ci + n1 * ct)
                    qs = B / A
                    z = ci == 0.0
                    ts, tp, qs = np.where(z, 0.0, ts), np.where(z, 0.0, tp), np.where(z, 0.0, qs)
                    Ts, Tp = qs * (ts * ts), qs * (tp * tp)
                else:
                    ts = (-math.sqrt(cTs) if m in (MIRROR, FIXED_MIRROR) else math.sqrt(cTs)) * one
                    tp, qs = math.sqrt(cTp) * one, one
                    Ts, Tp = cTs * one, cTp * one
                c = _cross(b4, N)
                cc = _dot(c, c)
                alt = np.where(np.abs(b4[0]) <= np.abs(b4[1]), _cross(b4, ex), _cross(b4, ey))
                c = np.where(cc == 0.0, alt, c)
                cc = _dot(c, c)
                sh = c / np.sqrt(cc)
                pi, po = _cross(b4, sh), _cross(d, sh)
                E1, E2 = _through(E1, sh, pi, po, ts, tp), _through(E2, sh, pi, po, ts, tp)
                q = q * qs
                Ts_all[k], Tp_all[k] = Ts, Tp
            b4 = d
        g11, g12, g22 = _dot(E1, E1), _dot(E1, E2), _dot(E2, E2)
        m, h = (g11 + g22) / 2.0, (g11 - g22) / 2.0
        r = np.sqrt(h * h + g12 * g12)
        D = np.where(m == 0.0, 0.0, r / m)
    rows = np.full((10 if fields else 4, R), np.nan)
    rows[0, ok], rows[1, ok], rows[2, ok], rows[3, ok] = q * m, q * g11, q * g22, D
    if fields:
        rows[4:7, ok], rows[7:10, ok] = E1, E2
    return dict(rows=rows, ok=ok, Ts=Ts_all, Tp=Tp_all, ci=ci_all)


def records(a, n_rays=None):
    """(surf, item): dicts named as rox_tx_surface's and rox_tx_item's fields, from (A)'s result;
    sums are math.fsum"""
    n_seg, n = a['Ts'].shape
    nanmin = lambda v: float(v.min()) if v.size else math.nan
    nanmax = lambda v: float(v.max()) if v.size else math.nan
    surf = dict(n=np.full(n_seg, n, np.int64))
    for name, v in (('ts', a['Ts']), ('tp', a['Tp']), ('ci', a['ci'])):
        surf[name + '_sum'] = np.array([math.fsum(v[k]) for k in range(n_seg)])
        surf[name + '_min'] = np.array([nanmin(v[k]) for k in range(n_seg)])
    surf['t_sum'] = np.array([math.fsum((a['Ts'][k] + a['Tp'][k]) / 2.0) for k in range(n_seg)])
    ok = a['ok']
    T, T1, T2, D = (a['rows'][j][ok] for j in range(4))
    item = dict(n_ok=n, n_rays=int(ok.shape[0] if n_rays is None else n_rays), t_sum=math.fsum(T), t_min=nanmin(T),
                t_max=nanmax(T), t1_sum=math.fsum(T1), t2_sum=math.fsum(T2), d_sum=math.fsum(D), d_max=nanmax(D))
    return surf, item


# ---- (B) polarization ray-tracing matrices and the SVD -----------------------------------------
def _unit(v):
    return v / np.linalg.norm(v, axis=0, keepdims=True)


def transmission_b(table, trace_flags, seg, status, wvl_idx, coat_kind=None, coat_value=None):
    """-> rows [4, R]: T, T1, T2, D (NaN where status != OK)"""
    seg = np.asarray(seg, dtype=np.float64)
    ok = np.asarray(status) == abi.OK
    R = ok.shape[0]
    si = slot_interfaces(table, trace_flags)
    n_seg = len(si)
    md = models(table, wvl_idx, coat_kind, coat_value)
    n = int(ok.sum())
    d0 = seg[0, 3:6][:, ok]
    P = np.broadcast_to(np.eye(3), (n, 3, 3)).copy()        # the field's map from the object frame on
    q = np.ones(n)
    prev = d0
    for k in range(1, n_seg):
        d, N = seg[k, 3:6][:, ok], seg[k, 7:10][:, ok]
        b4 = prev
        for i in range(si[k - 1], si[k]):
            Rm = np.array(list(table.rows[i].rt), dtype=np.float64).reshape(3, 3)
            b4 = Rm @ b4
            P = Rm[None] @ P
        if k < n_seg - 1:
            m, n1, n2, cTs, cTp = md[si[k]]
            ci = np.abs(np.einsum('ir,ir->r', b4, N))
            ct = np.abs(np.einsum('ir,ir->r', d, N))
            if m == BARE:
                graze = ci == 0.0                           # nothing enters: the entry's convention
                with np.errstate(all='ignore'):
                    ts = np.where(graze, 0.0, 2.0 * n1 * ci / (n1 * ci + n2 * ct))
                    tp = np.where(graze, 0.0, 2.0 * n1 * ci / (n2 * ci + n1 * ct))
                    q = np.where(graze, 0.0, q * (n2 * ct) / (n1 * ci))
            else:
                ts = np.full(n, -math.sqrt(cTs) if m in (MIRROR, FIXED_MIRROR) else math.sqrt(cTs))
                tp = np.full(n, math.sqrt(cTp))
            c = np.cross(b4, N, axis=0)
            small = np.linalg.norm(c, axis=0) == 0.0
            if small.any():
                # exactly normal incidence: the plane of incidence is undefined, and with ts != tp there
                # (a fixed coating with Ts != Tp, a mirror's field vectors) the result depends on the
                # axis chosen -- so the axis is the one the header names, as in (A)
                axis = np.where(np.abs(b4[0]) <= np.abs(b4[1]), np.array([[1.0], [0.0], [0.0]]),
                                np.array([[0.0], [1.0], [0.0]]))
                c = np.where(small, np.cross(b4, axis, axis=0), c)
            s = _unit(c)
            O_in = np.stack([s, np.cross(b4, s, axis=0), b4], axis=1)          # [3, 3, n]: columns s, p, k
            O_out = np.stack([s, np.cross(d, s, axis=0), d], axis=1)
            diag = np.stack([ts, tp, np.ones(n)])
            Ps = np.einsum('icr,cr,jcr->rij', O_out, diag, O_in)
            P = Ps @ P
        prev = d
    a = np.stack([d0[2], np.zeros(n), -d0[0]])
    a = np.where(np.linalg.norm(a, axis=0) == 0.0, np.array([[1.0], [0.0], [0.0]]), a)
    e1 = _unit(a)
    e2 = np.cross(d0, e1, axis=0)
    M = P @ np.stack([e1, e2], axis=2).transpose(1, 0, 2)   # [n, 3, 2]
    sv = np.linalg.svd(M, compute_uv=False) if n else np.zeros((0, 2))
    s1, s2 = sv[:, 0] ** 2, sv[:, 1] ** 2
    rows = np.full((4, R), np.nan)
    rows[0, ok] = q * (s1 + s2) / 2.0
    rows[1, ok] = q * (M[:, :, 0] ** 2).sum(axis=1)
    rows[2, ok] = q * (M[:, :, 1] ** 2).sum(axis=1)
    with np.errstate(all='ignore'):
        rows[3, ok] = np.where(s1 + s2 == 0.0, 0.0, (s1 - s2) / (s1 + s2))
    return rows
