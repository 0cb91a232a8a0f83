"""TEST INFRASTRUCTURE: rox_wave_differentials (include/roxtrace.h) restated in NumPy from host
copies of a FULL packet (``seg`` [n_seg, 10, R], ``status`` [R]) and the table's rt, indices and
profiles: the columns in the stated operation order, every step one float64 operation, so that a
ray's columns are the device's bit for bit; the pivot; and sums and gram in ``longdouble`` over the
float64 differences from the pivot, with the sums of the absolute terms for the any-order bound the
device's sums are held to.  And the perturbed tables the physics is checked against: a rigid motion
of one interface through rt / t of rows s-1 and s, its curvature, a gap's index."""
import ctypes as C
import math

import numpy as np

from fresnel_ref import _carry, _cross, slot_interfaces
from rayoptics_amd import SurfaceTable, abi

SLOT_COLS = 11
# What first order leaves out of a predicted wavefront change, as a fraction of the largest |dW| over
# the pupil: the largest value tests/test_wavediff_host.py measures on the CPU oracle (full vignetted
# 16 x 16 pupil of the double Gauss; 1.1e-3 .. 4.9e-3).  It is the margin the GPU test of
# analyses.tolerance_sensitivity allows between predicted and re-traced RMS.
FIRST_ORDER_MARGIN = 4.9e-3
Q_PROFILES = (abi.SPHERICAL, abi.CONIC, abi.EVENPOLY, abi.RADIALPOLY)


def columns(table, trace_flags, seg, status, wvl_idx, slots=None, aux=None):
    """-> (cols [n_cols, R], counted [R], n_bad): NaN (every column) where a ray is not counted"""
    seg = np.asarray(seg, dtype=np.float64)
    ok = np.asarray(status) == abi.OK
    R = ok.shape[0]
    si = slot_interfaces(table, trace_flags)
    n_seg = len(si)
    assert seg.shape[0] == n_seg
    slots = list(range(n_seg)) if slots is None else [int(k) for k in slots]
    n_aux = 0 if aux is None else int(np.shape(aux)[0])
    nt = np.asarray(table.n_table, dtype=np.float64)[wvl_idx]
    n = int(ok.sum())
    out = np.full((n_aux + SLOT_COLS * len(slots), n), np.nan)
    if n_aux:
        out[:n_aux] = np.asarray(aux, dtype=np.float64)[:, :R][:, ok]
    b4 = None
    with np.errstate(all='ignore'):
        for k in range(n_seg):
            p, d, dst = seg[k, 0:3][:, ok], seg[k, 3:6][:, ok], seg[k, 6][ok]
            s = si[k]
            if k >= 1:
                for i in range(si[k - 1], s):
                    b4 = _carry(table.rows[i], b4)
            else:
                b4 = d
            if k in slots:
                last = k == n_seg - 1
                n1 = abs(float(nt[0] if k == 0 else nt[s - 1]))
                n2 = 0.0 if last else abs(float(nt[0] if k == 0 else nt[s]))
                g = np.stack([n1 * b4[c] - n2 * d[c] for c in range(3)])
                m = _cross(p, g)
                x, y = p[0], p[1]
                r2 = x * x + y * y
                row = table.rows[s]
                cvf = r2 / 2.0
                if row.profile in Q_PROFILES:
                    rad = 1.0 - ((float(row.ec) * float(row.cv)) * float(row.cv)) * r2
                    q = np.sqrt(np.where(rad > 0.0, rad, 1.0))
                    cvf = np.where(rad > 0.0, r2 / (q * (1.0 + q)), cvf)
                c0 = n_aux + SLOT_COLS * slots.index(k)
                out[c0:c0 + 3] = g
                out[c0 + 3:c0 + 6] = m
                out[c0 + 6] = g[2] * cvf
                out[c0 + 7] = g[2] * r2
                out[c0 + 8] = g[2] * (x * x - y * y)
                out[c0 + 9] = g[2] * ((x + x) * y)
                out[c0 + 10] = 0.0 if last else dst
            b4 = d
    fin = np.isfinite(out).all(axis=0)
    cols = np.full((out.shape[0], R), np.nan)
    counted = np.zeros(R, bool)
    counted[np.flatnonzero(ok)[fin]] = True
    cols[:, counted] = out[:, fin]
    return cols, counted, int((~fin).sum())


def reduce(cols, counted):
    """-> dict(n, pivot_ray, pivot [n_cols], sums [n_cols], gram [n_cols, n_cols] (longdouble),
    abs_sums, abs_gram: the sums of the absolute terms)"""
    n_cols = cols.shape[0]
    idx = np.flatnonzero(counted)
    n = int(idx.size)
    if n == 0:
        z = np.zeros(n_cols, np.longdouble)
        zz = np.zeros((n_cols, n_cols), np.longdouble)
        return dict(n=0, pivot_ray=-1, pivot=np.full(n_cols, np.nan), sums=z, gram=zz, abs_sums=z, abs_gram=zz)
    pivot = cols[:, idx[0]].copy()
    dev = cols[:, idx] - pivot[:, None]                     # float64 differences, as the device forms them
    ld = dev.astype(np.longdouble)
    return dict(n=n, pivot_ray=int(idx[0]), pivot=pivot, sums=ld.sum(axis=1), gram=ld @ ld.T,
                abs_sums=np.abs(ld).sum(axis=1), abs_gram=np.abs(ld) @ np.abs(ld).T)


# ---- perturbed tables ------------------------------------------------------------------------
def copy_table(table):
    rows = (abi.Surface * table.n_ifcs)()
    C.memmove(rows, table.rows, C.sizeof(rows))
    t = SurfaceTable(rows, np.array(table.n_table), table.wvls, table.stop_idx)
    return t


def rodrigues(alpha):
    a = np.asarray(alpha, dtype=np.float64)
    th = float(np.linalg.norm(a))
    if th == 0.0:
        return np.identity(3)
    k = a / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.identity(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def moved(table, s, delta=(0, 0, 0), alpha=(0, 0, 0)):
    """interface s shifted by delta and rotated by alpha about its vertex (both in its own frame):
    x' = Ra^T (x - delta) are the new frame's coordinates, so rows s-1 and s become
    rt'[s-1] = Ra^T rt[s-1], t'[s-1] = t[s-1] + rt[s-1]^T delta; rt'[s] = rt[s] Ra, t'[s] = Ra^T (t[s] - delta)"""
    t = copy_table(table)
    Ra, delta = rodrigues(alpha), np.asarray(delta, dtype=np.float64)
    rt0 = np.array(list(table.rows[s - 1].rt)).reshape(3, 3)
    t0 = np.array(list(table.rows[s - 1].t))
    rt1 = np.array(list(table.rows[s].rt)).reshape(3, 3)
    t1 = np.array(list(table.rows[s].t))
    new = ((s - 1, Ra.T @ rt0, t0 + rt0.T @ delta), (s, rt1 @ Ra, Ra.T @ (t1 - delta)))
    for i, rt, tt in new:
        for e in range(9):
            t.rows[i].rt[e] = float(rt.reshape(-1)[e])
        for e in range(3):
            t.rows[i].t[e] = float(tt[e])
        t.rows[i].rt_order = abi.RT_C_ORDER
    return t


def curved(table, s, dcv):
    t = copy_table(table)
    t.rows[s].cv = table.rows[s].cv + dcv
    return t


def indexed(table, s, wvl, dn):
    """|n| of gap s grows by dn at wavelength row ``wvl`` (None: at every one)"""
    t = copy_table(table)
    for w in range(t.n_table.shape[0]) if wvl is None else (wvl,):
        t.n_table[w, s] = table.n_table[w, s] + (dn if table.n_table[w, s] > 0 else -dn)
    return t


def shifted_group(table, s1, s2, delta):
    """interfaces s1 .. s2 shifted together by delta (parallel frames)"""
    for s in range(s1, s2 + 1):
        table = moved(table, s, delta=delta)
    return table
