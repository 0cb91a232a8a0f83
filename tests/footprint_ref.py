"""rox_surface_footprints restated in NumPy: the records of every ray (``nseg``), the two selection
flags, every field of rox_footprint and the maps through numpy.histogram2d itself.  Sums are
math.fsum, so centroid, RMS radius and cos_inc_sum are the exact values the device's pairwise
reductions are bounded against (``exact=False``: plain NumPy sums, the restatement a user without
the entry would write)."""
import math

import numpy as np

from rayoptics_amd import abi


def slot_tables(table, trace_flags):
    """(nb, slot_ifc, n_seg): slots before interface s, the interface of slot k"""
    N = table.n_ifcs
    filt = bool(trace_flags & abi.FILTER_PHANTOMS)
    nb, slot_ifc = [], []
    for i, row in enumerate(table.rows):
        nb.append(len(slot_ifc))
        if not (filt and row.mode == abi.PHANTOM and 0 < i < N - 1):
            slot_ifc.append(i)
    return np.array(nb), np.array(slot_ifc), len(slot_ifc)


def nseg(table, trace_flags, status, fail_surf):
    """records per ray, as HostPackets.nseg counts them (an interface index outside the table: 0)"""
    nb, _si, n_seg = slot_tables(table, trace_flags)
    status, s = np.asarray(status).astype(int), np.asarray(fail_surf).astype(int)
    N = table.n_ifcs
    known = (s > 0) & (s < N)
    sc = np.clip(s, 1, N - 1)
    out = np.where(status == abi.MISSED_SURFACE, nb[sc - 1] + 1, nb[sc] + 1)
    out = np.where(known, out, 0)
    return np.where(status == abi.OK, n_seg, out)


def _rt_dot(row, v):
    """rt.dot(v) over the columns in the row's rt_order, each step one fma (as NumPy's dgemv)"""
    rt = np.array(list(row.rt)).reshape(3, 3)
    order = (1, 0, 2) if row.rt_order == abi.RT_C_ORDER else (0, 1, 2)
    # float64 products and sums without fma differ from the fused chain by a rounding: below the
    # 8 * 2^-53 bound the angle fields are held to
    out = np.zeros_like(v)
    for c in order:
        out = out + rt[:, c][:, None] * v[c][None, :]
    return out


def _m2_about(v, c):
    """sum((v - mean(v))^2) with c = the rounded mean: the deviations v - c as exact two-term sums
    (TwoSum), so that neither a mean that is large against the spread (an object at 1e10) nor its
    rounding enters; what remains is the rounding of each squared term, a few 2^-53 of the sum"""
    d = v - c
    bv = d - v                                  # TwoSum(v, -c): v - c == d + lo exactly
    lo = (v - (d - bv)) + (-c - bv)
    n = v.size
    eps = (math.fsum(d) + math.fsum(lo)) / n
    return math.fsum(d * d) + 2.0 * math.fsum(d * lo) - n * eps * eps


def footprints(table, trace_flags, seg, status, fail_surf, partial=True, ok_only=False, half_width=None,
               n_bins=0, exact=True):
    """-> (records, maps, terms): ``records`` a dict of arrays [n_seg] named as rox_footprint's
    fields (n_fail [n_seg, 5]); ``maps`` [n_seg, n_bins, n_bins] or None; ``terms`` a dict of
    the sums of absolute terms and counts the pairwise bound is formed from"""
    nb, slot_ifc, n_seg = slot_tables(table, trace_flags)
    seg = np.asarray(seg)
    status, fs = np.asarray(status).astype(int), np.asarray(fail_surf).astype(int)
    R = status.shape[0]
    assert seg.shape[0] == n_seg
    ns = nseg(table, trace_flags, status, fs)
    has_partial = (status != abi.OK) & (status != abi.MISSED_SURFACE) & (ns > 0)
    nfull = ns - has_partial
    if ok_only:
        nfull = np.where(status == abi.OK, nfull, 0)
    count_partial = has_partial & partial & (not ok_only)
    tot = math.fsum if exact else (lambda a: float(np.sum(a)))
    f64 = lambda fill: np.full(n_seg, fill, dtype=np.float64)
    rec = dict(n=np.zeros(n_seg, np.int64), n_fail=np.zeros((n_seg, 5), np.int64), n_inc=np.zeros(n_seg, np.int64),
               min=np.full((n_seg, 2), np.inf), max=np.full((n_seg, 2), -np.inf), r2_max=f64(-np.inf),
               cx=f64(np.nan), cy=f64(np.nan), rms_r=f64(np.nan), cos_inc_min=f64(np.nan),
               cos_inc_sum=f64(np.nan), cos_exit_min=f64(np.nan))
    terms = dict(abs_x=f64(0.0), abs_y=f64(0.0), abs_ci=f64(0.0), sq=f64(0.0))
    maps = np.zeros((n_seg, n_bins, n_bins), np.uint32) if n_bins else None
    N = table.n_ifcs
    for r in range(R):
        if status[r] != abi.OK and 1 <= status[r] <= 4 and 0 <= fs[r] < N:
            rec['n_fail'][nb[fs[r]], status[r]] += 1
    prev_d = None
    for k in range(n_seg):
        full = k < nfull
        geo = full | (count_partial & (k == ns - 1))
        x, y = seg[k, 0, geo], seg[k, 1, geo]
        n = int(geo.sum())
        rec['n'][k] = n
        if n:
            rec['min'][k] = x.min(), y.min()
            rec['max'][k] = x.max(), y.max()
            rec['r2_max'][k] = (x * x + y * y).max()
            cx, cy = tot(x) / n, tot(y) / n
            rec['cx'][k], rec['cy'][k] = cx, cy
            if exact and n <= 4096:     # the second moment about the exact centroid, in exact arithmetic
                from fractions import Fraction as Fr
                sx, sy = sum(map(Fr, x.tolist())), sum(map(Fr, y.tolist()))
                sxx = sum(Fr(v) * Fr(v) for v in x.tolist()) + sum(Fr(v) * Fr(v) for v in y.tolist())
                m2 = sxx - (sx * sx + sy * sy) / n
                rec['rms_r'][k] = math.sqrt(float(m2 / n))
            elif exact:
                rec['rms_r'][k] = math.sqrt((_m2_about(x, cx) + _m2_about(y, cy)) / n)
            else:
                rec['rms_r'][k] = math.sqrt(tot((x - cx) ** 2 + (y - cy) ** 2) / n)
            terms['abs_x'][k], terms['abs_y'][k] = tot(np.abs(x)), tot(np.abs(y))
            terms['sq'][k] = tot(x * x) + tot(y * y)
            if maps is not None:
                h = float(half_width[k])
                maps[k] = np.histogram2d(x, y, bins=n_bins, range=[[-h, h], [-h, h]])[0].astype(np.uint32)
        if full.any():
            d, nr = seg[k, 3:6][:, full], seg[k, 7:10][:, full]
            rec['cos_exit_min'][k] = np.abs((d * nr).sum(axis=0)).min()
            if k >= 1:
                b4 = prev_d[:, full]
                for i in range(slot_ifc[k - 1], slot_ifc[k]):
                    b4 = _rt_dot(table.rows[i], b4)
                ci = np.abs((b4 * nr).sum(axis=0))
                rec['n_inc'][k] = ci.size
                rec['cos_inc_min'][k] = ci.min()
                rec['cos_inc_sum'][k] = tot(ci)
                terms['abs_ci'][k] = rec['cos_inc_sum'][k]
        prev_d = seg[k, 3:6]
    return rec, maps, terms


def edges(h, n_bins):
    """the edges of a map axis, formed as the kernel forms them"""
    step = (h + h) / n_bins
    e = np.array([-h + j * step for j in range(n_bins + 1)])
    e[-1] = h
    return e
