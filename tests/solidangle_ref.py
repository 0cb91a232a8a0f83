"""TEST INFRASTRUCTURE: rox_projected_solid_angle restated in NumPy float64, one operation per step
in the order include/roxtrace.h states, and its records summed with math.fsum (the exactly rounded
sum, which any order of summation approaches within n * 2^-53 * sum|terms|).  Not the code under
test: no HIP, no engine."""
import math

import numpy as np

from rayoptics_amd import abi
from rayoptics_amd.engine import SA_ITEM_DTYPE

EPS = 2.0 ** -53
SUMS = ('a_full', 'a_tri', 'a_abs', 'aw_full', 'aw_tri', 'l_sum', 'm_sum')
A, B, C, D = ((slice(0, -1), slice(0, -1)), (slice(1, None), slice(0, -1)), (slice(1, None), slice(1, None)),
              (slice(0, -1), slice(1, None)))


def cells(L, M, status, num, weight=None):
    """rays r = i*num + j -> dict(k [num-1, num-1] counted corners, area, w the cell weight,
    ok [num, num]); a value of a ray that does not count is never used (it may be NaN)"""
    ok = (np.asarray(status).reshape(num, num) == abi.OK)
    L = np.where(ok, np.asarray(L, dtype=np.float64).reshape(num, num), 0.0)
    M = np.where(ok, np.asarray(M, dtype=np.float64).reshape(num, num), 0.0)
    W = np.ones((num, num)) if weight is None else \
        np.where(ok, np.asarray(weight, dtype=np.float64).reshape(num, num), 0.0)
    k = ok[A].astype(np.int64) + ok[B] + ok[C] + ok[D]

    def half_cross(p, q, r):
        t1 = L[q] - L[p]
        t2 = M[r] - M[p]
        t3 = L[r] - L[p]
        t4 = M[q] - M[p]
        return (t1 * t2 - t3 * t4) * 0.5

    # k = 4: ((Lc - La)*(Md - Mb) - (Ld - Lb)*(Mc - Ma)) * 0.5
    t1 = L[C] - L[A]
    t2 = M[D] - M[B]
    t3 = L[D] - L[B]
    t4 = M[C] - M[A]
    quad = (t1 * t2 - t3 * t4) * 0.5
    wquad = ((W[A] + W[B]) + (W[C] + W[D])) * 0.25
    area = np.where(k == 4, quad, 0.0)
    w = np.where(k == 4, wquad, 0.0)
    # k = 3: the counted corners in the order a, b, c, d
    for miss, (p, q, r) in ((A, (B, C, D)), (B, (A, C, D)), (C, (A, B, D)), (D, (A, B, C))):
        sel = (k == 3) & ~ok[miss]
        area = np.where(sel, half_cross(p, q, r), area)
        w = np.where(sel, ((W[p] + W[q]) + W[r]) / 3.0, w)
    return dict(k=k, area=area, w=w, ok=ok, L=L, M=M)


def record(c):
    """the rox_sa_item of cells(): (SA_ITEM_DTYPE record, {sum name: (terms n, sum of |terms|)})"""
    k, area, w, ok = c['k'], c['area'], c['w'], c['ok']
    rec = np.zeros((), SA_ITEM_DTYPE)
    rec['n_ok'] = int(ok.sum())
    rec['n_cells'] = [int((k == n).sum()) for n in range(5)]
    terms = dict(a_full=area[k == 4], a_tri=area[k == 3], a_abs=np.abs(area[k >= 3]),
                 aw_full=(area * w)[k == 4], aw_tri=(area * w)[k == 3], l_sum=c['L'][ok], m_sum=c['M'][ok])
    bounds = {}
    for name in SUMS:
        rec[name] = math.fsum(terms[name])
        bounds[name] = (int(terms[name].size), math.fsum(np.abs(terms[name])))
    any_ = bool(ok.any())
    Lo, Mo = c['L'][ok], c['M'][ok]
    rec['l_min'] = Lo.min() if any_ else np.nan
    rec['l_max'] = Lo.max() if any_ else np.nan
    rec['m_min'] = Mo.min() if any_ else np.nan
    rec['m_max'] = Mo.max() if any_ else np.nan
    rec['r2_max'] = (Lo * Lo + Mo * Mo).max() if any_ else np.nan
    return rec, bounds


def solid_angle(L, M, status, num, weight=None):
    """-> (record, cells [num-1, num-1], bounds)"""
    c = cells(L, M, status, num, weight)
    rec, bounds = record(c)
    return rec, c['area'], bounds


def dir_row(seg):
    """the row of L in a LAST [10, R] or FULL [n_seg, 10, R] packet"""
    return 3 if seg.ndim == 2 else (seg.shape[0] - 1) * 10 + 3


def of_packet(seg, status, num, weight=None):
    """solid_angle of a host packet, LAST or FULL"""
    flat = np.asarray(seg).reshape(-1, np.asarray(seg).shape[-1])
    r = dir_row(np.asarray(seg))
    return solid_angle(flat[r], flat[r + 1], status, num, weight)


def same(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


def check_record(got, rec, bounds, what, log=print):
    """a device record against the restatement's: counts, minima and maxima exact, sums within
    n * 2^-53 * sum|terms| of math.fsum; returns the largest error over bound"""
    assert int(got['n_ok']) == int(rec['n_ok']), what
    assert np.array_equal(got['n_cells'], rec['n_cells']), (what, got['n_cells'], rec['n_cells'])
    for name in ('l_min', 'l_max', 'm_min', 'm_max', 'r2_max'):
        assert same(float(got[name]), float(rec[name])), (what, name, float(got[name]), float(rec[name]))
    worst = 0.0
    for name in SUMS:
        n, mag = bounds[name]
        err, bound = abs(float(got[name]) - float(rec[name])), n * EPS * mag
        log(f'{what}: {name} n {n} error {err:.3g} (bound {bound:.3g})')
        assert err <= bound, (what, name, float(got[name]), float(rec[name]), err, bound)
        worst = max(worst, err / bound if bound > 0 else 0.0)
    return worst
