"""TEST INFRASTRUCTURE: the NumPy restatement of rox_weighted_maps (include/roxtrace.h) -- every
step one NumPy operation in the header's order: the edges as numpy.linspace builds them, the bin by
searchsorted(..., 'right') - 1 with the last edge closed, the largest usable value and the scale
exponent per map, q = rint(ldexp(v, e)) as int64, and np.add.at on int64.  Integer sums: the device
must reproduce every output bit for bit."""
import numpy as np

OK = 0
DTYPE = np.dtype([(name, np.int64) for name in ('n_in', 'n_out', 'n_bad', 'q_in', 'q_out')])


def edges(c, h, n):
    """the n + 1 edges of [c - h, c + h]: lo + j*((hi - lo)/n), the last one hi (numpy.linspace)"""
    lo, hi = np.float64(c) - np.float64(h), np.float64(c) + np.float64(h)
    e = lo + np.arange(n + 1, dtype=np.float64) * ((hi - lo) / np.float64(n))
    e[-1] = hi
    return e


def bin_of(e, v):
    """searchsorted(e, v, 'right') - 1, the last edge in the last bin; -1 outside and for NaN"""
    v = np.asarray(v, dtype=np.float64)
    b = np.searchsorted(e, v, 'right') - 1
    b = np.where(v == e[-1], len(e) - 2, b)
    return np.where((v >= e[0]) & (v <= e[-1]), b, -1)


def scale_exp(vmax, N):
    """61 - ceil(log2(N)) - E with vmax = f * 2^E, f in [0.5, 1), clamped to [-1000, 1000]; 0 where
    the map has no usable ray (vmax None) or vmax == 0"""
    if vmax is None or not vmax > 0.0:
        return 0
    _f, E = np.frexp(np.float64(vmax))
    return int(min(1000, max(-1000, 61 - (int(N) - 1).bit_length() - int(E))))


def values(status, weight, factor):
    """per ray: (usable, bad, v) -- v = weight * factor of the OK rays (absent operands are 1)"""
    status = np.asarray(status)
    ok = status == OK
    w = np.ones(status.shape[0]) if weight is None else np.asarray(weight, dtype=np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        v = w * np.float64(1.0 if factor is None else factor)
        good = (w >= 0.0) & np.isfinite(w) & np.isfinite(v)
    return ok & good, ok & ~good, np.where(ok & good, v, 0.0)


def weighted_maps(xs, ys, statuses, weights, item_factor, item_map, n_maps, window, nbx, nby):
    """items i = 0 .. n - 1 with positions xs[i], ys[i] [R], statuses[i] [R] and weights[i] [R] (or
    ``weights`` None) -> (wmaps int64 [n_maps, nbx, nby], counts uint32 likewise, scale_exp int32
    [n_maps], item DTYPE [n])"""
    n = len(xs)
    R = len(xs[0])
    imap = list(range(n)) if item_map is None else [int(m) for m in item_map]
    window = np.broadcast_to(np.asarray(window, dtype=np.float64), (n_maps, 4))
    parts = [values(statuses[i], None if weights is None else weights[i],
                    None if item_factor is None else item_factor[i]) for i in range(n)]
    exps = np.zeros(n_maps, np.int32)
    for m in range(n_maps):
        mine = [i for i in range(n) if imap[i] == m]
        vs = [parts[i][2][parts[i][0]] for i in mine]
        vs = np.concatenate(vs) if vs else np.zeros(0)
        exps[m] = scale_exp(vs.max() if vs.size else None, R * len(mine))
    wmaps = np.zeros((n_maps, nbx, nby), np.int64)
    counts = np.zeros((n_maps, nbx, nby), np.uint32)
    item = np.zeros(n, DTYPE)
    for i in range(n):
        m = imap[i]
        use, bad, v = parts[i]
        q = np.rint(np.ldexp(v, int(exps[m]))).astype(np.int64)
        cx, cy, hx, hy = window[m]
        bx = bin_of(edges(cx, hx, nbx), np.where(use, xs[i], np.nan))
        by = bin_of(edges(cy, hy, nby), np.where(use, ys[i], np.nan))
        inside = use & (bx >= 0) & (by >= 0)
        outside = use & ~inside
        np.add.at(wmaps[m], (bx[inside], by[inside]), q[inside])
        np.add.at(counts[m], (bx[inside], by[inside]), 1)
        item[i] = (inside.sum(), outside.sum(), bad.sum(), q[inside].sum(), q[outside].sum())
    return wmaps, counts, exps, item
