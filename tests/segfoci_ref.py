"""TEST INFRASTRUCTURE: the NumPy restatement of rox_segment_foci (include/roxtrace.h), with the
same partition and the same merge order, every step one float64 operation:

* the rays of an item in tiles of 1024; thread t (0 .. 255) of tile T holds rays
  1024*T + 256*j + t, j = 0 .. 3; wave v of the tile is its threads 64*v .. 64*v + 63
* a counted ray is a record of its own (W = w, means a and b, moments 0); a thread merges its
  counted rays in the order of j into an empty record
* a wave: for o = 32 .. 1 every lane merges its value with lane ^ o's (its own first)
* an (item, slot): thread t of 256 merges waves t, t + 256, .. in that order into an empty record,
  then for h = 128 .. 1 thread t < h merges its value with thread t + h's
* the merge of P with Q is Chan, Golub and LeVeque's pairwise update, weighted, P first

``segment_foci`` returns the records, and for the tests' bounds the absolute sums of each
sum's terms and an evaluation of the same quantities in ``numpy.longdouble`` (plain sums, no
partition)."""
import numpy as np

OK = 0
TILE, BLOCK, RAYS = 1024, 256, 4
DTYPE = np.dtype([(name, np.int64) for name in ('n', 'n_flat', 'n_bad', 'n_in')] +
                 [('w_sum', np.float64), ('w_in', np.float64), ('a_mean', np.float64, (2,)),
                  ('b_mean', np.float64, (2,))] +
                 [(name, np.float64) for name in ('m_aa', 'm_ab', 'm_bb', 'z_in_min', 'z_in_max', 'z_out_min',
                                                  'z_out_max')])
FLOATS = ('w', 'w_in', 'ax', 'ay', 'bx', 'by', 'maa', 'mab', 'mbb')
COUNTS = ('n', 'n_flat', 'n_bad', 'n_in')


def empty(shape):
    acc = {k: np.zeros(shape) for k in FLOATS}
    acc.update({k: np.zeros(shape, np.int64) for k in COUNTS})
    acc.update(zi_min=np.full(shape, np.inf), zi_max=np.full(shape, -np.inf),
               zo_min=np.full(shape, np.inf), zo_max=np.full(shape, -np.inf))
    return acc


def merge(P, Q):
    """P merged with Q, P's rays first (elementwise over arrays of records)"""
    with np.errstate(all='ignore'):
        both = (Q['w'] > 0.0) & (P['w'] > 0.0)
        take = (Q['w'] > 0.0) & ~(P['w'] > 0.0)
        ww = P['w'] + Q['w']
        f = Q['w'] / ww
        g = P['w'] * f
        d = {k: Q[k] - P[k] for k in ('ax', 'ay', 'bx', 'by')}
        out = {}
        for k in ('ax', 'ay', 'bx', 'by'):
            out[k] = np.where(both, P[k] + d[k] * f, np.where(take, Q[k], P[k]))
        out['maa'] = np.where(both, (P['maa'] + Q['maa']) + (d['ax'] * d['ax'] + d['ay'] * d['ay']) * g,
                              np.where(take, Q['maa'], P['maa']))
        out['mab'] = np.where(both, (P['mab'] + Q['mab']) + (d['ax'] * d['bx'] + d['ay'] * d['by']) * g,
                              np.where(take, Q['mab'], P['mab']))
        out['mbb'] = np.where(both, (P['mbb'] + Q['mbb']) + (d['bx'] * d['bx'] + d['by'] * d['by']) * g,
                              np.where(take, Q['mbb'], P['mbb']))
        out['w'] = np.where(both, ww, np.where(take, Q['w'], P['w']))
        out['w_in'] = P['w_in'] + Q['w_in']
        for k in ('zi_min', 'zo_min'):
            out[k] = np.minimum(P[k], Q[k])
        for k in ('zi_max', 'zo_max'):
            out[k] = np.maximum(P[k], Q[k])
        for k in COUNTS:
            out[k] = P[k] + Q[k]
    return out


def ray_terms(seg_k, use, window):
    """the per-ray quantities of one slot for the rays in ``use``: (cnt, ax, ay, bx, by, z, zo, inside)"""
    x, y, z, L, M, N, dst = (seg_k[i] for i in range(7))
    with np.errstate(all='ignore'):
        cnt = use & (N != 0.0)
        Ns = np.where(cnt, N, 1.0)
        bx = np.where(cnt, L / Ns, 0.0)
        by = np.where(cnt, M / Ns, 0.0)
        ax = np.where(cnt, x - z * bx, 0.0)
        ay = np.where(cnt, y - z * by, 0.0)
        zo = z + dst * N
        inside = cnt if window is None else cnt & (np.abs(ax) <= window[0]) & (np.abs(ay) <= window[1])
    return cnt, ax, ay, bx, by, z, zo, inside


def segment_foci(seg, status, weight=None, window=None):
    """``seg`` [n_seg, 10, R], ``status`` [R], ``weight`` [R] or None, ``window`` (hx, hy) or None
    -> (records [n_seg] of DTYPE, abs_sums, exact): ``abs_sums[name][k]`` the sum of the absolute
    values of the terms of sum ``name`` (w_sum, w_in, sa [2], sb [2], m_aa, m_ab, m_bb: the first
    moments' terms w*a, the second moments' about the frame's origin), ``exact[name][k]`` the
    quantity of the record evaluated in longdouble"""
    n_seg, _ten, R = seg.shape
    n_tiles = (R + TILE - 1) // TILE
    pad = n_tiles * TILE
    ok = np.zeros(pad, bool)
    ok[:R] = np.asarray(status) == OK
    w = np.ones(pad)
    if weight is not None:
        w[:R] = np.where(ok[:R], weight, 1.0)
    with np.errstate(invalid='ignore'):
        good = ok & (w >= 0.0) & (w <= np.finfo(np.float64).max)
    bad = ok & ~good
    w = np.where(good, w, 0.0)
    shape = (n_tiles, RAYS, BLOCK)                          # ray = T*1024 + j*256 + t
    rec = np.zeros(n_seg, DTYPE)
    abs_sums = {k: np.zeros(n_seg) for k in ('w_sum', 'w_in', 'm_aa', 'm_ab', 'm_bb')}
    abs_sums.update(sa=np.zeros((n_seg, 2)), sb=np.zeros((n_seg, 2)))
    exact = {k: np.full(n_seg, np.nan, np.longdouble) for k in ('w_sum', 'w_in', 'm_aa', 'm_ab', 'm_bb')}
    exact.update(a_mean=np.full((n_seg, 2), np.nan, np.longdouble), b_mean=np.full((n_seg, 2), np.nan, np.longdouble))
    wj = w.reshape(shape)
    for k in range(n_seg):
        sk = np.zeros((7, pad))
        sk[:, :R] = np.where(good[None, :R], seg[k, :7, :], 0.0)
        cnt, ax, ay, bx, by, z, zo, inside = ray_terms(sk, good, window)
        c3, in3 = cnt.reshape(shape), inside.reshape(shape)
        v = {'ax': ax.reshape(shape), 'ay': ay.reshape(shape), 'bx': bx.reshape(shape), 'by': by.reshape(shape)}
        z3, zo3 = z.reshape(shape), zo.reshape(shape)
        t = empty((n_tiles, BLOCK))
        t['n_bad'] = bad.reshape(shape).sum(axis=1)
        t['n_flat'] = (good & ~cnt).reshape(shape).sum(axis=1)
        for j in range(RAYS):
            c = c3[:, j]
            q = empty((n_tiles, BLOCK))                     # empty where the ray does not count
            q['w'] = np.where(c, wj[:, j], 0.0)
            q['w_in'] = np.where(in3[:, j], wj[:, j], 0.0)
            for name in v:
                q[name] = np.where(c, v[name][:, j], 0.0)
            q['zi_min'] = np.where(c, z3[:, j], np.inf)
            q['zi_max'] = np.where(c, z3[:, j], -np.inf)
            q['zo_min'] = np.where(c, zo3[:, j], np.inf)
            q['zo_max'] = np.where(c, zo3[:, j], -np.inf)
            q['n'] = c.astype(np.int64)
            q['n_in'] = in3[:, j].astype(np.int64)
            t = merge(t, q)
        # the waves: [n_tiles * 4, 64], the butterfly, lane 0
        wv = {name: arr.reshape(n_tiles * 4, 64) for name, arr in t.items()}
        lanes = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            wv = merge(wv, {name: arr[:, lanes ^ o] for name, arr in wv.items()})
        part = {name: arr[:, 0] for name, arr in wv.items()}
        n_waves = n_tiles * 4
        # the finishing kernel
        m = empty((BLOCK,))
        for w0 in range(0, n_waves, BLOCK):
            q = empty((BLOCK,))
            c = min(BLOCK, n_waves - w0)
            for name in q:
                q[name][:c] = part[name][w0:w0 + c]
            m = merge(m, q)
        h = BLOCK // 2
        while h > 0:
            lo = merge({name: arr[:h] for name, arr in m.items()}, {name: arr[h:2 * h] for name, arr in m.items()})
            for name in m:
                m[name][:h] = lo[name]
            h //= 2
        r = rec[k]
        for name in COUNTS:
            r[name] = m[name][0]
        any_ = m['n'][0] > 0 and m['w'][0] > 0.0
        r['w_sum'], r['w_in'] = m['w'][0], m['w_in'][0]
        r['a_mean'] = (m['ax'][0], m['ay'][0]) if any_ else np.nan
        r['b_mean'] = (m['bx'][0], m['by'][0]) if any_ else np.nan
        for name, src in (('m_aa', 'maa'), ('m_ab', 'mab'), ('m_bb', 'mbb')):
            r[name] = m[src][0] if any_ else np.nan
        r['z_in_min'], r['z_in_max'] = m['zi_min'][0], m['zi_max'][0]
        r['z_out_min'], r['z_out_max'] = m['zo_min'][0], m['zo_max'][0]

        # the absolute sums and the longdouble evaluation, over the counted rays in any order
        ld = np.longdouble
        wl = w[cnt].astype(ld)
        al = np.stack([ax[cnt], ay[cnt]]).astype(ld)
        bl = np.stack([bx[cnt], by[cnt]]).astype(ld)
        abs_sums['w_sum'][k] = float(np.abs(wl).sum())
        abs_sums['w_in'][k] = float(np.abs(w[inside]).astype(ld).sum())
        abs_sums['sa'][k] = (np.abs(wl * al)).sum(axis=1).astype(np.float64)
        abs_sums['sb'][k] = (np.abs(wl * bl)).sum(axis=1).astype(np.float64)
        abs_sums['m_aa'][k] = float((wl * (al * al).sum(axis=0)).sum())
        abs_sums['m_ab'][k] = float((wl * np.abs(al * bl).sum(axis=0)).sum())
        abs_sums['m_bb'][k] = float((wl * (bl * bl).sum(axis=0)).sum())
        W = wl.sum()
        exact['w_sum'][k] = W
        exact['w_in'][k] = w[inside].astype(ld).sum()
        if cnt.any() and W > 0:
            am, bm = (wl * al).sum(axis=1) / W, (wl * bl).sum(axis=1) / W
            ea, eb = al - am[:, None], bl - bm[:, None]
            exact['a_mean'][k], exact['b_mean'][k] = am, bm
            exact['m_aa'][k] = (wl * (ea * ea).sum(axis=0)).sum()
            exact['m_ab'][k] = (wl * (ea * eb).sum(axis=0)).sum()
            exact['m_bb'][k] = (wl * (eb * eb).sum(axis=0)).sum()
    return rec, abs_sums, exact


def derive(rec):
    """(zeta*, smallest mean-square radius, mean-square radius at z = 0) of records, in longdouble"""
    ld = np.longdouble
    maa, mab, mbb, w = (rec[k].astype(ld) for k in ('m_aa', 'm_ab', 'm_bb', 'w_sum'))
    with np.errstate(all='ignore'):
        return -mab / mbb, (maa - mab * mab / mbb) / w, maa / w
