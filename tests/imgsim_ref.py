"""TEST INFRASTRUCTURE: the NumPy restatement of rox_varying_blur and rox_image_warp
(include/roxtrace.h) -- every step one NumPy float64 operation in the header's order: the hat
weights from one quotient, the weighted source scene * (wy * wx), one product and one sum per node
and tap, nodes and taps in row-major order; the warp's two bilinear blends.  NumPy does not fuse a
multiply into an add, so the device must reproduce every value (compared with ==: a skipped zero
term can change the sign of a zero and nothing else)."""
import numpy as np

EDGE_ZERO, EDGE_REPLICATE = 0, 1


def hat_cells(coord, node):
    """the cell k and fraction t of every coordinate among the strictly increasing ``node``: k = 0,
    t = 0 before the first node or with one node; k = len - 1, t = 0 from the last node on; else
    node[k] <= coord < node[k + 1] and t = (coord - node[k]) / (node[k + 1] - node[k])"""
    coord = np.asarray(coord, dtype=np.float64)
    node = np.asarray(node, dtype=np.float64)
    g = len(node)
    k = np.zeros(coord.shape, dtype=np.int64)
    t = np.zeros(coord.shape, dtype=np.float64)
    if g == 1:
        return k, t
    last = coord >= node[-1]
    k[last] = g - 1
    mid = ~(coord < node[0]) & ~last
    km = np.searchsorted(node, coord[mid], 'right') - 1
    k[mid] = km
    t[mid] = (coord[mid] - node[km]) / (node[km + 1] - node[km])
    return k, t


def hat_weights(n, node):
    """[len(node), n]: the hat weight of every node at the pixels 0 .. n - 1"""
    k, t = hat_cells(np.arange(n, dtype=np.float64), node)
    w = np.zeros((len(node), n), dtype=np.float64)
    idx = np.arange(n)
    w[k, idx] = 1.0 - t
    up = k + 1 < len(node)
    w[k[up] + 1, idx[up]] = t[up]
    return w


def varying_blur(scene, psf, node_y, node_x, edge=EDGE_ZERO):
    """scene [C, H, W], psf [C, GY, GX, S, S] -> [C, H, W]; vectorised over the pixels, one NumPy
    product and one sum per node and tap.  A node none of whose weights is non-zero is skipped."""
    scene = np.asarray(scene, dtype=np.float64)
    psf = np.asarray(psf, dtype=np.float64)
    C, H, W = scene.shape
    _c, GY, GX, S, _s = psf.shape
    r = (S - 1) // 2
    wy, wx = hat_weights(H, node_y), hat_weights(W, node_x)
    out = np.zeros((C, H, W), dtype=np.float64)
    for c in range(C):
        acc = np.zeros((H, W), dtype=np.float64)
        for ky in range(GY):
            for kx in range(GX):
                w = wy[ky][:, None] * wx[kx][None, :]
                if not w.any():
                    continue
                sw = scene[c] * w
                # source (i - (a - r), j - (b - r)) is p[i + 2r - a, j + 2r - b]
                p = np.pad(sw, r, mode='edge' if edge == EDGE_REPLICATE else 'constant')
                for a in range(S):
                    for b in range(S):
                        acc = acc + p[2 * r - a:2 * r - a + H, 2 * r - b:2 * r - b + W] * psf[c, ky, kx, a, b]
        out[c] = acc
    return out


def varying_blur_loop(scene, psf, node_y, node_x, edge=EDGE_ZERO):
    """the same sums pixel by pixel, terms of zero hat weight and sources outside the picture (zero
    edge) skipped -- the form a device kernel takes"""
    scene = np.asarray(scene, dtype=np.float64)
    C, H, W = scene.shape
    _c, GY, GX, S, _s = psf.shape
    r = (S - 1) // 2
    wy, wx = hat_weights(H, node_y), hat_weights(W, node_x)
    out = np.zeros((C, H, W), dtype=np.float64)
    for c in range(C):
        for i in range(H):
            for j in range(W):
                acc = np.float64(0.0)
                for ky in range(GY):
                    for kx in range(GX):
                        for a in range(S):
                            si = i - (a - r)
                            if edge == EDGE_REPLICATE:
                                si = min(max(si, 0), H - 1)
                            elif not 0 <= si < H:
                                continue
                            for b in range(S):
                                sj = j - (b - r)
                                if edge == EDGE_REPLICATE:
                                    sj = min(max(sj, 0), W - 1)
                                elif not 0 <= sj < W:
                                    continue
                                w = wy[ky, si] * wx[kx, sj]
                                if w == 0.0:
                                    continue
                                acc = acc + (scene[c, si, sj] * w) * psf[c, ky, kx, a, b]
                out[c, i, j] = acc
    return out


def _node_blend(v, k, ty, l, tx):
    """the header's bilinear blend of node values v [GY, GX] at the cells (k, ty) x (l, tx)"""
    GY, GX = v.shape
    k1, l1 = np.minimum(k + 1, GY - 1), np.minimum(l + 1, GX - 1)
    k, k1, ty = k[:, None], k1[:, None], ty[:, None]
    l, l1, tx = l[None, :], l1[None, :], tx[None, :]
    return (1.0 - ty) * ((1.0 - tx) * v[k, l] + tx * v[k, l1]) + ty * ((1.0 - tx) * v[k1, l] + tx * v[k1, l1])


def image_warp(img, node_y, node_x, disp):
    """img [C, H, W], disp [GY, GX, 2] = (dy, dx) -> [C, H, W]"""
    img = np.asarray(img, dtype=np.float64)
    disp = np.asarray(disp, dtype=np.float64)
    C, H, W = img.shape
    k, ty = hat_cells(np.arange(H, dtype=np.float64), node_y)
    l, tx = hat_cells(np.arange(W, dtype=np.float64), node_x)
    dy = _node_blend(disp[:, :, 0], k, ty, l, tx)
    dx = _node_blend(disp[:, :, 1], k, ty, l, tx)
    y = np.arange(H, dtype=np.float64)[:, None] + dy
    x = np.arange(W, dtype=np.float64)[None, :] + dx
    y0, x0 = np.floor(y), np.floor(x)
    fy, fx = y - y0, x - x0

    def tap(c, yy, xx):
        ok = (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
        yi = np.where(ok, yy, 0).astype(np.int64)
        xi = np.where(ok, xx, 0).astype(np.int64)
        return np.where(ok, img[c, yi, xi], 0.0)

    out = np.empty((C, H, W), dtype=np.float64)
    for c in range(C):
        out[c] = (1.0 - fy) * ((1.0 - fx) * tap(c, y0, x0) + fx * tap(c, y0, x0 + 1.0)) + \
            fy * ((1.0 - fx) * tap(c, y0 + 1.0, x0) + fx * tap(c, y0 + 1.0, x0 + 1.0))
    return out
