"""include/lara_depthsurface.h restated in numpy, twice: in fp32 in the written order (what the kernels must give bit
for bit where the header fixes every operation) and in float64 on the same fp32 inputs (the true values of the formulas), plus
the set of (sample, view) decisions of the observation test that are AMBIGUOUS: a comparison of it, evaluated in float64, lies
within 2^-18 relative of the magnitudes it compares, so that the fp32 evaluation may legitimately land on either side.

The inputs of both are the fp32 arrays the library receives: depth [V,H,W], k [V,4] = fx, fy, cx, cy, pose [V,16]."""
import numpy as np

U = 2.0 ** -24
EPS = 2.0 ** -18
MAX_CELLS = 1 << 27
ROW = 13


def cameras(ixt, c2w, invert=False):
    """fp32 (k [V,4], pose [V,16]) of float64 ixt [V,3,3] and c2w [V,4,4]; ``invert``: the float64 inverse, rounded once."""
    K, M = np.asarray(ixt, np.float64), np.asarray(c2w, np.float64)
    k = np.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], axis=1).astype(np.float32)
    return k, (np.linalg.inv(M) if invert else M).reshape(-1, 16).astype(np.float32)


def nonzero(mask, shape):
    """`.bool()` of a mask of any dtype (a float -0 is zero, a NaN is not); None: all ones."""
    return np.ones(shape, bool) if mask is None else np.asarray(mask) != 0


def valid(depth, mask, depth_max=np.inf):
    d = np.asarray(depth, np.float32)
    with np.errstate(invalid="ignore"):
        return nonzero(mask, d.shape) & np.isfinite(d) & (d > 0) & (d <= np.float32(depth_max))


def selected(depth, mask, stride=1, depth_max=np.inf):
    V, H, W = depth.shape
    grid = ((np.arange(H) % stride == 0)[:, None] & (np.arange(W) % stride == 0)[None, :])[None]
    return valid(depth, mask, depth_max) & grid


def points_map(depth, k, pose, dtype):
    """P(v, y, x) of every pixel, [V,H,W,3] of ``dtype`` (np.float32: the written order; np.float64: the same formula, true),
    and the sum of the magnitudes added, [V,H,W,3] float64 (what the rounding error scales with)."""
    f = dtype
    V, H, W = depth.shape
    d = np.asarray(depth, np.float32).astype(f)
    k, r = np.asarray(k, np.float32).astype(f), np.asarray(pose, np.float32).astype(f).reshape(V, 4, 4)
    x, y = np.arange(W, dtype=np.float32).astype(f)[None, None, :], np.arange(H, dtype=np.float32).astype(f)[None, :, None]
    kk = k[:, :, None, None]
    with np.errstate(all="ignore"):
        a = ((x + f(0.5)) - kk[:, 2]) / kk[:, 0]
        b = ((y + f(0.5)) - kk[:, 3]) / kk[:, 1]
        px, py = a * d, b * d
        out, mag = np.empty((V, H, W, 3), f), np.empty((V, H, W, 3), np.float64)
        for i in range(3):
            R = r[:, i, :, None, None]
            t0, t1, t2 = R[:, 0] * px, R[:, 1] * py, R[:, 2] * d
            out[..., i] = ((t0 + t1) + t2) + R[:, 3]
            mag[..., i] = np.abs(t0.astype(np.float64)) + np.abs(t1) + np.abs(t2) + np.abs(R[:, 3])
    return out, mag


def unit64(c):
    """c / |c| in float64, (0, 0, 0) where |c| is 0 or not finite."""
    c = np.asarray(c, np.float64)
    with np.errstate(all="ignore"):
        n = np.sqrt((c[..., 0] * c[..., 0] + c[..., 1] * c[..., 1]) + c[..., 2] * c[..., 2])
        ok = np.isfinite(n) & (n > 0)
        return np.where(ok[..., None], c / np.where(ok, n, 1.0)[..., None], 0.0)


def depth_normals(depth, mask, k, pose, depth_max=np.inf, jump=np.inf):
    """(normal map [V,H,W,3] float64 from the fp32 points, applies [V,H,W] bool): the header's NORMALS_DEPTH rule."""
    d = np.asarray(depth, np.float32)
    V, H, W = d.shape
    P = points_map(d, k, pose, np.float32)[0].astype(np.float64)
    ok = valid(d, mask, depth_max)
    applies = np.zeros((V, H, W), bool)
    c = np.zeros((V, H, W, 3))
    if H >= 3 and W >= 3:
        inner = (slice(None), slice(1, H - 1), slice(1, W - 1))
        nb = [(slice(None), slice(2, H), slice(1, W - 1)), (slice(None), slice(0, H - 2), slice(1, W - 1)),
              (slice(None), slice(1, H - 1), slice(2, W)), (slice(None), slice(1, H - 1), slice(0, W - 2))]
        app = ok[inner].copy()
        with np.errstate(invalid="ignore"):
            for s in nb:
                app &= ok[s] & (np.abs(d[s] - d[inner]) <= np.float32(jump))          # (an fp32 difference)
        with np.errstate(all="ignore"):
            a, b = P[nb[0]] - P[nb[1]], P[nb[2]] - P[nb[3]]
            cc = np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                           a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)
        applies[inner] = app
        c[inner] = np.where(app[..., None], cc, 0.0)
    return unit64(c), applies


def backproject(depth, mask, k, pose, stride=1, depth_max=np.inf, normals=None, jump=np.inf):
    """dict: pixel [N] int64 (ascending g), points32 [N,3] fp32 (bit-exact expectation), points64 and mag [N,3] float64,
    normals [N,3] float64 or None (``normals``: None, "depth" or a map [V,H,W,3]), applies [N] bool (depth mode)."""
    sel = selected(depth, mask, stride, depth_max).reshape(-1)
    pixel = np.nonzero(sel)[0].astype(np.int64)
    p32 = points_map(depth, k, pose, np.float32)[0].reshape(-1, 3)[pixel]
    p64, mag = points_map(depth, k, pose, np.float64)
    out = {"pixel": pixel, "points32": p32, "points64": p64.reshape(-1, 3)[pixel], "mag": mag.reshape(-1, 3)[pixel], "normals": None,
           "applies": None}
    if isinstance(normals, str):
        n, app = depth_normals(depth, mask, k, pose, depth_max, jump)
        out["normals"], out["applies"] = n.reshape(-1, 3)[pixel], app.reshape(-1)[pixel]
    elif normals is not None:
        out["normals"] = unit64(np.asarray(normals, np.float32).reshape(-1, 3)[pixel])
    return out


def thin(points, voxel, max_cells=MAX_CELLS):
    """(kept_index [N'] int64, dropped): fp32 cells in the written order; the smallest index of each occupied cell, ascending."""
    P = np.asarray(points, np.float32).reshape(-1, 3)
    fin = np.isfinite(P).all(axis=1)
    idx = np.nonzero(fin)[0]
    if len(idx) == 0:
        return np.zeros(0, np.int64), int((~fin).sum())
    Q = P[idx]
    lo = Q.min(axis=0)
    with np.errstate(over="ignore"):
        f = np.floor((Q - lo) / np.float32(voxel))
    cell = np.where(f < 2.0 ** 27, f, 2.0 ** 27).astype(np.int64)
    R = cell.max(axis=0) + 1
    if int(R[0]) * int(R[1]) * int(R[2]) > max_cells:
        raise ValueError("depthsurface_restate: more cells than max_cells")
    word = (cell[:, 2] * R[1] + cell[:, 1]) * R[0] + cell[:, 0]
    _, first = np.unique(word, return_index=True)
    return idx[np.sort(first)].astype(np.int64), int((~fin).sum())


def observe(points, depth, mask, k, w2c, tau, background_is_free=True, depth_max=np.inf, dtype=np.float64):
    """(seen [N] int64, ambiguous [N,V] bool): the header's observation test in ``dtype`` arithmetic.  ``ambiguous`` marks the
    (sample, view) pairs where a comparison the float64 evaluation REACHES lies within EPS of the magnitudes it compares:
    z_c against 0 (magnitude: the sum of the absolute summands of z_c), u and w against 0, W, H and the nearest integer (magnitude:
    what the errors of the projected summands, of z_c and of the principal point add up to), z_c - d against tau (magnitude: the
    summands of z_c, d and tau).  Computed from the float64 values whatever ``dtype`` is."""
    f = dtype
    tau = np.float32(tau)          # (the library takes it as a float)
    P = np.asarray(points, np.float32)
    d32 = np.asarray(depth, np.float32)
    V, H, W = d32.shape
    ok_pix = valid(d32, mask, depth_max)
    N = len(P)
    seen = np.zeros(N, np.int64)
    amb = np.zeros((N, V), bool)
    fin = np.isfinite(P).all(axis=1)
    kk, ww = np.asarray(k, np.float32), np.asarray(w2c, np.float32).reshape(V, 4, 4)
    with np.errstate(all="ignore"):
        for v in range(V):
            res = {}
            for g in (f, np.float64):
                x, y, z = (P[:, j].astype(g) for j in range(3))
                Wm, kv = ww[v].astype(g), kk[v].astype(g)
                q = [((Wm[i, 0] * x + Wm[i, 1] * y) + Wm[i, 2] * z) + Wm[i, 3] for i in range(3)]
                S = [np.abs(Wm[i, 0] * x) + np.abs(Wm[i, 1] * y) + np.abs(Wm[i, 2] * z) + np.abs(Wm[i, 3]) for i in range(3)]
                zc = q[2]
                front = fin & (zc > 0)
                u, w = (q[0] * kv[0]) / zc + kv[2], (q[1] * kv[1]) / zc + kv[3]
                inside = front & (u >= 0) & (u < g(W)) & (w >= 0) & (w < g(H))
                col = np.where(inside, np.floor(u), 0).astype(np.int64)
                row = np.where(inside, np.floor(w), 0).astype(np.int64)
                dd = d32[v, row, col].astype(g)
                on = inside & ok_pix[v, row, col]
                obs = np.where(on, zc <= dd + g(tau), inside & bool(background_is_free))
                res[g] = (obs, S, q, zc, front, u, w, inside, on, dd, kv)
            obs, S, q, zc, front, u, w, inside, on, dd, kv = res[np.float64]
            a = fin & (np.abs(zc) <= EPS * S[2])
            az = np.abs(zc)
            Mu = (S[0] * kv[0]) / az + np.abs(q[0] * kv[0] / zc) * (S[2] / az) + np.abs(kv[2])
            Mw = (S[1] * kv[1]) / az + np.abs(q[1] * kv[1] / zc) * (S[2] / az) + np.abs(kv[3])
            near_u = np.minimum.reduce([np.abs(u), np.abs(u - W), np.abs(u - np.round(u))]) <= EPS * Mu
            near_w = np.minimum.reduce([np.abs(w), np.abs(w - H), np.abs(w - np.round(w))]) <= EPS * Mw
            # a sample clearly outside on one axis is decided by that axis alone; otherwise either axis may tip the pixel
            clear_out = front & (((u < 0) | (u >= W)) & ~near_u | ((w < 0) | (w >= H)) & ~near_w)
            a |= front & ~clear_out & (near_u | near_w)
            a |= on & (np.abs((zc - dd) - np.float64(tau)) <= EPS * (S[2] + np.abs(dd) + np.float64(tau)))
            amb[:, v] = a & fin
            seen |= np.where(res[f][0], np.int64(1) << np.int64(v), np.int64(0))
    return seen, amb


def bits(seen, V):
    """[N,V] bool of the int64 masks."""
    return ((np.asarray(seen, np.int64)[:, None] >> np.arange(V, dtype=np.int64)[None, :]) & 1).astype(bool)


def reduce_row(dist, index, M, keep, nq, nt, thresholds):
    """(row [ROW] float64 of lara_depthsurface_reduce from its fp32 inputs: exact counts, float64 sums; the sums of the absolute
    summands of [1], [2], [3], for the bars)."""
    d32 = np.asarray(dist, np.float32)
    idx = np.asarray(index, np.int64)
    k = np.ones(len(d32), bool) if keep is None else np.asarray(keep) != 0
    d = d32.astype(np.float64)
    row = np.zeros(ROW)
    row[0], row[1], row[2] = k.sum(), d[k].sum(), (d[k] * d[k]).sum()
    if nq is not None and nt is not None:
        inr = (idx >= 0) & (idx < M)
        a, b = np.asarray(nq, np.float32).astype(np.float64), np.asarray(nt, np.float32).astype(np.float64)[np.where(inr, idx, 0)]
        pair = k & inr & (a != 0).any(axis=1) & (b != 0).any(axis=1)
        dots = np.abs((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2])
        row[3], row[4] = dots[pair].sum(), pair.sum()
    for j, t in enumerate(thresholds):
        row[5 + j] = (k & (d32 <= np.float32(t))).sum()
    return row
