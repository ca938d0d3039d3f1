"""include/lara_meshrender.h restated in float64 and exact integers (numpy int64: every product stays below 2^47), without
the library or a device.  The reference of tests/test_meshrender.py and tests/test_meshrender_gpu.py.

``snap_vertices`` is stage V; ``rasterize`` is stages R and S from a stage-V array (snapped x, y and view z) -- its own, or
the device's, in which case coverage and tie-breaking are integer-exact by construction and only depths are compared in
floating point.  Every float64 result comes with the fp32 bound of its operands, first order in u = 2^-24, derived where it is
computed.  ``mutate`` turns one rule of the header into a wrong one (tests: each mutation fails exactly what it touches).
"""
import numpy as np

U = 2.0 ** -24
SUB, RANGE, FAR = 256, 1 << 22, 1 << 30
DEPTH_ROUNDINGS = 8.0       # r_i, float(w_i), q_i: 3u on every (non-negative) term; two adds; float(area); the divide: 7u, + slack


def snap_vertices(vertices, view, proj, H, W):
    """Stage V in float64 from the fp32 operands.  Returns (sx, sy int64 [Nv], z float64 [Nv], z_bound [Nv]): z is a sum of
    four fp32 terms t_k = V[k][2] p_k (the last one exact), rounded after each product and each of three adds:
    |z_fp32 - z| <= (1 + 3) u sum |t_k|, taken as 4.5 u sum |t_k| for the second-order terms."""
    p = np.asarray(vertices, np.float32).astype(np.float64).reshape(-1, 3)
    M = np.asarray(proj, np.float32).astype(np.float64).reshape(4, 4)
    V = np.asarray(view, np.float32).astype(np.float64).reshape(4, 4)
    h = p @ M[:3] + M[3]
    tz = np.concatenate([p * V[:3, 2], np.full((len(p), 1), V[3, 2])], 1)
    z = tz.sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        px = ((h[:, 0] / h[:, 3] + 1.0) * W - 1.0) * 0.5
        py = ((h[:, 1] / h[:, 3] + 1.0) * H - 1.0) * 0.5

    def snap(v):
        v = v * SUB
        far = ~(np.abs(v) < FAR)
        return np.where(far, FAR, np.rint(np.where(far, 0.0, v))).astype(np.int64)
    return snap(px), snap(py), z, 4.5 * U * np.abs(tz).sum(1)


def _edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def classify(sx, sy, z, triangles, znear):
    """(class [T]: 0 drawn, 1 behind, 2 degenerate, 3 out of range; ordered [T,3]: the indices with area > 0; area [T])."""
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    behind = ~(z[t] > znear).all(1)
    rng = (np.abs(sx[t]) > RANGE).any(1) | (np.abs(sy[t]) > RANGE).any(1)
    ok = ~behind & ~rng
    x, y = np.where(ok[:, None], sx[t], 0), np.where(ok[:, None], sy[t], 0)
    area = _edge(x[:, 0], y[:, 0], x[:, 1], y[:, 1], x[:, 2], y[:, 2])
    cls = np.where(behind, 1, np.where(rng, 3, np.where(area == 0, 2, 0)))
    ordered = np.where((area < 0)[:, None], t[:, [0, 2, 1]], t)
    return cls, ordered, np.abs(area)


def rasterize(sx, sy, z, triangles, H, W, znear, vertices=None, colors=None, proj=None, eye=None, albedo=(0.25, 0.5, 0.8),
              background=(0.722, 0.376, 0.161), ambient=0.25, diffuse=0.75, mutate=None):
    """Stages R and S.  ``mutate``: None, 'inclusive' (every edge owns its samples), 'screen_linear' (z, not 1/z, linear on the
    screen) or 'tie_high' (a depth tie goes to the higher id).  Returns a dict of [H, W(, 3)] arrays:

      face (-1 = background), depth, depth2 (the runner-up's depth, inf where there is none), count (triangles covering the
      sample), depth_bound; with ``vertices``: normal, normal_bound, colour (float64, before quantisation; the background
      included), colour_bound (of 255 colour), faces_eye (the exact side rule agrees with the geometric one);
      info [4] = triangles drawn, behind, degenerate, out of range.

    Triangles that are copies of one another (the same ordered stage-V records) compute the same fp32 depth bit for bit, so
    their tie is exact: they are drawn once, under the group's lowest id, and do not count as each other's runner-up."""
    sx, sy, z = np.asarray(sx, np.int64), np.asarray(sy, np.int64), np.asarray(z, np.float64)
    cls, ordered, area = classify(sx, sy, z, triangles, znear)
    info = np.array([(cls == k).sum() for k in (0, 1, 2, 3)], np.int64)
    best_d = np.full((H, W), np.inf)
    second_d = np.full((H, W), np.inf)
    best_i = np.full((H, W), -1, np.int64)
    count = np.zeros((H, W), np.int64)
    groups = {}
    for t in np.nonzero(cls == 0)[0]:
        i = ordered[t]
        groups.setdefault((tuple(sx[i]), tuple(sy[i]), tuple(z[i])), []).append(int(t))
    for ids in groups.values():
        t = max(ids) if mutate == "tie_high" else min(ids)
        i = ordered[t]
        x, y = sx[i], sy[i]
        bx0, bx1 = max(int(-((-x.min()) // SUB)), 0), min(int(x.max() // SUB), W - 1)
        by0, by1 = max(int(-((-y.min()) // SUB)), 0), min(int(y.max() // SUB), H - 1)
        if bx1 < bx0 or by1 < by0:
            continue
        PX, PY = np.meshgrid(np.arange(bx0, bx1 + 1, dtype=np.int64) * SUB, np.arange(by0, by1 + 1, dtype=np.int64) * SUB)
        cov = np.ones(PX.shape, bool)
        w = []
        for a, b in ((1, 2), (2, 0), (0, 1)):
            e = _edge(x[a], y[a], x[b], y[b], PX, PY)
            dy, dx = y[b] - y[a], x[b] - x[a]
            own = mutate == "inclusive" or dy < 0 or (dy == 0 and dx > 0)
            cov &= (e > 0) | ((e == 0) & own)
            w.append(e)
        if not cov.any():
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            if mutate == "screen_linear":
                d = (w[0] * z[i[0]] + w[1] * z[i[1]] + w[2] * z[i[2]]) / float(area[t])
            else:
                d = float(area[t]) / (w[0] / z[i[0]] + w[1] / z[i[1]] + w[2] / z[i[2]])
        sl = (slice(by0, by1 + 1), slice(bx0, bx1 + 1))
        bd, bi, sd = best_d[sl], best_i[sl], second_d[sl]
        tie = (t > bi) if mutate == "tie_high" else (t < bi)
        better = cov & ((d < bd) | ((d == bd) & tie))
        second_d[sl] = np.where(better, bd, np.where(cov, np.minimum(sd, d), sd))
        best_d[sl] = np.where(better, d, bd)
        best_i[sl] = np.where(better, t, bi)
        count[sl] += cov * len(ids)
    hit = best_i >= 0
    out = {"face": best_i, "depth": np.where(hit, best_d, 0.0), "depth2": second_d, "count": count, "info": info,
           "depth_bound": DEPTH_ROUNDINGS * U * np.where(hit, best_d, 0.0), "ordered": ordered}
    if vertices is None:
        return out
    # ---- stage S on the covered pixels, all at once
    p = np.asarray(vertices, np.float32).astype(np.float64).reshape(-1, 3)
    M = np.asarray(proj, np.float32).astype(np.float64).reshape(4, 4)
    eye = np.asarray(eye, np.float32).astype(np.float64).reshape(3)
    alb0 = np.asarray(albedo, np.float32).astype(np.float64)
    bg = np.asarray(background, np.float32).astype(np.float64)
    amb, dif = float(np.float32(ambient)), float(np.float32(diffuse))
    py, px = np.nonzero(hit)
    i = ordered[best_i[hit]]                                     # [n, 3]
    X, Y = px.astype(np.int64) * SUB, py.astype(np.int64) * SUB
    w = np.stack([_edge(sx[i[:, a]], sy[i[:, a]], sx[i[:, b]], sy[i[:, b]], X, Y) for a, b in ((1, 2), (2, 0), (0, 1))], 1)
    q = w / z[i]
    b = q / q.sum(1, keepdims=True)                              # fp32: q_i 3u, s 5u, the divide u: 9u b_i
    P = p[i]                                                     # [n, 3 vertices, 3]
    ea, eb = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]                # one rounding each: u |ea|, u |eb|
    c = np.cross(ea, eb)
    # a component of c is a difference of two products of once-rounded factors: (2u + u) on each product, u on the difference,
    # all relative to |product 1| + |product 2|
    mag = np.abs(ea[:, [1, 2, 0]] * eb[:, [2, 0, 1]]) + np.abs(ea[:, [2, 0, 1]] * eb[:, [1, 2, 0]])
    clen = np.linalg.norm(c, axis=1)
    # n = c / |c|: |dn| <= |dc| / |c| (the projection off n), doubled for the second order; 4u for squares, sum, root, divide
    n_bound = 2.0 * np.linalg.norm(4.0 * U * mag, axis=1) / clen + 4.0 * U
    A = M[:3][:, [0, 1, 3]]
    sgn = 1.0 if np.linalg.det(A) < 0 else -1.0
    n = sgn * c / clen[:, None]
    S = (b[:, :, None] * P).sum(1)                               # 9u on b_i, u the product, 2u the adds: 12u sum b_i |p_i|
    S_bound = 12.0 * U * (b[:, :, None] * np.abs(P)).sum(1)
    lv = eye - S
    llen = np.linalg.norm(lv, axis=1)
    l_bound = 2.0 * np.linalg.norm(S_bound + U * np.abs(lv), axis=1) / llen + 4.0 * U
    ldir = lv / llen[:, None]
    ndl = (n * ldir).sum(1)
    ndl_bound = n_bound + l_bound + 3.0 * U                      # |n| = |l| = 1; three products and two adds of terms <= 1
    shade = amb + dif * np.maximum(ndl, 0.0)
    shade_bound = dif * ndl_bound + 2.0 * U * (amb + dif * np.abs(ndl))
    if colors is None:
        alb, alb_bound = np.broadcast_to(alb0, (len(px), 3)), np.zeros((len(px), 3))
    else:
        col = np.asarray(colors, np.float32).astype(np.float64).reshape(-1, 3)[i]
        alb = (b[:, :, None] * col).sum(1)
        alb_bound = 12.0 * U * (b[:, :, None] * np.abs(col)).sum(1)
    colour = alb * shade[:, None]
    colour_bound = np.abs(alb) * shade_bound[:, None] + shade[:, None] * alb_bound + U * np.abs(colour)
    out["normal"] = np.zeros((H, W, 3)); out["normal"][hit] = n
    out["normal_bound"] = np.zeros((H, W)); out["normal_bound"][hit] = n_bound
    out["colour"] = np.broadcast_to(bg, (H, W, 3)).copy(); out["colour"][hit] = colour
    out["colour_bound"] = np.broadcast_to(255.0 * U * np.abs(bg), (H, W, 3)).copy()
    out["colour_bound"][hit] = 255.0 * colour_bound + 255.0 * U * np.abs(colour)     # the product with 255
    out["faces_eye"] = np.ones((H, W), bool); out["faces_eye"][hit] = (n * (eye - P[:, 0])).sum(1) > 0
    return out


def quantize(colour):
    """clamp(rint(255 colour), 0, 255): np.round rounds ties to even, as the kernel's rint does."""
    return np.clip(np.round(np.asarray(colour, np.float64) * 255.0), 0, 255).astype(np.uint8)


def near_tie(res):
    """Pixels whose winner and runner-up lie closer than their fp32 depth bounds: the only ones where an fp32 rasteriser started
    from the same stage-V array may legitimately pick another triangle."""
    hit = res["face"] >= 0
    gap = res["depth2"] - res["depth"]
    return hit & (gap <= DEPTH_ROUNDINGS * U * (res["depth"] + np.where(np.isfinite(res["depth2"]), res["depth2"], 0.0)))


def tie_margin(res):
    """Per colour component: is 255 colour further from a rounding tie (k + 1/2) than its bound?  (Beyond the clamp the code is
    certain as well.)"""
    v = res["colour"] * 255.0
    dist = np.abs(v - np.floor(v) - 0.5)
    return (dist > res["colour_bound"]) | (v < -0.5 - res["colour_bound"]) | (v > 255.5 + res["colour_bound"])


def render_view(vertices, triangles, view, proj, eye, H, W, znear, colors=None, mutate=None, **shading):
    """Both stages from the vertices: (result of ``rasterize``, stage-V tuple of ``snap_vertices``)."""
    sv = snap_vertices(vertices, view, proj, H, W)
    return rasterize(sv[0], sv[1], sv[2], triangles, H, W, znear, vertices, colors, proj, eye, mutate=mutate, **shading), sv
