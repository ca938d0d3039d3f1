"""include/lara_meshtexture.h restated in numpy (int64 for the layout, float64 in the header's order for the rest):
what tests/test_meshtexture.py holds the host entries to and tests/test_meshtexture_gpu.py the kernels, as integers and bit
patterns.  Nothing here is shared with lara_amd/meshtexture.py."""
import math

import numpy as np

from tests import meshdist_restate as R

F32 = np.float32
MAX_VIEWS = 64


def atlas(T, patch=None, width=None, max_texels=None):
    """(S, C, Wa, Ha) as the module's ``atlas`` documents it."""
    def one(S):
        cells = (T + 1) // 2
        if width is not None:
            C = max(1, width // (S + 1))
        else:
            C = max(1, math.isqrt(max(0, cells * S // (S + 1) - 1)) + 1) if cells else 1
        return S, C, C * (S + 1), max(1, -(-cells // C)) * S
    if max_texels is None:
        return one(8 if patch is None else patch)
    best = None
    for S in range(3, 4097):
        L = one(S)
        if L[2] * L[3] <= max_texels:
            best = L
    return best


def owner_tables(S, C, T):
    """(face, a, b) [Ha, Wa] int64 by a plain double loop over cells and their texels; face = -1 beyond T."""
    cells = (T + 1) // 2
    Wa, Ha = C * (S + 1), max(1, -(-cells // C)) * S
    face, a, b = np.full((Ha, Wa), -1, np.int64), np.zeros((Ha, Wa), np.int64), np.zeros((Ha, Wa), np.int64)
    for c in range((Ha // S) * C):
        x0, y0 = (c % C) * (S + 1), (c // C) * S
        for j in range(S):
            for i in range(S + 1):
                even = i + j <= S - 1
                f = 2 * c + (0 if even else 1)
                face[y0 + j, x0 + i] = f if f < T else -1
                a[y0 + j, x0 + i], b[y0 + j, x0 + i] = (i, j) if even else (S - i, S - 1 - j)
    return face, a, b


def corner_uvs(layout, T):
    S, C, Wa, Ha = layout
    out = np.zeros((T, 3, 2), np.float64)
    for f in range(T):
        c = f // 2
        for k, (a, b) in enumerate(((0, 0), (S - 2, 0), (0, S - 2))):
            i, j = (S - a, S - 1 - b) if f & 1 else (a, b)
            out[f, k] = ((c % C) * (S + 1) + i + 0.5) / Wa, 1.0 - ((c // C) * S + j + 0.5) / Ha
    return out.astype(F32)


def _bary(S, a, b):
    d = np.float64(S - 2)
    b1, b2 = a / d, b / d
    b0 = (1.0 - b1) - b2
    c0 = np.where(b0 > 0, b0, 0.0)
    s = (c0 + b1) + b2
    return (b0, b1, b2), (c0 / s, b1 / s, b2 / s)


def _blend(w, p):
    return (w[0][:, None] * p[0] + w[1][:, None] * p[1]) + w[2][:, None] * p[2]


def texels(layout, V, F):
    """(face [Ha,Wa] int32, point, anchor [Ha,Wa,3] fp32)."""
    S, C, Wa, Ha = layout
    V, F = np.asarray(V, F32), np.asarray(F, np.int64).reshape(-1, 3)
    face, a, b = owner_tables(S, C, len(F))
    ok = R.valid_triangles(V, F) if len(F) else np.zeros(0, bool)
    face = np.where((face >= 0) & ok[np.maximum(face, 0)] if len(F) else False, face, -1)
    own = face >= 0
    point, anchor = np.full((Ha, Wa, 3), np.nan, F32), np.full((Ha, Wa, 3), np.nan, F32)
    if own.any():
        p = [V[F[face[own], k]].astype(np.float64) for k in range(3)]
        bary, w = _bary(S, a[own].astype(np.float64), b[own].astype(np.float64))
        point[own], anchor[own] = _blend(bary, p).astype(F32), _blend(w, p).astype(F32)
    return face.astype(np.int32), point, anchor


def quantize(c):
    with np.errstate(invalid="ignore"):
        q = np.floor(255.0 * c + 0.5)
        return np.where(q > 0, np.minimum(q, 255.0), 0.0).astype(np.uint8)


def bake(layout, V, F, images, k, w2c, eyes, mask=None, vertex_colors=None, blend="weighted", power=2, min_cos=0.1, two_sided=False,
         near=0.0, fill=(0, 0, 0)):
    """(texture [Ha,Wa,4] uint8, weight [Ha,Wa] fp32, view [Ha,Wa] int32); the cameras as ``depthsurface.cameras`` gives them."""
    S, C, Wa, Ha = layout
    V, F = np.asarray(V, F32), np.asarray(F, np.int64).reshape(-1, 3)
    face, point, anchor = texels(layout, V, F)
    _, ta, tb = owner_tables(S, C, len(F))
    best_mode = blend == "best"
    fill = np.asarray(fill, F32).astype(np.float64)
    min_cos, near = np.float64(F32(min_cos)), np.float64(F32(near))
    texture = np.zeros((Ha, Wa, 4), np.uint8)
    texture[..., :3] = quantize(fill)
    weight, view = np.zeros((Ha, Wa), F32), np.full((Ha, Wa), -1 if best_mode else 0, np.int32)
    own = face >= 0
    n = int(own.sum())
    if n == 0:
        return texture, weight, view
    f = face[own].astype(np.int64)
    p = [V[F[f, c]].astype(np.float64) for c in range(3)]
    X, A = point[own].astype(np.float64), anchor[own].astype(np.float64)
    u, v = p[1] - p[0], p[2] - p[0]
    nrm = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)
    nl = np.sqrt((nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2])
    seen = None if mask is None else np.asarray(mask, np.int64)[own]
    I = np.asarray(images, F32)
    nv, H, W = I.shape[:3]
    sum_c, sum_w, accepted = np.zeros((n, 3)), np.zeros(n), np.zeros(n, np.int64)
    best_c, best_w, best = np.zeros((n, 3)), np.zeros(n), np.full(n, -1, np.int64)
    with np.errstate(all="ignore"):
        for e in range(nv):
            M, ke = np.asarray(w2c, F32)[e].astype(np.float64), np.asarray(k, F32)[e].astype(np.float64)
            ok = np.ones(n, bool) if seen is None else ((seen >> np.int64(e)) & 1).astype(bool)
            cam = [((M[4 * r] * X[:, 0] + M[4 * r + 1] * X[:, 1]) + M[4 * r + 2] * X[:, 2]) + M[4 * r + 3] for r in range(3)]
            ok &= cam[2] > near
            gx, gy = (ke[0] * (cam[0] / cam[2]) + ke[2]) - 0.5, (ke[1] * (cam[1] / cam[2]) + ke[3]) - 0.5
            ok &= (gx >= 0) & (gx < W - 1) & (gy >= 0) & (gy < H - 1)
            d = np.asarray(eyes, F32)[e].astype(np.float64)[None, :] - A
            dl = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
            cs = ((nrm[:, 0] * d[:, 0] + nrm[:, 1] * d[:, 1]) + nrm[:, 2] * d[:, 2]) / (nl * dl)
            if two_sided:
                cs = np.abs(cs)
            ok &= cs >= min_cos
            w = np.ones(n)
            for _ in range(power):
                w = w * cs
            gx, gy = np.where(ok, gx, 0.0), np.where(ok, gy, 0.0)
            fx, fy = np.floor(gx), np.floor(gy)
            tx, ty, x0, y0 = (gx - fx)[:, None], (gy - fy)[:, None], fx.astype(np.int64), fy.astype(np.int64)
            if W < 2 or H < 2:
                continue
            I00, I10, I01, I11 = (I[e, y0 + dy, x0 + dx].astype(np.float64) for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)))
            col = ((1.0 - tx) * (1.0 - ty) * I00 + tx * (1.0 - ty) * I10) + ((1.0 - tx) * ty * I01 + tx * ty * I11)
            accepted += ok
            sum_w = np.where(ok, sum_w + w, sum_w)
            sum_c = np.where(ok[:, None], sum_c + w[:, None] * col, sum_c)
            take = ok & ((best < 0) | (w > best_w))
            best, best_w, best_c = np.where(take, e, best), np.where(take, w, best_w), np.where(take[:, None], col, best_c)
        total = best_w if best_mode else sum_w
        coloured = total > 0
        col = best_c if best_mode else sum_c / sum_w[:, None]
        if vertex_colors is not None:
            _, wts = _bary(S, ta[own].astype(np.float64), tb[own].astype(np.float64))
            back = _blend(wts, [np.asarray(vertex_colors, F32)[F[f, c]].astype(np.float64) for c in range(3)])
        else:
            back = np.broadcast_to(fill, (n, 3))
        col = np.where(coloured[:, None], col, back)
    rgba = np.concatenate([quantize(col), np.where(coloured, 255, 0).astype(np.uint8)[:, None]], 1)
    texture[own] = rgba
    weight[own] = np.where(coloured, total, 0.0).astype(F32)
    view[own] = np.where(coloured, best, -1) if best_mode else accepted
    return texture, weight, view


def taps(layout, face, bary):
    """(x [N,4], y [N,4] int64, weights [N,4] float64) of faces >= 0: the taps (x0,y0), (x1,y0), (x0,y1), (x1,y1)."""
    S, C, Wa, Ha = layout
    f = np.asarray(face, np.int64)
    bary = np.asarray(bary, F32).astype(np.float64)
    d = np.float64(S - 2)
    with np.errstate(invalid="ignore"):
        a, b = bary[:, 1] * d, bary[:, 2] * d
        a = np.where(a > 0, np.where(a < d, a, d), 0.0)
        room = d - a
        b = np.where(b > 0, np.where(b < room, b, room), 0.0)
    odd = (f & 1).astype(bool)
    gx, gy = np.where(odd, S - a, a), np.where(odd, (S - 1) - b, b)
    fx, fy = np.floor(gx), np.floor(gy)
    tx, ty = gx - fx, gy - fy
    cell = f // 2
    x0, y0 = (cell % C) * (S + 1) + fx.astype(np.int64), (cell // C) * S + fy.astype(np.int64)
    x1, y1 = x0 + (tx > 0), y0 + (ty > 0)
    wt = np.stack([(1.0 - tx) * (1.0 - ty), tx * (1.0 - ty), (1.0 - tx) * ty, tx * ty], 1)
    return np.stack([x0, x1, x0, x1], 1), np.stack([y0, y0, y1, y1], 1), wt


def sample(layout, T, texture, face, bary, alpha=False, background=(0, 0, 0)):
    """[N, 3 or 4] fp32."""
    face = np.asarray(face, np.int64)
    ch = 4 if alpha else 3
    out = np.zeros((len(face), ch), F32)
    out[:, :3] = np.asarray(background, F32)
    ok = (face >= 0) & (face < T)
    if ok.any():
        x, y, wt = taps(layout, face[ok], np.asarray(bary, F32)[ok])
        t = texture[y, x][:, :, :ch].astype(np.float64)
        w = wt[:, :, None]
        out[ok] = (((w[:, 0] * t[:, 0] + w[:, 1] * t[:, 1]) + (w[:, 2] * t[:, 2] + w[:, 3] * t[:, 3])) / 255.0).astype(F32)
    return out
