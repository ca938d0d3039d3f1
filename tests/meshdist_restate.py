"""include/lara_meshdist.h restated in float64 (numpy, no GPU): the point-to-triangle distance in the header's operation
order, an independent seven-region (Ericson) closest point, brute force over a mesh, the unit face normals, and the grid search
itself -- cells, large list, rings, bound -- with the fp32 cell rule.  tests/test_meshdist.py holds this file to closed forms and
the host entry to it; tests/test_meshdist_gpu.py holds the kernels to it."""
import math

import numpy as np

U = 2.0 ** -24           # unit roundoff of fp32
RMAX, MAX_SPAN, MAX_GRID = 4, 4, 256
F32 = np.float32


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _segment(q, a, b):
    ab, aq = b - a, q - a
    den, num = _dot(ab, ab), _dot(aq, ab)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(den > 0.0, np.clip(num / np.where(den > 0.0, den, 1.0), 0.0, 1.0), 0.0)
    c = a + t[..., None] * ab
    d = q - c
    return _dot(d, d), c


def point_triangle(q, p0, p1, p2):
    """(d2, closest) of the header's sequence, float64, broadcast over leading axes; inputs are rounded to fp32 first."""
    q, p0, p1, p2 = (np.asarray(x, F32).astype(np.float64) for x in (q, p0, p1, p2))
    q, p0, p1, p2 = np.broadcast_arrays(q, p0, p1, p2)
    e0, e2 = p1 - p0, p2 - p0
    n = _cross(e0, e2)
    nn = _dot(n, n)
    w0 = q - p0
    f0, f1, f2 = _dot(_cross(e0, w0), n), _dot(_cross(p2 - p1, q - p1), n), _dot(_cross(p0 - p2, q - p2), n)
    inside = (nn > 0.0) & (f0 >= 0.0) & (f1 >= 0.0) & (f2 >= 0.0)
    s = _dot(n, w0)
    safe = np.where(nn > 0.0, nn, 1.0)
    d2_in, c_in = (s * s) / safe, q - (s / safe)[..., None] * n
    d2, c = _segment(q, p0, p1)
    for a, b in ((p1, p2), (p2, p0)):
        d, cc = _segment(q, a, b)
        take = d < d2
        d2, c = np.where(take, d, d2), np.where(take[..., None], cc, c)
    return np.where(inside, d2_in, d2), np.where(inside[..., None], c_in, c)


def ericson(q, a, b, c):
    """The closest point of triangle a b c to q by the seven Voronoi regions (Ericson, Real-Time Collision Detection, 5.1.5):
    one query, float64.  Independent of the formulation above."""
    q, a, b, c = (np.asarray(x, np.float64) for x in (q, a, b, c))
    ab, ac, ap = b - a, c - a, q - a
    d1, d2 = ab @ ap, ac @ ap
    if d1 <= 0 and d2 <= 0:
        return a
    bp = q - b
    d3, d4 = ab @ bp, ac @ bp
    if d3 >= 0 and d4 <= d3:
        return b
    vc = d1 * d4 - d3 * d2
    if vc <= 0 and d1 >= 0 and d3 <= 0:
        return a + (d1 / (d1 - d3)) * ab
    cp = q - c
    d5, d6 = ab @ cp, ac @ cp
    if d6 >= 0 and d5 <= d6:
        return c
    vb = d5 * d2 - d1 * d6
    if vb <= 0 and d2 >= 0 and d6 <= 0:
        return a + (d2 / (d2 - d6)) * ac
    va = d3 * d6 - d5 * d4
    if va <= 0 and (d4 - d3) >= 0 and (d5 - d6) >= 0:
        return b + ((d4 - d3) / ((d4 - d3) + (d5 - d6))) * (c - b)
    den = 1.0 / (va + vb + vc)
    return a + ab * (vb * den) + ac * (vc * den)


def valid_triangles(V, F):
    """Triangles that may be candidates: every index inside [0, Nv) and every coordinate finite."""
    V, F = np.asarray(V, F32), np.asarray(F, np.int64)
    ok = np.all((F >= 0) & (F < len(V)), axis=1)
    safe = np.where(ok[:, None], F, 0)
    return ok & np.isfinite(V[safe].astype(np.float64)).all(axis=(1, 2))


def corners(V, F):
    V, F = np.asarray(V, F32), np.asarray(F, np.int64)
    safe = np.where(valid_triangles(V, F)[:, None], F, 0)
    return V[safe[:, 0]], V[safe[:, 1]], V[safe[:, 2]]


def all_d2(Q, V, F, chunk=256):
    """[N, T] float64 squared distances (+inf in the columns of invalid triangles)."""
    Q = np.asarray(Q, F32)
    p0, p1, p2 = corners(V, F)
    ok = valid_triangles(V, F)
    out = np.empty((len(Q), len(p0)))
    for o in range(0, len(Q), chunk):
        out[o:o + chunk] = point_triangle(Q[o:o + chunk, None, :], p0[None], p1[None], p2[None])[0]
    out[:, ~ok] = np.inf
    return out


def brute(Q, V, F):
    """(d [N] float64, face [N], d2 [N, T]): the first minimum (= the smallest face id); face -1, d +inf without a valid triangle."""
    d2 = all_d2(Q, V, F)
    face = d2.argmin(1)
    best = d2[np.arange(len(d2)), face]
    return np.sqrt(best), np.where(np.isfinite(best), face, -1), d2


def face_normals(V, F):
    """c / |c| in float64; zero where |c| is 0 or an index is bad."""
    V, F = np.asarray(V, F32).astype(np.float64), np.asarray(F, np.int64)
    ok = np.all((F >= 0) & (F < len(V)), axis=1)
    S = np.where(ok[:, None], F, 0)
    c = _cross(V[S[:, 1]] - V[S[:, 0]], V[S[:, 2]] - V[S[:, 0]])
    ln = np.sqrt(_dot(c, c))
    good = ok & (ln > 0) & np.isfinite(ln)
    return np.where(good[:, None], c / np.where(good, ln, 1.0)[:, None], 0.0)


def scale(Q, V, F):
    """S of the bars: the largest coordinate magnitude among the queries and the valid triangles' vertices."""
    p = np.concatenate([x.ravel() for x in corners(V, F)] + [np.asarray(Q, F32).ravel()])
    p = p[np.isfinite(p)]
    return float(np.abs(p).max()) if len(p) else 0.0


# ---- the grid search, restated ------------------------------------------------------------------------------------------------

def grid_resolution(T):
    return min(max(int(math.ceil(math.sqrt(T / 4.0))), 1), MAX_GRID)


class Grid:
    """The header's build in numpy: fp32 box, cell edge and cell rule; the large list; the cells' triangle lists."""

    def __init__(self, V, F):
        V, F = np.asarray(V, F32), np.asarray(F, np.int64)
        self.T, self.ok = len(F), valid_triangles(V, F)
        self.p = corners(V, F)
        R = grid_resolution(self.T)
        P = np.stack(self.p, 1)[self.ok]          # [valid, 3, 3]
        if len(P):
            lo, hi = P.min((0, 1)), P.max((0, 1))
        else:
            lo, hi = np.zeros(3, F32), np.zeros(3, F32)
        ext = (hi - lo).astype(F32)
        emax = F32(ext.max())
        h, inv_h = F32(1), F32(1)
        if emax > 0 and np.isfinite(emax):
            hh = F32(emax / F32(R))
            with np.errstate(over="ignore", divide="ignore"):
                ii = F32(F32(1) / hh)
            if hh > 0 and np.isfinite(ii):
                h, inv_h = hh, ii
        self.lo, self.h, self.inv_h, self.ext = lo.astype(F32), h, inv_h, F32(F32(R) * h)
        f = (ext * inv_h).astype(F32)
        self.R = np.array([min(int(x) + 1, R) if 0 <= x < R else (R if x >= R else 1) for x in f])
        self.large, self.cells = [], {}
        for i in range(self.T):
            if not self.ok[i]:
                continue
            tri = np.stack([p[i] for p in self.p])
            c0, c1 = self.cell(tri.min(0)), self.cell(tri.max(0))
            if np.any(c1 - c0 + 1 > MAX_SPAN):
                self.large.append(i)
                continue
            for z in range(c0[2], c1[2] + 1):
                for y in range(c0[1], c1[1] + 1):
                    for x in range(c0[0], c1[0] + 1):
                        self.cells.setdefault((x, y, z), []).append(i)
        self.pairs = sum(len(v) for v in self.cells.values())

    def cell(self, p):
        u = ((np.asarray(p, F32) - self.lo).astype(F32) * self.inv_h).astype(F32)
        f = np.floor(u)
        return np.array([int(min(max(f[a], 0), self.R[a] - 1)) if not np.isnan(f[a]) else 0 for a in range(3)])

    def d2(self, q, ids):
        ids = np.asarray(ids, np.int64)
        return point_triangle(np.asarray(q, F32)[None], self.p[0][ids], self.p[1][ids], self.p[2][ids])[0]

    def search(self, q):
        """(face, d2, fell back, triangle tests) of one query, by the header's rule; the fallback is brute force."""
        q = np.asarray(q, F32)
        if not np.isfinite(q).all():
            return -1, np.inf, False, 0
        best, tests = (np.inf, 2 ** 31 - 1), 0

        def take(best, ids):
            if len(ids) == 0:
                return best
            ids = np.asarray(ids, np.int64)
            d = self.d2(q, ids)
            j = np.lexsort((ids, d))[0]          # the smallest d2, then the smallest id
            return (d[j], int(ids[j])) if d[j] < best[0] or (d[j] == best[0] and ids[j] < best[1]) else best
        best = take(best, self.large)
        tests += len(self.large)
        u = (q - self.lo).astype(F32)
        c = self.cell(q)
        margin = F32(max(abs(u[0]), abs(u[1]), abs(u[2]), self.ext) * F32(2.0 ** -18))
        for r in range(RMAX + 1):
            for z in range(max(c[2] - r, 0), min(c[2] + r, self.R[2] - 1) + 1):
                for y in range(max(c[1] - r, 0), min(c[1] + r, self.R[1] - 1) + 1):
                    for x in range(max(c[0] - r, 0), min(c[0] + r, self.R[0] - 1) + 1):
                        if max(abs(x - c[0]), abs(y - c[1]), abs(z - c[2])) == r:
                            ids = self.cells.get((x, y, z), [])
                            best = take(best, ids)
                            tests += len(ids)
            gap = F32(np.inf)
            for a in range(3):
                if c[a] - r > 0:
                    gap = min(gap, F32(u[a] - F32(F32(c[a] - r) * self.h)))
                if c[a] + r + 1 < self.R[a]:
                    gap = min(gap, F32(F32(F32(c[a] + r + 1) * self.h) - u[a]))
            bound = np.float64(max(F32(0), F32(gap - margin)))
            if best[0] < bound * bound:
                return best[1], best[0], False, tests
        ids = np.flatnonzero(self.ok)
        best = take((np.inf, 2 ** 31 - 1), ids)
        return (best[1] if np.isfinite(best[0]) else -1), best[0], True, tests + len(ids)


# ---- scores -------------------------------------------------------------------------------------------------------------------

def scores(P, Pn, G, Gn, near_p, near_g, nt_p, nt_g, thresholds):
    """The score dict from the two directions' (d, index) and the normals the indices point into (face normals of a mesh side)."""
    (d_p, i_p), (d_g, i_g) = near_p, near_g
    acc, comp = d_p.mean(), d_g.mean()
    prec = [float((d_p <= np.float64(F32(t))).mean()) for t in thresholds]
    rec = [float((d_g <= np.float64(F32(t))).mean()) for t in thresholds]
    nc = None
    if Pn is not None and Gn is not None:
        Pn, Gn = np.asarray(Pn, np.float64), np.asarray(Gn, np.float64)
        nc = float((np.abs((Pn * np.asarray(nt_p, np.float64)[i_p]).sum(1)).sum()
                    + np.abs((Gn * np.asarray(nt_g, np.float64)[i_g]).sum(1)).sum()) / (len(d_p) + len(d_g)))
    return {"accuracy": float(acc), "completeness": float(comp), "chamfer": float(acc + comp),
            "chamfer_sq": float((d_p ** 2).mean() + (d_g ** 2).mean()), "thresholds": list(thresholds), "precision": prec,
            "recall": rec, "fscore": [2 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(prec, rec)],
            "normal_consistency": nc, "n_pred": len(d_p), "n_gt": len(d_g)}


# ---- meshes the tests share ---------------------------------------------------------------------------------------------------

def icosphere(level=3, radius=1.0):
    """20 x 4^level triangles on the sphere (1 280 at level 3), outward windings."""
    t = (1.0 + math.sqrt(5.0)) / 2.0
    V = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1],
         [-t, 0, -1], [-t, 0, 1]]
    V = [list(np.array(v) / np.linalg.norm(v)) for v in V]
    F = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
         [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    for _ in range(level):
        mid, F2 = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                v = np.array(V[a]) + np.array(V[b])
                V.append(list(v / np.linalg.norm(v)))
                mid[key] = len(V) - 1
            return mid[key]
        for a, b, c in F:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            F2 += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        F = F2
    return (np.array(V) * radius).astype(F32), np.array(F, np.int64)


def fan(n=256, radius=1.0):
    """n triangles around the origin in the plane z = 0: they all share vertex 0."""
    ang = 2 * math.pi * np.arange(n) / n
    V = np.concatenate([[[0, 0, 0]], np.stack([radius * np.cos(ang), radius * np.sin(ang), np.zeros(n)], 1)]).astype(F32)
    F = np.array([[0, 1 + k, 1 + (k + 1) % n] for k in range(n)], np.int64)
    return V, F


def rippled_sphere_points(n, seed, amplitude=0.01, radius=1.0):
    """n points near the sphere: random directions, the radius rippled by +-amplitude."""
    g = np.random.default_rng(seed)
    d = g.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = radius * (1.0 + amplitude * np.sin(7 * d[:, 0]) * np.cos(5 * d[:, 1] + 3 * d[:, 2]))
    return (d * r[:, None]).astype(F32)
