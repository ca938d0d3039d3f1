"""include/lara_meshmetrics.h restated in float64 and exact integers (numpy, no GPU): the surface sampler, brute-force
nearest neighbours and the scores.  tests/test_meshmetrics.py holds this file to closed forms; tests/test_meshmetrics_gpu.py
holds the kernels to it."""
import math

import numpy as np

U = 2.0 ** -24           # unit roundoff of fp32
MAX_SAMPLES = 1 << 22


def mix(x):
    """The header's 32-bit mixer on uint32 arrays (wrapping)."""
    x = np.asarray(x, np.uint64) & 0xffffffff
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    x ^= x >> 16
    return x


def hashed_r(seed, n):
    """(r1, r2) of samples 0..n-1: 24-bit fractions as float64."""
    k = np.arange(n, dtype=np.uint64)
    s0 = mix(np.uint64((int(seed) + 0x9e3779b9) & 0xffffffff))
    h1, h2 = mix(s0 ^ (2 * k)), mix(s0 ^ (2 * k + 1))
    return (h1 >> 8).astype(np.float64) * U, (h2 >> 8).astype(np.float64) * U


def areas(V, F):
    V, F = np.asarray(V, np.float32).astype(np.float64), np.asarray(F, np.int64)
    c = np.cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]])
    return 0.5 * np.sqrt((c[:, 0] ** 2 + c[:, 1] ** 2) + c[:, 2] ** 2)


def scale_exp(total):
    """s with total 2^s in [2^38, 2^39)."""
    return 39 - math.frexp(float(total))[1]


def quantise(A, s):
    return np.floor(np.ldexp(np.asarray(A, np.float64), s)).astype(np.int64)


def faces_from_q(q, n):
    """The integer rule: sample k takes the smallest i with prefix[i] > ((2k + 1) S) // (2n)."""
    q = np.asarray(q, np.int64)
    S = int(q.sum())
    assert S > 0 and n <= MAX_SAMPLES
    t = np.array([((2 * k + 1) * S) // (2 * n) for k in range(n)], dtype=np.int64)
    return np.searchsorted(np.cumsum(q), t, side="right").astype(np.int64)


def barycentrics(seed, n):
    r1, r2 = hashed_r(seed, n)
    su = np.sqrt(r1)
    return np.stack([1.0 - su, su * (1.0 - r2), su * r2], 1)


def points_on_faces(V, F, face, seed):
    """(points, unit normals) in float64 for the chosen faces."""
    V, F = np.asarray(V, np.float32).astype(np.float64), np.asarray(F, np.int64)
    b = barycentrics(seed, len(face))
    p0, p1, p2 = (V[F[face, j]] for j in range(3))
    pts = (b[:, :1] * p0 + b[:, 1:2] * p1) + b[:, 2:] * p2
    c = np.cross(p1 - p0, p2 - p0)
    return pts, c / np.sqrt((c ** 2).sum(1, keepdims=True))


def sample_surface(V, F, n, seed=0):
    """(points, normals, face, q, s), float64 / int64."""
    if len(F) == 0:
        raise ValueError("no triangles")
    if n > MAX_SAMPLES:
        raise ValueError("n > 2^22")
    A = areas(V, F)
    total = float(A.sum())
    if not (total > 0.0 and math.isfinite(total)):
        raise ValueError("no area")
    s = scale_exp(total)
    q = quantise(A, s)
    face = faces_from_q(q, n)
    pts, nrm = points_on_faces(V, F, face, seed)
    return pts, nrm, face, q, s


def nearest(Q, P, chunk=512):
    """(d [N] float64, index [N]): brute force in float64, the first minimum (= the smallest index)."""
    Q, P = np.asarray(Q, np.float64), np.asarray(P, np.float64)
    if len(P) == 0:
        raise ValueError("no targets")
    d, idx = np.empty(len(Q)), np.empty(len(Q), np.int64)
    for o in range(0, len(Q), chunk):
        d2 = ((Q[o:o + chunk, None, :] - P[None, :, :]) ** 2).sum(-1)
        idx[o:o + chunk] = d2.argmin(1)
        d[o:o + chunk] = np.sqrt(d2.min(1))
    return d, idx


def distances_to(Q, P, index):
    Q, P = np.asarray(Q, np.float64), np.asarray(P, np.float64)
    return np.sqrt(((Q - P[index]) ** 2).sum(1))


def scores(P, Pn, G, Gn, thresholds, near=None):
    """The score dict of two point sets (normals may be None).  ``near``: ((d_p, i_p), (d_g, i_g)) computed before."""
    (d_p, i_p), (d_g, i_g) = near if near is not None else (nearest(P, G), nearest(G, P))
    acc, comp = d_p.mean(), d_g.mean()
    prec = [float((d_p <= np.float64(np.float32(t))).mean()) for t in thresholds]
    rec = [float((d_g <= np.float64(np.float32(t))).mean()) for t in thresholds]
    nc = None
    if Pn is not None and Gn is not None:
        Pn, Gn = np.asarray(Pn, np.float64), np.asarray(Gn, np.float64)
        nc = float((np.abs((Pn * Gn[i_p]).sum(1)).sum() + np.abs((Gn * Pn[i_g]).sum(1)).sum()) / (len(d_p) + len(d_g)))
    return {"accuracy": float(acc), "completeness": float(comp), "chamfer": float(acc + comp),
            "chamfer_sq": float((d_p ** 2).mean() + (d_g ** 2).mean()), "thresholds": list(thresholds), "precision": prec,
            "recall": rec, "fscore": [2 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(prec, rec)],
            "normal_consistency": nc, "n_pred": len(d_p), "n_gt": len(d_g)}


# ---- meshes the tests share ---------------------------------------------------------------------------------------------------

def unit_square(z=0.0):
    """Two triangles over [0, 1]^2 at height z."""
    V = np.array([[0, 0, z], [1, 0, z], [1, 1, z], [0, 1, z]], np.float32)
    return V, np.array([[0, 1, 2], [0, 2, 3]], np.int64)


def cube():
    V = np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], np.float32)
    F = np.array([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6],
                  [1, 3, 5], [3, 7, 5]], np.int64)
    return V, F


def uv_sphere(n_lat=12, n_lon=22, radius=1.0):
    """A closed UV sphere: 2 n_lon (n_lat - 1) triangles (484 by default), outward windings."""
    V = [[0.0, 0.0, radius]]
    for i in range(1, n_lat):
        th = math.pi * i / n_lat
        for j in range(n_lon):
            ph = 2 * math.pi * j / n_lon
            V.append([radius * math.sin(th) * math.cos(ph), radius * math.sin(th) * math.sin(ph), radius * math.cos(th)])
    V.append([0.0, 0.0, -radius])
    ring = lambda i, j: 1 + (i - 1) * n_lon + j % n_lon
    F = [[0, ring(1, j), ring(1, j + 1)] for j in range(n_lon)]
    for i in range(1, n_lat - 1):
        for j in range(n_lon):
            F += [[ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)], [ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)]]
    south = len(V) - 1
    F += [[south, ring(n_lat - 1, j + 1), ring(n_lat - 1, j)] for j in range(n_lon)]
    return np.array(V, np.float32), np.array(F, np.int64)
