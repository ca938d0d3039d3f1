"""include/lara_meshalign.h restated in float64 (numpy, no GPU): the transform's sequence, the 48-entry row term by term
(with the sum of the terms' magnitudes, which the summation-order bar of tests/test_meshalign_gpu.py is made of), and the ICP loop of
lara_amd/meshalign.py over brute-force closest triangles (tests/meshdist_restate.py).  The two host solves are the module's own
(float64 numpy, no device): tests/test_meshalign.py holds them to known motions through this row."""
import numpy as np

from lara_amd import meshalign
from tests import meshdist_restate as D

F32 = np.float32
ROW = 48
U = 2.0 ** -24


def transform(points, T, normals=None):
    """The header's sequence in float64, rounded once to fp32: ((A0 x + A1 y) + A2 z) + A3, and ((..) + A2 nz) inv_scale."""
    A = np.asarray(T, np.float64)[:3]
    P = np.asarray(points, F32).astype(np.float64).reshape(-1, 3)
    out = np.stack([((A[k, 0] * P[:, 0] + A[k, 1] * P[:, 1]) + A[k, 2] * P[:, 2]) + A[k, 3] for k in range(3)], 1)
    if normals is None:
        return out.astype(F32)
    inv = 1.0 / (float(np.linalg.det(A[:, :3])) ** (1.0 / 3.0))
    Nn = np.asarray(normals, F32).astype(np.float64).reshape(-1, 3)
    on = np.stack([((A[k, 0] * Nn[:, 0] + A[k, 1] * Nn[:, 1]) + A[k, 2] * Nn[:, 2]) * inv for k in range(3)], 1)
    return out.astype(F32), on.astype(F32)


def terms(src, tgt, index, normals, nindex, dist, max_dist, origin=(0.0, 0.0, 0.0), dtype=F32):
    """[N, 48] float64: every pair's contribution to every row entry (columns 0 and 47: 1 where it counts), by the header.  The
    coordinates are rounded to ``dtype`` first: fp32 as the kernel reads them, float64 for the tests of the host solves that need
    exact pairs."""
    src, tgt = np.asarray(src, dtype).reshape(-1, 3), np.asarray(tgt, dtype).reshape(-1, 3)
    N, M = len(src), len(tgt)
    j = np.arange(N) if index is None else np.asarray(index, np.int64)
    dist = np.asarray(dist, F32)
    keep = (j >= 0) & (j < M) & np.isfinite(dist) & (dist <= F32(max_dist))
    o = np.asarray(origin, np.float64)
    js = np.where(keep, j, 0)
    p = src.astype(np.float64) - o
    q = (tgt[js].astype(np.float64) if M else np.zeros((N, 3))) - o
    t = np.zeros((N, ROW))
    d = p - q
    t[:, 0] = 1.0
    t[:, 1] = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    t[:, 2:5], t[:, 5:8] = p, q
    t[:, 8:17] = (p[:, :, None] * q[:, None, :]).reshape(N, 9)
    t[:, 17] = (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]
    t[:, 18] = (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]
    has_n = np.zeros(N, bool)
    if normals is not None:
        normals = np.asarray(normals, dtype).reshape(-1, 3)
        k = np.asarray(nindex, np.int64)
        inside = keep & (k >= 0) & (k < len(normals))
        n = normals[np.where(inside, k, 0)] if len(normals) else np.zeros((N, 3), dtype)
        has_n = inside & np.isfinite(n).all(1) & (n != 0).any(1)
        n = np.where(has_n[:, None], n.astype(np.float64), 0.0)
        with np.errstate(invalid="ignore"):
            c = np.stack([p[:, 1] * n[:, 2] - p[:, 2] * n[:, 1], p[:, 2] * n[:, 0] - p[:, 0] * n[:, 2],
                          p[:, 0] * n[:, 1] - p[:, 1] * n[:, 0]], 1)
            J = np.concatenate([c, n], 1)
            r = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]
            iu = np.triu_indices(6)
            t[:, 19:40] = J[:, iu[0]] * J[:, iu[1]]
            t[:, 40:46] = J * r[:, None]
            t[:, 46] = r * r
        t[:, 47] = 1.0
    t[~keep] = 0.0
    t[~has_n, 19:] = 0.0
    return t


def row(src, tgt, index, normals, nindex, dist, max_dist, origin=(0.0, 0.0, 0.0), dtype=F32):
    """(row [48], magnitudes [48]): the entries summed in float64 (numpy's pairwise order) and the sums of the terms' magnitudes."""
    t = terms(src, tgt, index, normals, nindex, dist, max_dist, origin, dtype)
    return t.sum(0), np.abs(t).sum(0)


# ---- the case of the issue: a warped icosphere and a known motion ----------------------------------------------------------------

def warped_icosphere(level):
    """`icosphere(level)` with P -> P (1 + 0.25 x + 0.15 y z + 0.1 sin(3 z + 1) x y) (1, 0.8, 0.6): no symmetry left to hide a
    rotation in."""
    V, F = D.icosphere(level)
    P = V.astype(np.float64)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    w = 1.0 + 0.25 * x + 0.15 * y * z + 0.1 * np.sin(3.0 * z + 1.0) * x * y
    return (P * w[:, None] * np.array([1.0, 0.8, 0.6])).astype(F32), F


def rigid(angle_deg, axis=(1.0, 2.0, 3.0), t=(0.0, 0.0, 0.0), scale=1.0):
    a = np.asarray(axis, np.float64)
    T = np.eye(4)
    T[:3, :3] = scale * meshalign.rodrigues(a / np.linalg.norm(a) * np.deg2rad(angle_deg))
    T[:3, 3] = t
    return T


def moved_source(V, F, truth):
    """Vertices + face centroids of the mesh, moved by the INVERSE of ``truth`` (so that ``truth`` registers them), as fp32."""
    P = np.concatenate([V.astype(np.float64), V.astype(np.float64)[F].mean(1)])
    inv = np.linalg.inv(truth)
    return (P @ inv[:3, :3].T + inv[:3, 3]).astype(F32)


def closest_on_mesh(Q, V, F):
    """(dist fp32, face, closest float64) by brute force: the first minimum of the header's d2, its closest point."""
    d, face, _ = D.brute(Q, V, F)
    p = D.corners(V, F)
    _, c = D.point_triangle(Q, p[0][face], p[1][face], p[2][face])
    return d.astype(F32), face, c


def icp(S, V, F, *, max_dist, estimation="plane", with_scale=False, T0=None, max_iter=50, rel_fitness=1e-6, rel_rmse=1e-6):
    """The loop of `meshalign.icp` for a point-set source ``S`` against the mesh (V, F): brute-force closest triangles, the restated
    row, the module's host solves, the origin at the vertices' centroid.  What the device stores as fp32 is rounded to fp32 here as
    well, every iteration: the transformed points, the closest points, the face normals."""
    S = np.asarray(S, F32)
    nrm = D.face_normals(V, F).astype(F32)
    origin = V.astype(np.float64).mean(0)
    T = np.eye(4) if T0 is None else np.array(T0, np.float64)

    def evaluate(T):
        Q = transform(S, T)
        d, face, c = closest_on_mesh(Q, V, F)
        return row(Q, c.astype(F32), None, nrm, face, d, max_dist, origin)[0]

    def state(r):
        return {"fitness": r[0] / len(S), "inlier_rmse": float(np.sqrt(r[1] / r[0])) if r[0] > 0 else float("inf")}
    r = evaluate(T)
    history, transforms, converged = [state(r)], [T], False
    for _ in range(max_iter):
        step = meshalign.solve_plane(r, origin) if estimation == "plane" else meshalign.solve_point(r, with_scale, origin)
        T = step @ T
        r = evaluate(T)
        history.append(state(r))
        transforms.append(T)
        if abs(history[-1]["fitness"] - history[-2]["fitness"]) < rel_fitness and \
                abs(history[-1]["inlier_rmse"] - history[-2]["inlier_rmse"]) < rel_rmse:
            converged = True
            break
    return {"transformation": T, "iterations": len(history) - 1, "converged": converged, "history": history,
            "transforms": transforms, "fitness": history[-1]["fitness"], "inlier_rmse": history[-1]["inlier_rmse"]}


def rotation_error(T, truth):
    """|R_T R_truth^T - I| (Frobenius) of the two 3x3 blocks with their scales divided out."""
    a = T[:3, :3] / np.linalg.det(T[:3, :3]) ** (1.0 / 3.0)
    b = truth[:3, :3] / np.linalg.det(truth[:3, :3]) ** (1.0 / 3.0)
    return float(np.linalg.norm(a @ b.T - np.eye(3)))
