"""Rigid and similarity alignment (ICP) of two surfaces before they are scored (include/lara_meshalign.h,
csrc/meshalign.hip); opt-in like every module here.

  * ``transform_points``  a 4x4 similarity applied to points (and normals) on the device, in double, one rounding to fp32;
  * ``moments``           count, centroid and covariance of a point set: the accumulate kernel with the set paired with itself;
  * ``solve_point``       Umeyama's closed form (rotation, translation, optional scale) from the 48 doubles of one reduction row;
  * ``solve_plane``       one Gauss-Newton step of the point-to-plane objective: the row's 6x6 system by Cholesky, the rotation
                          vector made an exact rotation by Rodrigues' formula.  Both solves are float64 numpy on the host: the
                          loop needs the row there for its stopping rule anyway, one host read per iteration;
  * ``icp``               the loop: transform the ORIGINAL source samples by the accumulated transform (composed in float64 on the
                          host), find the correspondences (``meshdist.TriangleGrid`` for a mesh target: closest points and face
                          normals; ``meshmetrics.nearest`` for a point set), reduce, solve, until fitness and inlier RMSE settle;
  * ``align_mesh``, ``aligned_scores``  a mesh moved onto a ground truth, and ``meshmetrics.surface_scores`` after that.

The stopping rule (both |change of fitness| < rel_fitness and |change of inlier RMSE| < rel_rmse) and the shape of the loop follow
Open3D's ``registration_icp`` as recalled [RECALLED]; Open3D is absent here and parity with it is unpinned.  Out of scope: global
registration beyond the PCA start (RANSAC, FPFH), trimmed or robust kernels, non-rigid alignment.  No CPU path: tensors must live on
the GPU.
"""
from __future__ import annotations

import numpy as np
import torch

from . import meshmetrics
from ._native import call, host_array, query, require_device, rows3

ROW = 48                                # include/lara_meshalign.h
_PCA_SIGNS = ((1.0, 1.0, 1.0), (1.0, -1.0, -1.0), (-1.0, 1.0, -1.0), (-1.0, -1.0, 1.0))      # the four proper axis flips, in candidate order


def _similarity(T):
    """(4x4 float64, its scale) of a similarity given as anything 4x4; the scale is the cube root of the 3x3 block's determinant."""
    T = np.array(T.detach().cpu().numpy() if isinstance(T, torch.Tensor) else T, dtype=np.float64)
    if T.shape != (4, 4):
        raise ValueError("lara_amd.meshalign: a transformation is a 4x4 matrix")
    det = float(np.linalg.det(T[:3, :3]))
    if not det > 0.0 or not np.isfinite(T).all():
        raise ValueError("lara_amd.meshalign: a transformation needs a finite 3x3 block of positive determinant")
    return T, det ** (1.0 / 3.0)


@torch.no_grad()
def transform_points(points, T, normals=None, *, out=None):
    """``points`` [N,3] (fp32 on the device) moved by the 4x4 float64 similarity ``T`` = [[sR, t], [0, 1]]: (sR p + t) in double,
    rounded once.  With ``normals`` [N,3]: returns (points', normals') with normals' = (sR n) / s.  ``out``: the tensor(s) to
    write, which may be the inputs.  No host read."""
    require_device(points)
    dev = points.device
    P = rows3(points, dev, "points", "meshalign")
    T, s = _similarity(T)
    Nn = None
    if normals is not None:
        Nn = normals.detach().to(dev, torch.float32).contiguous()
        if tuple(Nn.shape) != tuple(P.shape):
            raise RuntimeError("lara_amd.meshalign: normals must have the shape of the points")
    out_p, out_n = (out if normals is not None else (out, None)) if out is not None else (None, None)
    out_p = torch.empty_like(P) if out_p is None else out_p
    out_n = (torch.empty_like(P) if out_n is None else out_n) if Nn is not None else None
    call("lara_meshalign_transform", dev, P.shape[0], P, Nn, host_array("d", [float(v) for v in T[:3].ravel()]), 1.0 / s, out_p, out_n)
    return out_p if Nn is None else (out_p, out_n)


def _accumulate(row, src, tgt, index, normals, nindex, dist, max_dist, origin):
    """One launch pair of lara_meshalign_accumulate into ``row`` (a device float64 [48] view); no host read."""
    dev = src.device
    N = src.shape[0]
    ws = meshmetrics._workspace(dev, query("lara_meshalign_accumulate_workspace_bytes", N,
                                            error=ValueError("lara_amd.meshalign: 2^30 points and more")))
    call("lara_meshalign_accumulate", dev, N, tgt.shape[0], 0 if normals is None else normals.shape[0], src, tgt, index, normals,
         nindex if normals is not None else None, dist, float(max_dist), host_array("d", [float(v) for v in origin]), row, ws)


@torch.no_grad()
def accumulate(src, tgt, index, dist, max_dist, normals=None, nindex=None, origin=(0.0, 0.0, 0.0)):
    """The reduction row of N correspondences as a device float64 [48] tensor (layout: the header's table).  ``index`` None pairs
    row i with row i.  No host read."""
    require_device(src)
    row = torch.empty(ROW, dtype=torch.float64, device=src.device)
    _accumulate(row, src, tgt, index, normals, nindex, dist, max_dist, origin)
    return row


@torch.no_grad()
def moments(points, origin=(0.0, 0.0, 0.0)):
    """(n, centroid [3], covariance [3,3]) of ``points`` [N,3] as float64 numpy: the accumulate kernel with the set paired with
    itself; ``origin`` is subtracted before anything is summed and added back to the centroid.  One host read."""
    require_device(points)
    P = points.detach().to(torch.float32).contiguous()
    if P.dim() != 2 or P.shape[1] != 3 or P.shape[0] == 0:
        raise RuntimeError("lara_amd.meshalign: expected points [N,3], N > 0")
    zeros = torch.zeros(P.shape[0], dtype=torch.float32, device=P.device)
    row = accumulate(P, P, None, zeros, 0.0, origin=origin).cpu().numpy()          # the call's one host read
    return moments_from_row(row, origin)


def moments_from_row(row, origin=(0.0, 0.0, 0.0)):
    n = float(row[0])
    if n < 1:
        raise ValueError("lara_amd.meshalign: no point with finite coordinates")
    mean = row[2:5] / n
    return int(n), mean + np.asarray(origin, np.float64), row[8:17].reshape(3, 3) / n - np.outer(mean, mean)


def _world(R, t, s, origin):
    """The 4x4 of x' - o = s R (x - o) + t."""
    o = np.asarray(origin, np.float64)
    T = np.eye(4)
    T[:3, :3] = s * R
    T[:3, 3] = t + o - s * (R @ o)
    return T


def solve_point(row, with_scale=False, origin=(0.0, 0.0, 0.0)):
    """The similarity (4x4 float64) that moves the source points of ``row`` onto their partners in the least-squares sense
    (Umeyama 1991): the centred cross-covariance from the row's sums, its SVD, the determinant fix that keeps the rotation proper,
    the scale trace(D S) / var(source) when ``with_scale``.  ``origin``: what the row's call subtracted; the result is in the
    points' own frame."""
    row = np.asarray(row, np.float64)
    n = float(row[0])
    if n < 3:
        raise ValueError(f"lara_amd.meshalign: the point solve needs at least 3 pairs, got {int(n)}")
    mp, mq = row[2:5] / n, row[5:8] / n
    cov = (row[8:17].reshape(3, 3) / n - np.outer(mp, mq)).T          # sum (q - mq)(p - mp)^T / n
    var_p = float(row[17]) / n - float(mp @ mp)
    if not np.isfinite(cov).all() or not var_p > 0.0:
        raise ValueError("lara_amd.meshalign: the point solve is singular (the source pairs coincide or are not finite)")
    U, D, Vt = np.linalg.svd(cov)
    if D[1] <= 1e-14 * D[0]:
        raise ValueError("lara_amd.meshalign: the point solve is singular (the pairs lie on a line)")
    S = np.array([1.0, 1.0, 1.0 if np.linalg.det(U) * np.linalg.det(Vt) > 0.0 else -1.0])
    R = (U * S) @ Vt
    s = float((D * S).sum() / var_p) if with_scale else 1.0
    if not s > 0.0:
        raise ValueError("lara_amd.meshalign: the point solve is singular (no positive scale)")
    return _world(R, mq - s * (R @ mp), s, origin)


def rodrigues(w):
    """exp([w]x): the exact rotation of the rotation vector ``w``."""
    w = np.asarray(w, np.float64)
    th = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-8:
        return np.eye(3) + K + 0.5 * (K @ K)
    return np.eye(3) + (np.sin(th) / th) * K + ((1.0 - np.cos(th)) / (th * th)) * (K @ K)


def solve_plane(row, origin=(0.0, 0.0, 0.0)):
    """One Gauss-Newton step of sum ((R p + t - q) . n)^2 (Chen & Medioni 1992; the small-angle form of Low 2004): with
    x = (w, t), (sum J J^T) x = -sum J r from the row, by Cholesky; R = exp([w]x).  Returns the rigid 4x4 float64."""
    row = np.asarray(row, np.float64)
    if float(row[47]) < 6:
        raise ValueError(f"lara_amd.meshalign: the plane solve needs at least 6 pairs with a normal, got {int(row[47])}")
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = row[19:40]
    A = A + np.triu(A, 1).T
    try:
        if not np.isfinite(A).all():
            raise np.linalg.LinAlgError
        L = np.linalg.cholesky(A)
        if L.diagonal().min() <= 1e-10 * L.diagonal().max():
            raise np.linalg.LinAlgError
    except np.linalg.LinAlgError:
        raise ValueError("lara_amd.meshalign: the plane solve is singular (the normals do not pin all six motions: a plane, a "
                         "sphere, a cylinder)") from None
    x = np.linalg.solve(L.T, np.linalg.solve(L, -row[40:46]))
    return _world(rodrigues(x[:3]), x[3:], 1.0, origin)


def _mesh_parts(x):
    """(vertices, triangles) where ``x`` is a mesh -- an integer second entry, as ``meshmetrics._surface`` tells --, else None."""
    if isinstance(x, (torch.Tensor, np.ndarray)) or len(x) < 2 or x[1] is None:
        return None
    second = torch.as_tensor(x[1])
    return None if second.dtype.is_floating_point else (torch.as_tensor(x[0]), second)


def _device(device, *sides):
    """``device``, else the device of the first side that lives on a GPU, else the current one; refused unless it is a GPU."""
    if device is None:
        firsts = [x if isinstance(x, torch.Tensor) else x[0] for x in sides]
        cuda = [a.device for a in firsts if isinstance(a, torch.Tensor) and a.is_cuda]
        device = cuda[0] if cuda else torch.device("cuda", torch.cuda.current_device())
    dev = torch.device(device)
    require_device(dev)
    return dev


def _check_search(search):
    if search not in ("grid", "bvh"):
        raise ValueError(f"lara_amd.meshalign: search must be 'grid' or 'bvh', got {search!r}")


class _Target:
    """The search side of a registration: a mesh (one ``TriangleGrid``, built once: closest points and face normals) or a point
    set (``meshmetrics.nearest``; its normals where given)."""

    def __init__(self, target, n, seed, dev, need_points, search="grid"):
        mesh = _mesh_parts(target)
        self.grid = None
        if mesh is not None:
            from . import meshdist
            self.grid = meshdist.search_structure(search)(mesh[0].to(dev, torch.float32), mesh[1].to(dev))
            self.normals = self.grid.face_normals
            self.reference = self.grid.vertices                                          # what the origin is taken from
            self.points = meshmetrics._surface(target, n, seed, dev)[0] if need_points else None      # (area-weighted: the PCA start)
        else:
            self.points, self.normals = meshmetrics._surface(target, n, seed, dev)
            self.reference = self.points
        if self.reference.shape[0] == 0:
            raise ValueError("lara_amd.meshalign: a surface without points")

    def correspondences(self, Q):
        """(tgt, index into tgt or None, nindex into the normals, dist, fallbacks) of the query points ``Q``."""
        if self.grid is not None:
            d, face, closest, f = self.grid.query(Q, return_closest=True, return_fallbacks=True)
            return closest, None, face, d, f
        d, i, f = meshmetrics.nearest(Q, self.points, return_fallbacks=True)
        return self.points, i, i, d, f


def _evaluate(out, S, T, tgt, max_dist, origin, with_normals, buf):
    """Transform the source samples by ``T``, search, reduce: row and fallback count into ``out`` (device float64 [49])."""
    Q = transform_points(S, T, out=buf)
    pts, index, nindex, d, f = tgt.correspondences(Q)
    _accumulate(out[:ROW], Q, pts, index, tgt.normals if with_normals else None, nindex, d, max_dist, origin)
    out[ROW:] = f.double()


def _state(host):
    kept = float(host[0])
    return {"fitness": kept, "inlier_rmse": float(np.sqrt(host[1] / kept)) if kept > 0 else float("inf")}


def pca_frame(cov):
    """The principal axes of a covariance as the columns of a proper rotation, the largest variance first."""
    w, E = np.linalg.eigh(cov)
    E = E[:, ::-1].copy()
    if np.linalg.det(E) < 0.0:
        E[:, 2] = -E[:, 2]
    return E


def pca_candidates(mean_s, cov_s, mean_t, cov_t):
    """The four rigid 4x4 that map the source's principal frame onto the target's (axes matched by rank of variance, the four
    proper sign choices), in candidate order."""
    Es, Et = pca_frame(cov_s), pca_frame(cov_t)
    out = []
    for signs in _PCA_SIGNS:
        R = (Et * np.array(signs)) @ Es.T
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, mean_t - R @ mean_s
        out.append(T)
    return out


@torch.no_grad()
def icp(source, target, *, max_dist, estimation="plane", with_scale=False, init=None, max_iter=50, rel_fitness=1e-6, rel_rmse=1e-6,
        n=100000, seed=0, device=None, search="grid"):
    """Register ``source`` onto ``target``.  Each is a mesh -- (vertices, triangles[, ...]), ``n`` points sampled from a source
    mesh -- or a point set -- points, (points,) or (points, normals) --, told apart as ``meshmetrics.surface_scores`` does.

    ``estimation``: "plane" minimises the residuals along the target's normals (a mesh target's face normals; a point-set target
    must bring its normals), "point" the distances to the closest points; ``with_scale`` (with "point" only) also estimates a
    scale.  Pairs farther apart than ``max_dist`` are left out.  ``init``: None (identity), "centroid" (translation of the source's
    centroid onto the target's), "pca" (the four proper rotations that map the source's principal axes onto the target's, each
    scored by one search and reduction; the smallest inlier RMSE wins, ties go to the smaller candidate number) or a 4x4.

    Every iteration transforms the ORIGINAL source samples by the accumulated transform -- composed in float64 on the host, never
    the previous iteration's fp32 points --, searches, reduces and solves.  Stops when both |change of fitness| < ``rel_fitness``
    and |change of inlier RMSE| < ``rel_rmse`` [RECALLED from Open3D; parity unpinned], or after ``max_iter`` solves.

    Returns a dict: transformation (4x4 float64), scale, fitness (kept pairs / source points), inlier_rmse (point-to-point over
    the kept pairs), iterations (solves done), converged, history (fitness, inlier_rmse and fallbacks of the start and after
    every iteration), fallbacks (queries the brute-force kernels resolved, all searches).  One host read per iteration, one for the
    start, one for the origin (the target's centroid, subtracted inside the reduction so that meshes far from the origin keep
    their digits), plus the samplers' own and one for "centroid" / "pca".

    ``search``: what a mesh target is searched with: "grid" (``meshdist.TriangleGrid``) or "bvh" (``meshbvh.TriangleBVH``: the
    same correspondences bit for bit, hence the same result, and no query falls back to brute force however far off the start)."""
    _check_search(search)
    if estimation not in ("plane", "point"):
        raise ValueError(f"lara_amd.meshalign: estimation must be 'plane' or 'point', got {estimation!r}")
    if with_scale and estimation != "point":
        raise ValueError("lara_amd.meshalign: with_scale needs estimation='point'")
    if not float(max_dist) > 0.0:
        raise ValueError("lara_amd.meshalign: max_dist must be positive")
    start = init if isinstance(init, str) or init is None else "given"
    if start not in (None, "centroid", "pca", "given"):
        raise ValueError(f"lara_amd.meshalign: init must be None, 'centroid', 'pca' or a 4x4, got {init!r}")
    dev = _device(device, source, target)
    S = meshmetrics._surface(source, n, seed, dev)[0]
    tgt = _Target(target, n, seed, dev, need_points=start in ("centroid", "pca"), search=search)
    if S.shape[0] == 0:
        raise ValueError("lara_amd.meshalign: a surface without points")
    plane = estimation == "plane"
    if plane and tgt.normals is None:
        raise ValueError("lara_amd.meshalign: estimation='plane' needs the normals of a point-set target")
    N = S.shape[0]
    _, origin, _ = moments(tgt.reference)
    buf = torch.empty_like(S)
    out = torch.empty(4, ROW + 1, dtype=torch.float64, device=dev)
    fallbacks = 0

    T = np.eye(4)
    if start == "given":
        T, _ = _similarity(init)
    elif start is not None:
        zs, zt = (torch.zeros(x.shape[0], dtype=torch.float32, device=dev) for x in (S, tgt.points))
        _accumulate(out[0, :ROW], S, S, None, None, None, zs, 0.0, origin)
        _accumulate(out[1, :ROW], tgt.points, tgt.points, None, None, None, zt, 0.0, origin)
        host = out[:2].cpu().numpy()
        (_, ms, cs), (_, mt, ct) = moments_from_row(host[0], origin), moments_from_row(host[1], origin)
        if start == "centroid":
            T[:3, 3] = mt - ms
        else:
            cands = pca_candidates(ms, cs, mt, ct)
            for k, Tk in enumerate(cands):
                _evaluate(out[k], S, Tk, tgt, max_dist, origin, False, buf)
            host = out.cpu().numpy()
            fallbacks += int(host[:, ROW].sum())
            rmse = [_state(h)["inlier_rmse"] for h in host]
            T = cands[int(np.argmin(rmse))]          # (argmin: the first of equal minima)

    def evaluate(T):
        _evaluate(out[0], S, T, tgt, max_dist, origin, plane, buf)
        host = out[0].cpu().numpy()          # the iteration's one host read
        return host[:ROW], int(host[ROW])

    row, f = evaluate(T)
    fallbacks += f
    state = _state(row)
    history = [dict(state, fitness=state["fitness"] / N, fallbacks=f)]
    converged, iterations = False, 0
    for _ in range(int(max_iter)):
        step = solve_plane(row, origin) if plane else solve_point(row, with_scale, origin)
        T = step @ T
        iterations += 1
        row, f = evaluate(T)
        fallbacks += f
        state = _state(row)
        history.append(dict(state, fitness=state["fitness"] / N, fallbacks=f))
        if abs(history[-1]["fitness"] - history[-2]["fitness"]) < rel_fitness and \
                abs(history[-1]["inlier_rmse"] - history[-2]["inlier_rmse"]) < rel_rmse:
            converged = True
            break
    return {"transformation": T, "scale": float(np.linalg.det(T[:3, :3]) ** (1.0 / 3.0)), "fitness": history[-1]["fitness"],
            "inlier_rmse": history[-1]["inlier_rmse"], "iterations": iterations, "converged": converged, "history": history,
            "fallbacks": fallbacks}


@torch.no_grad()
def align_mesh(pred, gt, **icp_kw):
    """``pred`` -- a mesh (vertices, triangles[, ...]) -- registered onto ``gt`` by ``icp(pred, gt, **icp_kw)``: returns
    (vertices' on the device, triangles, the registration dict)."""
    if _mesh_parts(pred) is None:
        raise ValueError("lara_amd.meshalign: align_mesh moves a mesh (vertices, triangles)")
    _check_search(icp_kw.get("search", "grid"))
    dev = _device(icp_kw.pop("device", None), pred, gt)
    reg = icp(pred, gt, device=dev, **icp_kw)
    return transform_points(torch.as_tensor(pred[0]).to(dev, torch.float32), reg["transformation"]), pred[1], reg


@torch.no_grad()
def aligned_scores(pred, gt, n=100000, thresholds=meshmetrics.THRESHOLDS, seed=0, distance="point", **icp_kw):
    """``meshmetrics.surface_scores`` of ``pred`` after ``align_mesh`` has moved it onto ``gt``: that dict (``distance`` as
    there: "point" or "triangle") plus ``"alignment"``, the registration.  ``Evaluator.add_geometry`` takes it as it is.
    ``search="bvh"`` (among ``icp_kw``) also reaches the "triangle" scores: ``meshdist.mesh_scores(..., search="bvh")``."""
    search = icp_kw.get("search", "grid")
    V, F, reg = align_mesh(pred, gt, n=n, seed=seed, **icp_kw)
    if search != "grid" and distance == "triangle":
        from . import meshdist
        out = meshdist.mesh_scores((V, F), gt, n, thresholds, seed, device=V.device, search=search)
    else:
        out = meshmetrics.surface_scores((V, F), gt, n, thresholds, seed, distance=distance, device=V.device)
    out["alignment"] = reg
    return out
