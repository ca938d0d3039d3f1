"""Geometry scores between an extracted mesh and a ground-truth surface on the device: accuracy, completeness, Chamfer distance,
precision / recall / F-score at distance thresholds and normal consistency (include/lara_meshmetrics.h,
csrc/meshmetrics.hip); opt-in like every module here.

  * ``sample_surface``  n points on a triangle mesh: area-weighted (integer-quantised areas, an exact prefix sum), stratified
                        (sample k takes the face that holds the k-th of n equal strata of the total area), deterministic (a
                        32-bit integer hash of (seed, k) gives the barycentrics);
  * ``nearest``         for every query the nearest target and its distance, exactly: a uniform grid over the targets, Chebyshev
                        rings of cells around the query, a conservative termination bound, a brute-force kernel for the queries
                        the rings do not settle.  Exact ties go to the smaller index: the result is reproducible although the
                        grid's build order is not;
  * ``surface_scores``  both of the above in both directions, one reduction pass per direction, one host read.

Point-to-point distances between samples by default; ``surface_scores(..., distance="triangle")`` measures against the other
mesh's triangles instead (`lara_amd.meshdist`).  The two surfaces are scored where they are: `lara_amd.meshalign` registers them
first (ICP; ``aligned_scores``).  No CPU path: tensors must live on the GPU.
"""
from __future__ import annotations

import numpy as np
import torch

from ._native import StreamWorkspace, call, host_array, query, require_device

MAX_SAMPLES, RMAX, MAX_GRID, MAX_THRESHOLDS, ROW = 1 << 22, 4, 256, 8, 12      # include/lara_meshmetrics.h
THRESHOLDS = (0.005, 0.01, 0.02)      # in the units of the meshes; LaRa's scenes live in [-1, 1]^3 or smaller boxes

_workspace = StreamWorkspace()      # (meshdist and meshalign take theirs from here too)


def grid_resolution(M):
    """Cells along the longest axis of the grid ``nearest`` builds over ``M`` targets: clamp(ceil(sqrt(M / 4)), 1, 256)."""
    return query("lara_meshmetrics_grid_resolution", int(M))


@torch.no_grad()
def sample_surface(vertices, triangles, n, seed=0, *, return_quantised=False):
    """``n`` points on the mesh (``vertices`` [Nv,3] fp32 on the device, ``triangles`` [T,3] of any integer type): returns
    (points [n,3] fp32, normals [n,3] fp32 -- the unit face normal --, face [n] int32).  Two calls give the same bits; another
    ``seed`` moves the points inside their faces and leaves ``face`` alone.  One 16-byte host read (the total area, from which
    the quantisation scale is chosen).  Raises for an empty mesh, a mesh without area, a triangle indexing outside [0, Nv) and
    ``n`` > 2^22.  ``return_quantised``: also return (q [T] int64 -- the integer areas --, s -- q = floor(area 2^s))."""
    require_device(vertices)
    dev = vertices.device
    V = vertices.detach().to(torch.float32).contiguous()
    if V.dim() != 2 or V.shape[1] != 3 or triangles.dim() != 2 or triangles.shape[1] != 3:
        raise RuntimeError("lara_amd.meshmetrics: expected vertices [Nv,3] and triangles [T,3]")
    F = triangles.to(device=dev, dtype=torch.int32).contiguous()
    Nv, T, n = V.shape[0], F.shape[0], int(n)
    if n > MAX_SAMPLES or n < 0:
        raise ValueError(f"lara_amd.meshmetrics: n must lie in [0, 2^22], got {n}")
    nbytes = query("lara_meshmetrics_sample_workspace_bytes", T,
                   error=ValueError("lara_amd.meshmetrics: the mesh has no triangles (or 2^28 and more)"))
    ws = _workspace(dev, nbytes)
    q = torch.empty(T, dtype=torch.int64, device=dev)
    points = torch.empty(n, 3, dtype=torch.float32, device=dev)
    normals = torch.empty(n, 3, dtype=torch.float32, device=dev)
    face = torch.empty(n, dtype=torch.int32, device=dev)
    s = host_array("i", 1)
    call("lara_meshmetrics_sample_surface", dev, Nv, T, V, F, n, ((int(seed) & 0xffffffff) ^ 0x80000000) - 0x80000000, q, s, points, normals, face, ws)
    return (points, normals, face, q, int(s[0])) if return_quantised else (points, normals, face)


@torch.no_grad()
def nearest(queries, targets, *, return_fallbacks=False):
    """(dist [N] fp32, index [N] int32): for every row of ``queries`` [N,3] the nearest row of ``targets`` [M,3] under the fp32
    squared distance (dx^2 + dy^2) + dz^2, an exact tie going to the smaller index.  No host read.  ``return_fallbacks``: also a
    device int32 [1], the number of queries the brute-force kernel resolved."""
    require_device(targets)
    dev = targets.device
    Q = queries.detach().to(dev, torch.float32).contiguous()
    P = targets.detach().to(torch.float32).contiguous()
    if Q.dim() != 2 or Q.shape[1] != 3 or P.dim() != 2 or P.shape[1] != 3:
        raise RuntimeError("lara_amd.meshmetrics: expected queries [N,3] and targets [M,3]")
    N, M = Q.shape[0], P.shape[0]
    nbytes = query("lara_meshmetrics_nearest_workspace_bytes", N, M,
                   error=ValueError("lara_amd.meshmetrics: nearest needs at least one target (and fewer than 2^30 points)"))
    dist = torch.empty(N, dtype=torch.float32, device=dev)
    index = torch.empty(N, dtype=torch.int32, device=dev)
    fallbacks = torch.zeros(1, dtype=torch.int32, device=dev)
    call("lara_meshmetrics_nearest", dev, N, M, Q, P, dist, index, fallbacks, _workspace(dev, nbytes))
    return (dist, index, fallbacks) if return_fallbacks else (dist, index)


def _surface(x, n, seed, dev):
    """(points, normals or None) of a mesh -- (vertices, triangles, ...): sampled -- or of a point set -- points, (points,) or
    (points, normals).  numpy arrays (``mesh.read_obj``) go to ``dev``."""
    if isinstance(x, (torch.Tensor, np.ndarray)):
        x = (x,)
    parts = [None if a is None else torch.as_tensor(a) for a in tuple(x)[:2]]          # (what follows -- colours, info -- is not read)
    first = parts[0].to(dev, torch.float32)
    if len(parts) > 1 and parts[1] is not None and not parts[1].dtype.is_floating_point:
        points, normals, _ = sample_surface(first, parts[1].to(dev), n, seed)
        return points, normals
    normals = parts[1].to(dev, torch.float32).contiguous() if len(parts) > 1 and parts[1] is not None else None
    if normals is not None and tuple(normals.shape) != tuple(first.shape):
        raise RuntimeError("lara_amd.meshmetrics: a point set's normals must have the shape of its points")
    return first.contiguous(), normals


@torch.no_grad()
def surface_scores(pred, gt, n=100000, thresholds=THRESHOLDS, seed=0, *, return_samples=False, device=None, distance="point"):
    """The geometry scores of ``pred`` against ``gt``.  Each is a mesh -- (vertices, triangles[, ...]): what `lara_amd.mesh`
    returns and what ``mesh.read_obj`` reads, taken as they are, ``n`` points sampled from each -- or a point set -- points [N,3],
    (points,) or (points, normals).  Returns a dict of Python floats:

      accuracy (mean pred -> gt distance), completeness (mean gt -> pred), chamfer (their sum), chamfer_sq (the same with squared
      distances), precision / recall / fscore (lists, one entry per threshold t: the share of pred / gt points with d <=
      float32(t), and 2 p r / (p + r), 0 when p + r is 0), thresholds, normal_consistency (mean |n . n_nn| over both directions;
      None when a side has no normals), n_pred, n_gt, fallbacks (queries of either direction the brute-force kernel resolved).

    One host read (the two reduction rows), plus one per sampled mesh.  ``return_samples``: also ``samples``, the device tensors
    scored (pred_points, pred_normals, gt_points, gt_normals, d_pred, i_pred, d_gt, i_gt).

    ``distance``: "point" measures every sample against the other side's SAMPLES (what the text above describes); "triangle"
    measures it against the other mesh's triangles, exactly: ``lara_amd.meshdist.mesh_scores``, same arguments, same dict plus
    ``"distance": "triangle"``."""
    if distance == "triangle":
        from . import meshdist
        return meshdist.mesh_scores(pred, gt, n, thresholds, seed, return_samples=return_samples, device=device)
    if distance != "point":
        raise ValueError(f"lara_amd.meshmetrics: distance must be 'point' or 'triangle', got {distance!r}")
    thresholds = [float(t) for t in thresholds]
    if len(thresholds) > MAX_THRESHOLDS:
        raise ValueError(f"lara_amd.meshmetrics: at most {MAX_THRESHOLDS} thresholds")
    if device is None:
        firsts = [x if isinstance(x, torch.Tensor) else x[0] for x in (pred, gt)]
        cuda = [a.device for a in firsts if isinstance(a, torch.Tensor) and a.is_cuda]
        device = cuda[0] if cuda else torch.device("cuda", torch.cuda.current_device())
    dev = torch.device(device)
    require_device(dev)
    P, Pn = _surface(pred, n, seed, dev)
    G, Gn = _surface(gt, n, seed, dev)
    if P.shape[0] == 0 or G.shape[0] == 0:
        raise ValueError("lara_amd.meshmetrics: a surface without points")
    d_p, i_p, f_p = nearest(P, G, return_fallbacks=True)
    d_g, i_g, f_g = nearest(G, P, return_fallbacks=True)
    with_normals = Pn is not None and Gn is not None
    rows = torch.empty(2 * ROW + 2, dtype=torch.float64, device=dev)
    thr = host_array("f", thresholds)
    for k, (d, i, nq, nt) in enumerate(((d_p, i_p, Pn, Gn), (d_g, i_g, Gn, Pn))):
        N = d.shape[0]
        ws = _workspace(dev, query("lara_meshmetrics_reduce_workspace_bytes", N))
        call("lara_meshmetrics_reduce", dev, N, (G if k == 0 else P).shape[0], d, i, nq if with_normals else None, nt if with_normals else None,
             len(thresholds), thr, rows[k * ROW:(k + 1) * ROW], ws)
    rows[2 * ROW:] = torch.stack([f_p[0], f_g[0]]).double()
    host = rows.cpu().numpy()          # the call's one host read
    out = scores_from_rows(host[:ROW], host[ROW:2 * ROW], thresholds, with_normals)
    out["fallbacks"] = int(host[2 * ROW] + host[2 * ROW + 1])
    if return_samples:
        out["samples"] = (P, Pn, G, Gn, d_p, i_p, d_g, i_g)
    return out


def scores_from_rows(row_pred, row_gt, thresholds, with_normals):
    """The score dict from the two rows ``lara_meshmetrics_reduce`` writes (host arrays of ROW doubles: pred -> gt, gt -> pred)."""
    n_p, n_g = float(row_pred[0]), float(row_gt[0])
    acc, comp = float(row_pred[1]) / n_p, float(row_gt[1]) / n_g
    prec = [float(row_pred[4 + k]) / n_p for k in range(len(thresholds))]
    rec = [float(row_gt[4 + k]) / n_g for k in range(len(thresholds))]
    return {"accuracy": acc, "completeness": comp, "chamfer": acc + comp,
            "chamfer_sq": float(row_pred[2]) / n_p + float(row_gt[2]) / n_g,
            "thresholds": list(thresholds), "precision": prec, "recall": rec,
            "fscore": [2.0 * p * r / (p + r) if p + r > 0.0 else 0.0 for p, r in zip(prec, rec)],
            "normal_consistency": (float(row_pred[3]) + float(row_gt[3])) / (n_p + n_g) if with_normals else None,
            "n_pred": int(n_p), "n_gt": int(n_g)}
