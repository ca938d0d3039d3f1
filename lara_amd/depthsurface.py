"""Geometry scores of an extracted mesh against ground-truth DEPTH MAPS on the device (include/lara_depthsurface.h,
csrc/depthsurface.hip); opt-in like every module here.  LaRa's evaluation sets ship no ground-truth surface, only ``tar_dep`` /
``tar_msk`` / ``tar_ixt`` / ``tar_c2w`` (GSO) and ``tar_nrm`` (gobjaverse); this module makes the surface and scores against it:

  * ``backproject``   the valid pixels of V depth maps as world points, with normals (given, or from the depth), in the order
                      (view, row, column): an ordered compaction, reproducible bit for bit;
  * ``thin``          one point per occupied voxel (the smallest input index wins), so that overlapping views and foreshortening
                      do not weight the surface unevenly;
  * ``observe``       for every sample the set of views that saw it: in front of, or within ``tau`` behind, the view's depth;
  * ``depth_scores``  the dict of ``meshmetrics.surface_scores``, with accuracy / precision over the OBSERVED samples of the
                      prediction only -- the depth maps say nothing about the underside or the inside of the visible shell.

A depth is a view-space z (what ``output['depth_fine']`` holds); pixel (y, x) looks through (x + 0.5, y + 0.5).  Point-to-point
distances; no alignment; the prediction's own geometry occludes only where asked (``observe(occluder=...)``,
``depth_scores(self_occlusion=True)``: `lara_amd.meshray`).  No CPU path: tensors must live on the GPU (the cameras, a
few floats per view, are read and inverted on the host).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import meshmetrics
from ._native import StreamWorkspace, call, host_array, query, require_device, rows3

MAX_VIEWS, MAX_CELLS, MAX_THRESHOLDS, ROW = 64, 1 << 27, 8, 13      # include/lara_depthsurface.h
NORMALS_NONE, NORMALS_GIVEN, NORMALS_DEPTH = 0, 1, 2

_workspace = StreamWorkspace()      # its own: ``meshmetrics.nearest`` runs while a call here holds it


def cameras(ixt, c2w, invert=False):
    """Host float32 arrays (k [V,4] = fx, fy, cx, cy; pose [V,16]: ``c2w``, or with ``invert`` its float64 inverse) of ``ixt``
    [V,3,3] and ``c2w`` [V,4,4].  Raises for a skewed intrinsic matrix or a last row other than (0, 0, 1)."""
    K = np.asarray(torch.as_tensor(ixt).detach().cpu().numpy(), np.float64)
    M = np.asarray(torch.as_tensor(c2w).detach().cpu().numpy(), np.float64)
    if K.ndim != 3 or K.shape[1:] != (3, 3) or M.shape != (K.shape[0], 4, 4):
        raise ValueError("lara_amd.depthsurface: expected ixt [V,3,3] and c2w [V,4,4]")
    if np.any(K[:, 0, 1] != 0) or np.any(K[:, 1, 0] != 0) or np.any(K[:, 2] != np.array([0.0, 0.0, 1.0])):
        raise ValueError("lara_amd.depthsurface: intrinsics must be [[fx,0,cx],[0,fy,cy],[0,0,1]] (no skew)")
    if not np.all(K[:, 0, 0] > 0) or not np.all(K[:, 1, 1] > 0) or not np.all(np.isfinite(K)) or not np.all(np.isfinite(M)):
        raise ValueError("lara_amd.depthsurface: focal lengths must be positive and the cameras finite")
    k = np.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], axis=1).astype(np.float32)
    pose = (np.linalg.inv(M) if invert else M).reshape(-1, 16).astype(np.float32)
    return np.ascontiguousarray(k), np.ascontiguousarray(pose)


def _maps(depth, mask):
    """(depth fp32 contiguous, mask or None, bytes per mask element, V, H, W)."""
    require_device(depth)
    D = depth.detach().to(torch.float32).contiguous()
    if D.dim() != 3 or D.numel() == 0:
        raise ValueError("lara_amd.depthsurface: expected depth [V,H,W]")
    V, H, W = D.shape
    if V > MAX_VIEWS or V * H * W >= 1 << 31:
        raise ValueError(f"lara_amd.depthsurface: at most {MAX_VIEWS} views and fewer than 2^31 pixels")
    nbytes = 1
    if mask is not None:
        mask = mask.detach().to(D.device)
        if tuple(mask.shape) != (V, H, W):
            raise ValueError("lara_amd.depthsurface: the mask must have the depth's shape [V,H,W]")
        if mask.dtype == torch.float32:
            nbytes = 4
        elif mask.dtype not in (torch.uint8, torch.bool):
            mask = (mask != 0).to(torch.uint8)          # `.bool()` of any other type
        mask = mask.contiguous()
    return D, mask, nbytes, V, H, W


def _limit(x, what):
    x = math.inf if x is None else float(x)
    if math.isnan(x) or x < 0:
        raise ValueError(f"lara_amd.depthsurface: {what} must be a number >= 0 (None: no limit)")
    return x


@torch.no_grad()
def backproject(depth, mask, ixt, c2w, *, stride=1, depth_max=None, normals=None, jump=None):
    """(points [N,3] fp32, normals [N,3] fp32 or None, pixel [N] int32) of the valid pixels of ``depth`` [V,H,W] -- mask nonzero
    (``mask`` [V,H,W] uint8 / bool / float32, or None), depth finite, 0 < depth <= ``depth_max`` --, every ``stride``-th row and
    column, in the order (view, row, column); ``pixel`` = (v H + y) W + x.  ``normals``: None, "depth" (the cross product of the
    central differences of the back-projected map, zero at borders, silhouettes and depth steps beyond ``jump``) or a world-space
    map [V,H,W,3] (normalised; zero where it is zero or not finite).  One 8-byte host read (N).  Two calls give the same bits."""
    D, M, mbytes, V, H, W = _maps(depth, mask)
    dev = D.device
    k, pose = cameras(ixt, c2w)
    if k.shape[0] != V:
        raise ValueError("lara_amd.depthsurface: one camera per depth map")
    stride = int(stride)
    if stride < 1:
        raise ValueError("lara_amd.depthsurface: stride must be at least 1")
    dmax, jmp = _limit(depth_max, "depth_max"), _limit(jump, "jump")
    mode, nmap = NORMALS_NONE, None
    if isinstance(normals, str):
        if normals != "depth":
            raise ValueError('lara_amd.depthsurface: normals is None, "depth" or a [V,H,W,3] map')
        mode = NORMALS_DEPTH
    elif normals is not None:
        nmap = normals.detach().to(dev, torch.float32).contiguous()
        if tuple(nmap.shape) != (V, H, W, 3):
            raise ValueError("lara_amd.depthsurface: a normal map must be [V,H,W,3]")
        mode = NORMALS_GIVEN
    ws = _workspace(dev, query("lara_depthsurface_backproject_workspace_bytes", V, H, W))
    n = host_array("l", 1)
    call("lara_depthsurface_backproject_count", dev, V, H, W, D, M, mbytes, stride, dmax, n, ws)      # the one host read
    N = int(n[0])
    points = torch.empty(N, 3, dtype=torch.float32, device=dev)
    nrm = torch.empty(N, 3, dtype=torch.float32, device=dev) if mode != NORMALS_NONE else None
    pixel = torch.empty(N, dtype=torch.int32, device=dev)
    kd, pd = torch.from_numpy(k).to(dev), torch.from_numpy(pose).to(dev)
    call("lara_depthsurface_backproject_emit", dev, V, H, W, D, M, mbytes, stride, dmax, kd, pd, mode, nmap, jmp, points, nrm, pixel, ws)
    return points, nrm, pixel


@torch.no_grad()
def thin(points, normals, voxel, *, max_cells=MAX_CELLS, return_dropped=False):
    """(points [N',3], normals [N',3] or None, kept_index [N'] int32): of the points of each cell of a ``voxel`` grid (anchored at
    the points' minimum) the one with the smallest index, in input order; rows are bit copies.  A point with a non-finite
    coordinate is dropped (``return_dropped``: their number as a fourth entry).  One host read (N' and the dropped count).  Raises
    when the grid would have more than ``max_cells`` (at most 2^27) cells."""
    require_device(points)
    dev = points.device
    P = rows3(points, dev, "points", "depthsurface")
    Nn = normals.detach().to(dev, torch.float32).contiguous() if normals is not None else None
    if Nn is not None and tuple(Nn.shape) != tuple(P.shape):
        raise RuntimeError("lara_amd.depthsurface: normals must have the shape of the points")
    voxel = float(voxel)
    if not (voxel > 0.0 and math.isfinite(voxel) and float(np.float32(voxel)) > 0.0):
        raise ValueError("lara_amd.depthsurface: voxel must be a positive finite number")
    N = P.shape[0]
    nbytes = query("lara_depthsurface_thin_workspace_bytes", N, int(max_cells),
                   error=ValueError("lara_amd.depthsurface: max_cells must lie in [1, 2^27] (and N below 2^31)"))
    kept = torch.empty(N, dtype=torch.int32, device=dev)
    out_p = torch.empty(N, 3, dtype=torch.float32, device=dev)
    out_n = torch.empty(N, 3, dtype=torch.float32, device=dev) if Nn is not None else None
    counts = host_array("l", 2)
    try:
        call("lara_depthsurface_thin", dev, N, P, Nn, voxel, int(max_cells), kept, out_p, out_n, counts, _workspace(dev, nbytes))
    except RuntimeError as e:
        if "invalid argument" in str(e):
            raise ValueError(f"lara_amd.depthsurface: a voxel of {voxel} puts more than {int(max_cells)} cells over the points") from e
        raise
    n_kept = int(counts[0])
    out = (out_p[:n_kept], None if out_n is None else out_n[:n_kept], kept[:n_kept])
    return out + (int(counts[1]),) if return_dropped else out


@torch.no_grad()
def observe(points, depth, mask, ixt, c2w, tau, background_is_free=True, *, depth_max=None, occluder=None, occluder_faces=None,
            shrink=2.0 ** -10):
    """``seen`` [N] int64: bit v is set when view v observed the point -- it projects inside the image in front of the camera and
    lies no further than ``tau`` behind the depth there; on a pixel without valid depth (masked background) it counts as observed
    iff ``background_is_free``.  A non-finite point has ``seen`` = 0.  No host read.

    ``occluder``: a ``meshbvh.TriangleBVH``; a view then also has to SEE the point past that mesh -- no triangle of it (but
    ``occluder_faces[i]``, the one point i lies on) meets the segment from the camera centre to the point before its last
    ``shrink`` (``meshray.visibility``).  None: the bits of before."""
    D, M, mbytes, V, H, W = _maps(depth, mask)
    dev = D.device
    P = rows3(points, dev, "points", "depthsurface")
    k, pose = cameras(ixt, c2w, invert=True)
    if k.shape[0] != V:
        raise ValueError("lara_amd.depthsurface: one camera per depth map")
    tau = float(tau)
    if not tau >= 0.0:
        raise ValueError("lara_amd.depthsurface: tau must be >= 0")
    seen = torch.empty(P.shape[0], dtype=torch.int64, device=dev)
    call("lara_depthsurface_observe", dev, P.shape[0], P, V, H, W, D, M, mbytes, _limit(depth_max, "depth_max"),
         torch.from_numpy(k).to(dev), torch.from_numpy(pose).to(dev), tau, 1 if background_is_free else 0, seen)
    if occluder is not None:
        from . import meshray
        eyes = torch.as_tensor(c2w).detach().to(dev, torch.float32)[:, :3, 3]
        seen &= meshray.visibility(occluder, P, eyes, occluder_faces, shrink)
    return seen


def views_of(batch, b):
    """(depth [V,H,W], mask [V,H,W], ixt [V,3,3], c2w [V,4,4], normals [V,H,W,3] or None) of scene ``b`` of a collated batch:
    ``tar_dep``, ``tar_msk``, ``tar_ixt``, ``tar_c2w`` and, where the dataset has it, ``tar_nrm`` taken out of its [H, V W, 3]
    strip (already rotated into the batch's frame)."""
    dep = batch["tar_dep"][b]
    V, H, W = dep.shape
    nrm = batch.get("tar_nrm")
    if nrm is not None:
        nrm = nrm[b].reshape(H, V, W, 3).permute(1, 0, 2, 3)
    return dep, batch["tar_msk"][b], batch["tar_ixt"][b], batch["tar_c2w"][b], nrm


def _reduce(dev, dist, index, M, keep, nq, nt, thr, n_thr, row):
    N = dist.shape[0]
    ws = _workspace(dev, query("lara_depthsurface_reduce_workspace_bytes", N))
    call("lara_depthsurface_reduce", dev, N, M, dist, index, keep, nq, nt, n_thr, thr, row, ws)


@torch.no_grad()
def depth_scores(pred, depth, mask, ixt, c2w, *, n=100000, thresholds=meshmetrics.THRESHOLDS, voxel=None, tau=None, stride=1,
                 depth_max=None, normals="depth", jump=None, background_is_free=True, seed=0, return_samples=False,
                 distance="point", self_occlusion=False):
    """The geometry scores of ``pred`` -- a mesh (vertices, triangles[, ...]), ``n`` points sampled from it, or a point set taken
    as it is -- against the surface the depth maps show: ``backproject`` (then ``thin`` when ``voxel`` is given).  Accuracy and
    precision run over the OBSERVED samples of ``pred`` only (``observe`` with ``tau``, by default the largest threshold: a sample
    that could still count as precise there is never masked out); completeness and recall over all ground-truth points against ALL
    samples; normal consistency over the pairs where both normals are non-zero.  Returns the dict of
    ``meshmetrics.surface_scores`` (``Evaluator.add_geometry`` takes it), plus n_pred_observed, n_pred_unobserved, n_gt_raw, n_gt,
    normal_pairs, tau, voxel.  With no observed sample accuracy and precision are None and fscore is 0.
    Host reads: N, N' when thinning, the two rows, and the sampler's own.

    ``distance``: "point" is the above.  "triangle", for a ``pred`` that is a mesh: completeness and recall measure every
    ground-truth point against the predicted mesh's TRIANGLES (`lara_amd.meshdist`), exactly, and the normal of that direction is
    the closest face's; the ground truth is a point cloud, so accuracy and precision stay sample-to-point, bit for bit.  The dict
    gains ``"distance": "triangle"``; ``samples`` then holds faces of ``pred`` in i_gt.  A ``pred`` given as points is measured as
    with "point".

    ``self_occlusion``, for a ``pred`` that is a mesh (a point set raises ValueError): a sample also has to be visible past the
    prediction's OWN triangles from a view that observed it (`lara_amd.meshbvh`, `lara_amd.meshray`; the sample's own face is
    ignored): an inner layer less than ``tau`` behind the seen shell no longer counts.  The samples are the same points.  The dict
    gains ``n_pred_self_occluded``: observed by the depth rule, hidden by the mesh."""
    if distance not in ("point", "triangle"):
        raise ValueError(f"lara_amd.depthsurface: distance must be 'point' or 'triangle', got {distance!r}")
    if self_occlusion and not _is_mesh(pred):
        raise ValueError("lara_amd.depthsurface: self_occlusion needs a prediction that is a mesh (vertices, triangles)")
    thresholds = [float(t) for t in thresholds]
    if len(thresholds) > MAX_THRESHOLDS:
        raise ValueError(f"lara_amd.depthsurface: at most {MAX_THRESHOLDS} thresholds")
    require_device(depth)
    dev = depth.device
    if tau is None:
        if not thresholds:
            raise ValueError("lara_amd.depthsurface: tau defaults to the largest threshold; give one of them")
        tau = max(thresholds)
    occluder = _own_mesh(pred, dev) if self_occlusion else None
    if distance == "triangle":
        from . import meshdist
        P, Pn, pred_grid = meshdist._side(pred, n, seed, dev)
    else:
        (P, Pn), pred_grid = meshmetrics._surface(pred, n, seed, dev), None
    G, Gn, _ = backproject(depth, mask, ixt, c2w, stride=stride, depth_max=depth_max, normals=normals, jump=jump)
    n_gt_raw = G.shape[0]
    if voxel is not None:
        G, Gn, _ = thin(G, Gn, voxel)
    if P.shape[0] == 0 or G.shape[0] == 0:
        raise ValueError("lara_amd.depthsurface: a surface without points")
    seen = observe(P, depth, mask, ixt, c2w, tau, background_is_free, depth_max=depth_max)
    hidden = None
    if occluder is not None:
        from . import meshray
        bvh, faces = occluder
        by_depth = seen != 0
        seen = seen & meshray.visibility(bvh, P, torch.as_tensor(c2w).detach().to(dev, torch.float32)[:, :3, 3], faces(n, seed))
        hidden = (by_depth & (seen == 0)).sum()
    keep = (seen != 0).to(torch.uint8)
    d_p, i_p, f_p = meshmetrics.nearest(P, G, return_fallbacks=True)
    if pred_grid is None:
        (d_g, i_g, f_g), Tn, m_g = meshmetrics.nearest(G, P, return_fallbacks=True), Pn, P.shape[0]
    else:
        d_g, i_g, Tn, m_g, f_g = meshdist.distances_to(G, P, Pn, pred_grid)
    with_normals = Pn is not None and Gn is not None
    extra = [] if hidden is None else [hidden.to(f_p.dtype)]
    rows = torch.empty(2 * ROW + 2 + len(extra), dtype=torch.float64, device=dev)
    thr = host_array("f", thresholds)
    nq, nt = (Pn, Gn) if with_normals else (None, None)
    _reduce(dev, d_p, i_p, G.shape[0], keep, nq, nt, thr, len(thresholds), rows[:ROW])
    _reduce(dev, d_g, i_g, m_g, None, nt, Tn if with_normals else None, thr, len(thresholds), rows[ROW:2 * ROW])
    rows[2 * ROW:] = torch.stack([f_p[0], f_g[0]] + extra).double()
    host = rows.cpu().numpy()          # the one host read of the scores
    out = scores_from_rows(host[:ROW], host[ROW:2 * ROW], thresholds, with_normals, n_pred=P.shape[0])
    out.update(fallbacks=int(host[2 * ROW] + host[2 * ROW + 1]), n_gt_raw=int(n_gt_raw), tau=float(tau),
               voxel=None if voxel is None else float(voxel))
    if distance == "triangle":
        out["distance"] = "triangle"
    if hidden is not None:
        out["n_pred_self_occluded"] = int(host[2 * ROW + 2])
    if return_samples:
        out["samples"] = (P, Pn, G, Gn, d_p, i_p, d_g, i_g, seen)
    return out


def _is_mesh(pred):
    """Told apart as ``meshmetrics._surface`` does: a mesh has an integer second entry."""
    if isinstance(pred, (torch.Tensor, np.ndarray)) or len(pred) < 2 or pred[1] is None:
        return False
    return not torch.as_tensor(pred[1]).dtype.is_floating_point


def _own_mesh(pred, dev):
    """(the ``TriangleBVH`` of the mesh ``pred``, a function (n, seed) -> the faces ``meshmetrics.sample_surface`` draws its
    samples from)."""
    from . import meshbvh
    V, F = torch.as_tensor(pred[0]).to(dev, torch.float32), torch.as_tensor(pred[1]).to(dev)
    return meshbvh.TriangleBVH(V, F), lambda n, seed: meshmetrics.sample_surface(V, F, n, seed)[2]


def scores_from_rows(row_pred, row_gt, thresholds, with_normals, n_pred=None):
    """The score dict from the two rows ``lara_depthsurface_reduce`` writes (host arrays of ROW doubles: the kept pred samples ->
    gt, gt -> all pred samples); ``n_pred``: all samples of the prediction, kept or not (default: the kept ones)."""
    k_p, n_g = float(row_pred[0]), float(row_gt[0])
    n_pred = int(k_p) if n_pred is None else int(n_pred)
    some = k_p > 0
    acc, comp = (float(row_pred[1]) / k_p if some else None), float(row_gt[1]) / n_g
    prec = [float(row_pred[5 + k]) / k_p for k in range(len(thresholds))] if some else None
    rec = [float(row_gt[5 + k]) / n_g for k in range(len(thresholds))]
    pairs = float(row_pred[4]) + float(row_gt[4])
    return {"accuracy": acc, "completeness": comp, "chamfer": acc + comp if some else None,
            "chamfer_sq": float(row_pred[2]) / k_p + float(row_gt[2]) / n_g if some else None,
            "thresholds": list(thresholds), "precision": prec, "recall": rec,
            "fscore": [2.0 * p * r / (p + r) if p + r > 0.0 else 0.0 for p, r in zip(prec, rec)] if some else [0.0] * len(rec),
            "normal_consistency": (float(row_pred[3]) + float(row_gt[3])) / pairs if with_normals and pairs > 0 else None,
            "n_pred": n_pred, "n_gt": int(n_g), "n_pred_observed": int(k_p), "n_pred_unobserved": n_pred - int(k_p),
            "normal_pairs": int(pairs)}
