"""Is a point inside a mesh, on the device: crossings of fixed rays counted on a mesh's triangle hierarchy, the vote over them, signed
distances, and the volumetric IoU of two meshes (include/lara_meshsign.h, csrc/meshsign.hip, csrc/raycross.h,
csrc/bvhwalk.h); opt-in like every module here.  Every function takes a built ``meshbvh.TriangleBVH`` and walks the buffer it
holds; nothing is added to it.

  * ``crossings``        per point and ray (up to three fixed directions, ``DIRECTIONS``) the number of triangles the ray crosses
                         and the sum of their orientations (+1 where the ray leaves through an outward face).  Equal to brute force
                         over all triangles as integers: the crossing is ``meshray``'s watertight ray-triangle function, and the
                         walk only skips boxes its margined bound proves free of hits.  A ray that meets an edge or a vertex as
                         computed is unusable (cross = -1): counted once per touching triangle it would spoil a parity;
  * ``contains``         the vote of the usable rays under ``rule``: "parity" (an odd number of crossings) or "winding" (a winding
                         sum that is not zero: the union of overlapping closed parts).  A tie, and a point without a usable ray,
                         count as outside; ``status`` says so (bit 0: the rays disagree, bit 1: a ray was unusable, bit 2: none
                         was usable);
  * ``signed_distance``  ``bvh.query``'s exact distance with that sign: negative inside.  The magnitude's bits are ``query``'s;
  * ``sdf_grid``         the signed distance at the cell centres of an R x R x R lattice;
  * ``mesh_volume``      signed volume, area and the number of valid triangles, in double, in a fixed order of summation;
  * ``volume_scores``    volumetric IoU of two meshes over a lattice on the union of their boxes, with the share of lattice points
                         on which each mesh's rays were unanimous: the honest flag for a mesh that is not closed.

Parity with Open3D's occupancy (its rule, as recalled, is "parity") is unpinned: Open3D is not available here.  No CPU path: tensors
must live on the GPU.
"""
from __future__ import annotations

import numpy as np
import torch

from ._native import call, rows3

MAX_RAYS = 3                                                     # include/lara_meshsign.h
RULES = {"parity": 0, "winding": 1}
DIRECTIONS = ((1.0, 0.375, 0.6875), (-0.4375, 1.0, 0.3125), (0.5625, -0.3125, -1.0))
STATUS_DISAGREE, STATUS_UNUSABLE, STATUS_NONE = 1, 2, 4


def _checked(rays, rule):
    rays = int(rays)
    if not 1 <= rays <= MAX_RAYS:
        raise ValueError(f"lara_amd.meshsign: rays must be 1 .. {MAX_RAYS}")
    if rule not in RULES:
        raise ValueError(f"lara_amd.meshsign: rule must be one of {sorted(RULES)}")
    return rays, RULES[rule]


@torch.no_grad()
def crossings(bvh, points, rays=3):
    """(cross [N,K] int32, wind [N,K] int32) of ``points`` [N,3] under the first K = ``rays`` directions: the accepted crossings
    of the ray from the point and the sum of their orientations; cross = -1, wind = 0 for a ray that touches an edge or a vertex and
    for a point with a coordinate that is not finite.  A mesh without a valid triangle gives zeros."""
    K, _ = _checked(rays, "parity")
    P = rows3(points, bvh.device, "points", "meshsign")
    N = P.shape[0]
    if N * K >= 1 << 30:
        raise ValueError("lara_amd.meshsign: 2^30 (point, ray) pairs and more")
    cross = torch.empty(N, K, dtype=torch.int32, device=bvh.device)
    wind = torch.empty(N, K, dtype=torch.int32, device=bvh.device)
    call("lara_meshsign_rows", bvh.device, N, P, K, bvh.bvh, cross, wind)
    return cross, wind


def verdicts(device, N, dist=None):
    """Uninitialised (inside [N] uint8, status [N] uint8, sdf [N] fp32 or None without ``dist``) for a classifier to fill."""
    inside = torch.empty(N, dtype=torch.uint8, device=device)
    status = torch.empty(N, dtype=torch.uint8, device=device)
    return inside, status, None if dist is None else torch.empty(N, dtype=torch.float32, device=device)


def vote(bvh, cross, wind, rule, dist=None):
    """(inside [N] uint8, status [N] uint8, sdf [N] fp32 or None) of the rows under ``rule`` (its number)."""
    N, K = cross.shape
    out = verdicts(bvh.device, N, dist)
    call("lara_meshsign_vote", bvh.device, N, K, cross, wind, rule, dist, *out)
    return out


def _classifier(rays, rule):
    """The rule as the shells below take it: (bvh, points[, dist]) -> (inside, status, sdf)."""
    K, r = _checked(rays, rule)
    return lambda bvh, P, dist=None: vote(bvh, *crossings(bvh, P, K), r, dist)


@torch.no_grad()
def contains(bvh, points, rays=3, rule="parity", return_status=False):
    """bool [N][, status [N] uint8]: the point lies inside the mesh by the vote of its usable rays."""
    inside, status, _ = _classifier(rays, rule)(bvh, points)
    return (inside.bool(), status) if return_status else inside.bool()


def signed_distance_by(classify, mesh, bvh, points, who, return_face=False, return_status=False):
    """``signed_distance`` under any rule: ``bvh.query``'s distance with the sign ``classify(mesh, points, dist)`` gives it;
    ``mesh`` is what the classifier walks (``bvh``, or what was built on it), ``who`` the module a refusal names."""
    P = rows3(points, bvh.device, "points", who)
    dist, face = bvh.query(P)
    _, status, sdf = classify(mesh, P, dist)
    out = (sdf,) + ((face,) if return_face else ()) + ((status,) if return_status else ())
    return out if len(out) > 1 else sdf


@torch.no_grad()
def signed_distance(bvh, points, rays=3, rule="parity", return_face=False, return_status=False):
    """sdf [N] fp32[, face [N] int32][, status [N] uint8]: ``bvh.query``'s distance, negative where ``contains``; NaN and +inf
    as ``query`` gives them."""
    return signed_distance_by(_classifier(rays, rule), bvh, bvh, points, "meshsign", return_face, return_status)


def lattice(lo, hi, resolution, device):
    """([R,R,R,3] fp32 cell centres on ``device``, step [3] fp32 numpy): R cells per axis over the box ``lo`` .. ``hi`` (fp32),
    step = fl32(fl32(hi - lo) / R), centre i at fl32(lo + fl32(fl32(i + 0.5) step)) -- one fp32 torch operation per rounding."""
    R = int(resolution)
    if R < 1 or R > 1024:
        raise ValueError("lara_amd.meshsign: resolution must be 1 .. 1024")
    lo, hi = np.asarray(lo, np.float32).reshape(3), np.asarray(hi, np.float32).reshape(3)
    step = ((hi - lo).astype(np.float32) / np.float32(R)).astype(np.float32)
    half = torch.arange(R, dtype=torch.float32, device=device) + 0.5
    axes = [torch.full((R,), float(lo[a]), dtype=torch.float32, device=device) + half * float(step[a]) for a in range(3)]
    grid = torch.stack(torch.meshgrid(*axes, indexing="ij"), -1)
    return grid.contiguous(), step


def root_box(bvh):
    """[6] fp32 device view of the root's box (lo, hi); lo > hi when the mesh has no valid triangle."""
    return bvh.level_boxes(len(bvh.layout["levels"]) - 1)[0]


def union_box(boxes):
    """(lo, hi) fp32 numpy of the union of [n,6] host boxes, the empty ones (lo > hi) left out; zeros when all are empty."""
    boxes = [b for b in np.asarray(boxes, np.float32).reshape(-1, 6) if b[0] <= b[3]]
    if not boxes:
        return np.zeros(3, np.float32), np.zeros(3, np.float32)
    return np.min([b[:3] for b in boxes], 0), np.max([b[3:] for b in boxes], 0)


def own_box(bvh, lo=None, hi=None):
    """``lo``, ``hi`` of a lattice over ``bvh``'s mesh: each as given, or the root box's (one host read of six floats)."""
    if lo is None or hi is None:
        blo, bhi = union_box(root_box(bvh).cpu().numpy())
        lo, hi = blo if lo is None else lo, bhi if hi is None else hi
    return lo, hi


@torch.no_grad()
def sdf_grid(bvh, resolution, lo=None, hi=None, rays=3, rule="parity"):
    """[R,R,R] fp32: ``signed_distance`` at the cell centres of ``lattice(lo, hi, R)``, index [x, y, z]; ``lo`` / ``hi`` default
    to the mesh's own box (one host read of six floats)."""
    R = int(resolution)
    P, _ = lattice(*own_box(bvh, lo, hi), R, bvh.device)
    return signed_distance(bvh, P.view(-1, 3), rays, rule).view(R, R, R)


@torch.no_grad()
def mesh_volume(bvh):
    """Device float64 [3]: the signed volume (positive: the faces point outwards), the area and the number of valid triangles
    of ``bvh``'s mesh.  Fixed order of summation: two calls give the same bits.  No host read."""
    out = torch.empty(3, dtype=torch.float64, device=bvh.device)
    call("lara_meshsign_volume", bvh.device, bvh.bvh, out)
    return out


def as_bvh(mesh, device):
    """``mesh`` as a ``TriangleBVH``: itself, or one built from a (vertices, triangles) pair, moved to ``device`` if one is given."""
    from .meshbvh import TriangleBVH
    if isinstance(mesh, TriangleBVH):
        return mesh
    V, F = mesh
    if device is not None:
        V, F = V.to(device), F.to(device)
    return TriangleBVH(V, F)


def lattice_scores(classify, pred, gt, resolution, who):
    """``volume_scores`` under any rule: ``pred`` and ``gt`` are (mesh, its ``TriangleBVH``) pairs, ``mesh`` what
    ``classify(mesh, points)`` walks.  Returns the keys every rule shares; a rule adds its own, the shares of undisputed centres
    (1 - counts[4] / n_lattice, 1 - counts[5] / n_lattice) under its own names among them.  Two host reads: the boxes, the results."""
    (a, bvh_a), (b, bvh_b) = pred, gt
    if bvh_a.device != bvh_b.device:
        raise RuntimeError(f"lara_amd.{who}: the two meshes live on different devices")
    dev, R = bvh_a.device, int(resolution)
    lo, hi = union_box(torch.stack([root_box(bvh_a), root_box(bvh_b)]).cpu().numpy())
    P, step = lattice(lo, hi, R, dev)
    P = P.view(-1, 3)
    N = P.shape[0]
    sides = [classify(m, P)[:2] for m in (a, b)]
    counts = torch.empty(8, dtype=torch.int64, device=dev)
    call("lara_meshsign_counts", dev, N, sides[0][0], sides[0][1], sides[1][0], sides[1][1], counts)
    vols = torch.stack([mesh_volume(bvh_a), mesh_volume(bvh_b)])
    counts, vols = counts.cpu().tolist(), vols.cpu().tolist()
    cell = float(step[0]) * float(step[1]) * float(step[2])
    return {"volume_iou": counts[2] / counts[3] if counts[3] else None, "volume_pred": counts[0] * cell, "volume_gt": counts[1] * cell,
            "volume_pred_mesh": vols[0][0], "volume_gt_mesh": vols[1][0], "n_lattice": N, "resolution": R, "counts": counts}


@torch.no_grad()
def volume_scores(pred, gt, resolution=128, rays=3, rule="parity", device=None):
    """Volumetric IoU of two meshes (each a ``TriangleBVH`` or a (vertices, triangles) pair): the cell centres of a lattice of
    ``resolution``^3 cells over the union of the two boxes are classified against both, and counted on the device.  A dict:
    ``volume_iou`` = n_and / n_or (None when no centre is inside either), ``volume_pred``, ``volume_gt`` (count x cell volume),
    ``volume_pred_mesh``, ``volume_gt_mesh`` (``mesh_volume``'s signed volumes), ``unanimous_pred``, ``unanimous_gt`` (the share
    of centres on which the side's usable rays agreed: below 1 for a mesh that is not closed, and then the IoU is a number about
    a surface without an inside), ``n_lattice``, ``resolution``, ``rule``, ``rays``, and ``counts``: the eight integers of ``lara_meshsign_counts``.  Two host
    reads: the boxes, the results."""
    classify = _classifier(rays, rule)
    a, b = as_bvh(pred, device), as_bvh(gt, device)
    s = lattice_scores(classify, (a, a), (b, b), resolution, "meshsign")
    counts, N = s["counts"], s["n_lattice"]
    return {**s, "unanimous_pred": 1.0 - counts[4] / N, "unanimous_gt": 1.0 - counts[5] / N, "rule": rule, "rays": int(rays)}
