"""Generalised (solid-angle) winding numbers of a mesh, on the device: w(q) = (1 / 4 pi) x the sum of the signed solid angles of all
triangles seen from q, walked over a mesh's triangle hierarchy with per-node moments (include/lara_meshwind.h,
csrc/meshwind.hip, csrc/solidangle.h, csrc/bvhwalk.h); opt-in like every module here.  For an outward-oriented closed mesh w is 1
inside and 0 outside; where the mesh has holes, open boundaries, duplicated or non-manifold parts it degrades smoothly, which the
crossing counts of ``meshsign`` do not: this is the inside/outside for the open surfaces ``MeshExtractor`` returns.

  * ``WindingField``     a built ``meshbvh.TriangleBVH`` and the moments of its nodes (dipole, area, area-weighted centre, squared
                         radius), built once in a buffer of their own; nothing is added to the hierarchy's buffer;
  * ``winding``          w [N] float64 of ``points``: a node farther than ``beta`` radii from the point contributes its dipole term,
                         a nearer leaf the exact term of each triangle.  ``beta=inf`` never approximates: the exact sum in tree
                         order.  The same bits on two calls;
  * ``contains``         w > ``threshold``; ``status`` bit 0: |w - threshold| < ``band`` (undecided), bit 2: w is not finite
                         (outside).  The default band exceeds the approximation error of the default ``beta`` on the suite's
                         meshes: a point outside it classifies as the exact sum does;
  * ``signed_distance``  ``bvh.query``'s exact distance with that sign: negative inside.  The magnitude's bits are ``query``'s;
  * ``winding_grid``     w at the cell centres of ``meshsign.lattice``;
  * ``volume_scores``    ``meshsign.volume_scores`` under this rule: its keys, with ``decided_pred`` / ``decided_gt`` (the share of
                         lattice points outside the band) in the place of ``unanimous_*``, and ``rule`` = "solid_angle".
                         ``Evaluator.add_volume`` takes the dict as it is.

Every function that takes ``bvh_or_field`` builds the moments when it is given a ``TriangleBVH``; hold a ``WindingField`` to build them
once.  No CPU path: tensors must live on the GPU.
"""
from __future__ import annotations

import math

import torch

from . import meshsign
from ._native import alloc_bytes, call, query, require_device, rows3
from .meshbvh import TriangleBVH

SLOT_BYTES, HEADER_BYTES = 64, 256                              # include/lara_meshwind.h
RULE = "solid_angle"
STATUS_UNDECIDED, STATUS_NOT_FINITE = 1, 4


def _checked(beta, band=0.0):
    beta, band = float(beta), float(band)
    if not beta > 0.0:
        raise ValueError("lara_amd.meshwind: beta must be > 0 (inf: the exact sum)")
    if not band >= 0.0:
        raise ValueError("lara_amd.meshwind: band must be >= 0")
    return beta, band


class WindingField:
    """The moments of ``bvh``'s nodes (a built ``TriangleBVH``), built on the current stream without a host read.  ``level(k)`` is a
    [stored slots of level k, 8] float64 view {N_x, N_y, N_z, A, c_x, c_y, c_z, r2}; a slot with A = 0 is all zero."""

    def __init__(self, bvh):
        if not isinstance(bvh, TriangleBVH):
            raise TypeError("lara_amd.meshwind: expected a meshbvh.TriangleBVH")
        require_device(bvh.device)
        self.bvh, self.device, T = bvh, bvh.device, bvh.n_triangles
        self.moments = alloc_bytes(query("lara_meshwind_moments_bytes", T), self.device)
        self.offsets, o = [], HEADER_BYTES
        for _, n in bvh.layout["levels"]:
            stored = (n + 7) // 8 * 8
            self.offsets.append((o, stored))
            o += SLOT_BYTES * stored
        assert o == self.moments.shape[0]
        call("lara_meshwind_moments", self.device, T, bvh.bvh, self.moments)

    def level(self, k):
        o, stored = self.offsets[k]
        return self.moments[o:o + SLOT_BYTES * stored].view(torch.float64).view(-1, 8)


def _field(bvh_or_field, field=None):
    """The ``WindingField`` to walk: the one given, the one passed beside its ``TriangleBVH``, or one built now."""
    if isinstance(bvh_or_field, WindingField):
        if field is not None and field is not bvh_or_field:
            raise RuntimeError("lara_amd.meshwind: the field was built for another BVH")
        return bvh_or_field
    if field is not None:
        if not isinstance(field, WindingField) or field.bvh is not bvh_or_field:
            raise RuntimeError("lara_amd.meshwind: the field was built for another BVH")
        return field
    return WindingField(bvh_or_field)


@torch.no_grad()
def winding(bvh_or_field, points, beta=2.0, return_counts=False, field=None):
    """w [N] float64[, n_tri [N] int32, n_far [N] int32] of ``points`` [N,3]: the winding number, the triangles tested and the far
    nodes accepted on the way.  NaN and zero counters for a point with a coordinate that is not finite; 0 for a mesh without a valid
    triangle."""
    beta, _ = _checked(beta)
    f = _field(bvh_or_field, field)
    P = rows3(points, f.device, "points", "meshwind")
    N = P.shape[0]
    if N >= 1 << 30:
        raise ValueError("lara_amd.meshwind: 2^30 points and more")
    w = torch.empty(N, dtype=torch.float64, device=f.device)
    n_tri = torch.empty(N, dtype=torch.int32, device=f.device) if return_counts else None
    n_far = torch.empty(N, dtype=torch.int32, device=f.device) if return_counts else None
    call("lara_meshwind_rows", f.device, N, P, f.bvh.bvh, f.moments, beta, w, n_tri, n_far)
    return (w, n_tri, n_far) if return_counts else w


def _classifier(beta, threshold, band):
    """The rule as ``meshsign``'s shells take it: (field, points[, dist]) -> (inside [N] uint8, status [N] uint8, sdf [N] fp32
    or None)."""
    def classify(f, P, dist=None):
        w = winding(f, P, beta)
        out = meshsign.verdicts(f.device, w.shape[0], dist)
        call("lara_meshwind_classify", f.device, w.shape[0], w, float(threshold), float(band), dist, *out)
        return out
    return classify


@torch.no_grad()
def contains(bvh_or_field, points, beta=2.0, threshold=0.5, band=0.05, return_status=False, field=None):
    """bool [N][, status [N] uint8]: w > ``threshold``."""
    beta, band = _checked(beta, band)
    inside, status, _ = _classifier(beta, threshold, band)(_field(bvh_or_field, field), points)
    return (inside.bool(), status) if return_status else inside.bool()


@torch.no_grad()
def signed_distance(bvh_or_field, points, beta=2.0, threshold=0.5, band=0.05, return_face=False, return_status=False, field=None):
    """sdf [N] fp32[, face [N] int32][, status [N] uint8]: ``bvh.query``'s distance, negative where ``contains``; NaN and +inf as
    ``query`` gives them."""
    beta, band = _checked(beta, band)
    f = _field(bvh_or_field, field)
    return meshsign.signed_distance_by(_classifier(beta, threshold, band), f, f.bvh, points, "meshwind", return_face, return_status)


@torch.no_grad()
def winding_grid(bvh_or_field, resolution, lo=None, hi=None, beta=2.0):
    """[R,R,R] float64: ``winding`` at the cell centres of ``meshsign.lattice(lo, hi, R)``, index [x, y, z]; ``lo`` / ``hi`` default
    to the mesh's own box (one host read of six floats)."""
    f = _field(bvh_or_field)
    R = int(resolution)
    P, _ = meshsign.lattice(*meshsign.own_box(f.bvh, lo, hi), R, f.device)
    return winding(f, P.view(-1, 3), beta).view(R, R, R)


@torch.no_grad()
def volume_scores(pred, gt, resolution=128, beta=2.0, threshold=0.5, band=0.05, device=None):
    """Volumetric IoU of two meshes (each a ``WindingField``, a ``TriangleBVH`` or a (vertices, triangles) pair) under the
    solid-angle rule: the cell centres of ``meshsign.lattice`` over the union of the two boxes are classified against both and counted
    by ``lara_meshsign_counts``.  ``meshsign.volume_scores``' dict, with ``decided_pred`` / ``decided_gt`` (the share of centres
    outside the band around the threshold) where it has ``unanimous_*``, ``rule`` = "solid_angle", ``rays`` = 0, and the three
    parameters ``beta``, ``threshold``, ``band`` beside them.  Two host reads: the boxes, the results."""
    beta, band = _checked(beta, band)
    a, b = (m if isinstance(m, WindingField) else WindingField(meshsign.as_bvh(m, device)) for m in (pred, gt))
    s = meshsign.lattice_scores(_classifier(beta, threshold, band), (a, a.bvh), (b, b.bvh), resolution, "meshwind")
    counts, N = s["counts"], s["n_lattice"]
    return {**s, "decided_pred": 1.0 - counts[4] / N, "decided_gt": 1.0 - counts[5] / N, "rule": RULE, "rays": 0,
            "beta": beta if math.isfinite(beta) else "inf", "threshold": float(threshold), "band": band}
