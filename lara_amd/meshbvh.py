"""Exact point-to-triangle distances at any distance from the mesh: a bounding-volume hierarchy over the triangles, the second
search structure next to ``meshdist.TriangleGrid`` (include/lara_meshbvh.h, csrc/meshbvh.hip, csrc/boxbound.h); opt-in like
every module here.

  * ``TriangleBVH``   the triangles sorted by the Morton code of their box centres (the sort itself is ``torch.sort`` between two
                      calls of the library) under an implicit complete 8-ary tree of fp32 boxes, built once.  ``query`` has the
                      surface of ``TriangleGrid.query`` and returns the same bits: both are argmins of the same double-precision
                      distance (csrc/tridist.h) under the same tie rule, the smaller face id.  There is no ring limit and no
                      brute-force route: a query far from the surface costs a walk, not T triangle tests.  About 60 bytes a
                      triangle where the grid takes 316 and 8 a cell;
  * ``point_to_mesh`` the one-shot form.

``meshdist.point_to_mesh``, ``meshdist.mesh_scores``, ``meshalign.icp``, ``meshalign.align_mesh`` and ``meshalign.aligned_scores``
take ``search="bvh"`` and come here; their default stays the grid.  No CPU path: tensors must live on the GPU.
"""
from __future__ import annotations

import torch

from ._native import call, host_array
from .meshdist import _TriangleSearch

MAX_LEVELS = 9                                                  # include/lara_meshbvh.h
HEADER_INTS, HDR_BAD, HDR_VALID, HDR_TRIANGLES, HDR_LEVELS = 4, 0, 1, 2, 3


def layout(T):
    """{"keys": byte offset, "records": byte offset, "total": bytes, "levels": [(byte offset, slots n_k), ...]} of the buffer of a
    mesh of ``T`` triangles (host code)."""
    out = host_array("l", 4 + 2 * MAX_LEVELS)
    call("lara_meshbvh_layout", None, int(T), out)
    return {"keys": out[0], "records": out[1], "total": out[3], "levels": [(out[4 + 2 * k], out[5 + 2 * k]) for k in range(out[2])]}


class TriangleBVH(_TriangleSearch):
    """The hierarchy of one mesh (``vertices`` [Nv,3] fp32 on the device, ``triangles`` [T,3] of any integer type), built on the
    current stream without a host read.  ``counts`` is a device int32 [4] view of the header: triangles never taken as candidates
    (an index outside [0, Nv) or a coordinate that is not finite), the valid ones, T, the number of levels.  ``face_normals`` and
    ``query`` are ``TriangleGrid``'s, and ``query`` returns its bits; nothing falls back."""
    _module, _falls_back = "meshbvh", False

    def _build(self):
        dev, V, F, T = self.device, self.vertices, self.triangles, self.n_triangles
        self.bvh = self._buffer("lara_meshbvh_bytes")
        self.layout = layout(T)
        call("lara_meshbvh_keys", dev, V.shape[0], T, V, F, self.bvh)
        with torch.cuda.device(dev):
            self.keys = self.bvh[self.layout["keys"]:self.layout["keys"] + 8 * T].view(torch.int64)
            self.keys.copy_(torch.sort(self.keys).values)          # (unique keys: any sort gives this order)
        call("lara_meshbvh_build", dev, V.shape[0], T, V, F, self.bvh)
        self.counts = self.bvh[:4 * HEADER_INTS].view(torch.int32)

    def _query(self, N, Q, dist, face, closest, fallbacks):
        call("lara_meshbvh_query", self.device, N, Q, self.bvh, dist, face, closest)

    @property
    def nbytes(self):
        return self.bvh.shape[0]

    @property
    def records(self):
        """[T,12] fp32 view of the sorted records {p0, p1, p2, id (an int32's bits), -, -}."""
        o = self.layout["records"]
        return self.bvh[o:o + 48 * self.n_triangles].view(torch.float32).view(-1, 12)

    def level_boxes(self, k):
        """[n_k,6] fp32 view of level ``k``'s boxes (lo, hi)."""
        o, n = self.layout["levels"][k]
        return self.bvh[o:o + 24 * n].view(torch.float32).view(-1, 6)


@torch.no_grad()
def point_to_mesh(points, vertices, triangles, return_closest=False, return_fallbacks=False):
    """``TriangleBVH(vertices, triangles).query(points, ...)``."""
    return TriangleBVH(vertices, triangles).query(points, return_closest, return_fallbacks)
