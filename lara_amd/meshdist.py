"""Exact point-to-triangle distances on the device, and the geometry scores measured with them (include/lara_meshdist.h,
csrc/meshdist.hip, csrc/tridist.h); opt-in like every module here.

  * ``TriangleGrid``    a uniform grid over a mesh's triangles, built once: every triangle is registered in the cells its bounding
                        box overlaps (triangles spanning more than four cells go to a list every query tests).  ``query`` gives,
                        for every point, the distance to the mesh, the nearest face and optionally the closest point: Chebyshev
                        rings of cells with the conservative bound of ``meshmetrics.nearest``, a brute-force kernel for the
                        queries the rings do not settle.  All arithmetic in double; exact ties go to the smaller face id, so two
                        calls give the same bits;
  * ``point_to_mesh``   the one-shot form;
  * ``mesh_scores``     ``meshmetrics.surface_scores`` with every sample measured against the OTHER MESH'S TRIANGLES instead of
                        its samples: a mesh against itself scores 0 up to the rounding of its samples.

The two surfaces are scored where they are: `lara_amd.meshalign` registers them first (ICP; ``aligned_scores``, which searches
through the ``TriangleGrid`` of this module).  No CPU path: tensors must live on the GPU.
"""
from __future__ import annotations

import numpy as np
import torch

from . import meshmetrics
from ._native import alloc_bytes, call, host_array, query, require_device, rows3

RMAX, MAX_SPAN, MAX_GRID = 4, 4, 256                           # include/lara_meshdist.h
HEADER_INTS, HDR_BAD, HDR_LARGE, HDR_PAIRS, HDR_TRIANGLES = 4, 0, 1, 2, 3


def grid_resolution(T):
    """Cells along the longest axis of the grid over ``T`` triangles: clamp(ceil(sqrt(T / 4)), 1, 256)."""
    return query("lara_meshdist_grid_resolution", int(T))


class _TriangleSearch:
    """What the search structures over one mesh share (``TriangleGrid`` here, ``meshbvh.TriangleBVH``): the mesh as the kernels
    take it, the face normals, and ``query`` around the one call that differs.  A subclass names its ``_module``, says whether its
    search ``_falls_back`` to brute force, builds its buffer in ``_build()`` and runs its search in ``_query(...)``."""

    def __init__(self, vertices, triangles):
        require_device(vertices)
        dev = vertices.device
        V = vertices.detach().to(torch.float32).contiguous()
        if V.dim() != 2 or V.shape[1] != 3 or triangles.dim() != 2 or triangles.shape[1] != 3:
            raise RuntimeError(f"lara_amd.{self._module}: expected vertices [Nv,3] and triangles [T,3]")
        F = triangles.to(device=dev, dtype=torch.int32).contiguous()
        if V.shape[0] == 0:
            raise ValueError(f"lara_amd.{self._module}: the mesh has no vertices")
        self.vertices, self.triangles, self.device = V, F, dev
        self._normals = None
        self._build()

    def _buffer(self, bytes_query):
        """The structure's uninitialised buffer, sized by the library for this mesh."""
        nbytes = query(bytes_query, self.n_triangles,
                       error=ValueError(f"lara_amd.{self._module}: the mesh has no triangles (or 2^26 and more)"))
        return alloc_bytes(nbytes, self.device)

    @property
    def n_triangles(self):
        return self.triangles.shape[0]

    @property
    def face_normals(self):
        """[T,3] fp32 unit face normals (zero where a face has no area), computed once."""
        if self._normals is None:
            self._normals = torch.empty(self.n_triangles, 3, dtype=torch.float32, device=self.device)
            call("lara_meshdist_face_normals", self.device, self.vertices.shape[0], self.n_triangles, self.vertices, self.triangles,
                 self._normals)
        return self._normals

    @torch.no_grad()
    def query(self, points, return_closest=False, return_fallbacks=False):
        """(dist [N] fp32, face [N] int32[, closest [N,3] fp32][, fallbacks: device int32 [1]]) of ``points`` [N,3]: the same bits
        from either structure.  face = -1 and dist = +inf for a point with a coordinate that is not finite, or when the mesh has no
        valid triangle.  ``fallbacks``: the queries brute force settled (the grid), zero where nothing falls back (the hierarchy);
        there for the callers that sum it.  No host read."""
        Q = rows3(points, self.device, "points", self._module)
        N = Q.shape[0]
        if N >= 1 << 30:
            raise ValueError(f"lara_amd.{self._module}: 2^30 points and more")
        dist = torch.empty(N, dtype=torch.float32, device=self.device)
        face = torch.empty(N, dtype=torch.int32, device=self.device)
        closest = torch.empty(N, 3, dtype=torch.float32, device=self.device) if return_closest else None
        fallbacks = torch.zeros(1, dtype=torch.int32, device=self.device) if return_fallbacks or self._falls_back else None
        self._query(N, Q, dist, face, closest, fallbacks)
        return (dist, face) + ((closest,) if return_closest else ()) + ((fallbacks,) if return_fallbacks else ())


class TriangleGrid(_TriangleSearch):
    """The search structure of one mesh (``vertices`` [Nv,3] fp32 on the device, ``triangles`` [T,3] of any integer type), built
    on the current stream without a host read.  ``counts`` is a device int32 [4] view of the grid's header: triangles never taken
    as candidates (an index outside [0, Nv) or a coordinate that is not finite), the large list's length, the (triangle, cell)
    pairs, T."""
    _module, _falls_back = "meshdist", True

    def _build(self):
        self.grid = self._buffer("lara_meshdist_grid_bytes")
        call("lara_meshdist_build", self.device, self.vertices.shape[0], self.n_triangles, self.vertices, self.triangles, self.grid)
        self.counts = self.grid[:4 * HEADER_INTS].view(torch.int32)

    def _query(self, N, Q, dist, face, closest, fallbacks):
        ws = meshmetrics._workspace(self.device, query("lara_meshdist_query_workspace_bytes", N))
        call("lara_meshdist_query", self.device, N, Q, self.grid, dist, face, closest, fallbacks, ws)


def search_structure(search):
    """The class behind ``search``: "grid" -> ``TriangleGrid``, "bvh" -> ``meshbvh.TriangleBVH`` (imported here, on that route
    only); any other value is refused."""
    if search == "grid":
        return TriangleGrid
    if search == "bvh":
        from . import meshbvh
        return meshbvh.TriangleBVH
    raise ValueError(f"lara_amd.meshdist: search must be 'grid' or 'bvh', got {search!r}")


@torch.no_grad()
def point_to_mesh(points, vertices, triangles, return_closest=False, return_fallbacks=False, *, search="grid"):
    """``TriangleGrid(vertices, triangles).query(points, ...)``; ``search="bvh"``: ``meshbvh.TriangleBVH`` instead, the same bits."""
    return search_structure(search)(vertices, triangles).query(points, return_closest, return_fallbacks)


def _side(x, n, seed, dev, structure=TriangleGrid):
    """(points, normals or None, grid or None) of one side, told apart as ``meshmetrics._surface`` does: a mesh -- an integer
    second entry -- is sampled AND gets a grid (``structure``) over its triangles; a point set is taken as it is."""
    points, normals = meshmetrics._surface(x, n, seed, dev)
    second = None if isinstance(x, (torch.Tensor, np.ndarray)) or len(x) < 2 or x[1] is None else torch.as_tensor(x[1])
    if second is None or second.dtype.is_floating_point:
        return points, normals, None
    return points, normals, structure(torch.as_tensor(x[0]).to(dev, torch.float32), second.to(dev))


def distances_to(points, target_points, target_normals, target_grid):
    """(dist, index, normals the index points into, their count, fallbacks) from ``points`` to one side: to its triangles where
    it is a mesh (index = the face, normals = the unit face normals), to its points where it is a point set."""
    if target_grid is not None:
        d, i, f = target_grid.query(points, return_fallbacks=True)
        return d, i, target_grid.face_normals, target_grid.n_triangles, f
    d, i, f = meshmetrics.nearest(points, target_points, return_fallbacks=True)
    return d, i, target_normals, target_points.shape[0], f


@torch.no_grad()
def mesh_scores(pred, gt, n=100000, thresholds=meshmetrics.THRESHOLDS, seed=0, *, return_samples=False, device=None, search="grid"):
    """``meshmetrics.surface_scores`` with exact distances: ``n`` points are sampled from each mesh as there, and every sample is
    measured against the other mesh's TRIANGLES; normal consistency is |n_sample . n_closest_face|.  A side given as a bare point
    set has no triangles: the other side's samples are measured against its points, as ``surface_scores`` does.  Returns its dict
    (``Evaluator.add_geometry`` takes it) plus ``"distance": "triangle"``.  One host read (the two reduction rows), plus one per
    sampled mesh.  ``return_samples``: also ``samples``, the device tensors scored (pred_points, pred_normals, gt_points,
    gt_normals, d_pred, face_pred, d_gt, face_gt) -- an index is a face of the other side where that side is a mesh.
    ``search``: "grid" (``TriangleGrid``) or "bvh" (``meshbvh.TriangleBVH``: the same distances and faces, no fallbacks)."""
    structure = search_structure(search)
    thresholds = [float(t) for t in thresholds]
    if len(thresholds) > meshmetrics.MAX_THRESHOLDS:
        raise ValueError(f"lara_amd.meshdist: at most {meshmetrics.MAX_THRESHOLDS} thresholds")
    if device is None:
        firsts = [x if isinstance(x, torch.Tensor) else x[0] for x in (pred, gt)]
        cuda = [a.device for a in firsts if isinstance(a, torch.Tensor) and a.is_cuda]
        device = cuda[0] if cuda else torch.device("cuda", torch.cuda.current_device())
    dev = torch.device(device)
    require_device(dev)
    P, Pn, Pg = _side(pred, n, seed, dev, structure)
    G, Gn, Gg = _side(gt, n, seed, dev, structure)
    if P.shape[0] == 0 or G.shape[0] == 0:
        raise ValueError("lara_amd.meshdist: a surface without points")
    d_p, i_p, nt_p, m_p, f_p = distances_to(P, G, Gn, Gg)
    d_g, i_g, nt_g, m_g, f_g = distances_to(G, P, Pn, Pg)
    with_normals = Pn is not None and Gn is not None
    ROW = meshmetrics.ROW
    rows = torch.empty(2 * ROW + 2, dtype=torch.float64, device=dev)
    thr = host_array("f", thresholds)
    for k, (d, i, nq, nt, M) in enumerate(((d_p, i_p, Pn, nt_p, m_p), (d_g, i_g, Gn, nt_g, m_g))):
        N = d.shape[0]
        ws = meshmetrics._workspace(dev, query("lara_meshmetrics_reduce_workspace_bytes", N))
        call("lara_meshmetrics_reduce", dev, N, M, d, i, nq if with_normals else None, nt if with_normals else None,
             len(thresholds), thr, rows[k * ROW:(k + 1) * ROW], ws)
    rows[2 * ROW:] = torch.stack([f_p[0], f_g[0]]).double()
    host = rows.cpu().numpy()          # the call's one host read
    out = meshmetrics.scores_from_rows(host[:ROW], host[ROW:2 * ROW], thresholds, with_normals)
    out["fallbacks"] = int(host[2 * ROW] + host[2 * ROW + 1])
    out["distance"] = "triangle"
    if return_samples:
        out["samples"] = (P, Pn, G, Gn, d_p, i_p, d_g, i_g)
    return out
