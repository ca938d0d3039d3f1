"""The connectivity of a triangle mesh on the device: which triangles share an edge (include/lara_meshtopo.h,
csrc/meshtopo.hip, csrc/meshtopo_ops.h); opt-in like every module here.

  * ``MeshTopology``      the unique undirected edges in ascending (lo, hi) with their incident faces -- ``edges`` [E,2], ``edge_n`` [E]
                          (incident valid triangles), ``edge_fwd`` [E] (half-edges directed lo -> hi), ``edge_face`` [E,2] (the two smallest
                          incident triangle ids, -1 where absent), ``tri_edge`` [T,3] (the edge of every half-edge, -1 for a triangle that
                          is not valid) -- and, built on first use, ``vertex_neighbors()`` (the unique neighbours of each vertex in
                          ascending vertex id) and ``vertex_faces()`` (the valid triangles around each vertex in ascending triangle id, with
                          the corner), both as CSR.  The sorts are ``torch.sort`` between calls of the library;
  * ``report``            the direct question ``meshsign``'s vote shares only hint at: is every edge shared by exactly two faces, in
                          opposite directions?  Counts of boundary, manifold, non-manifold and inconsistently oriented edges, the Euler
                          characteristic, ``is_edge_manifold``, ``is_closed``, ``is_oriented``; with ``components=True`` the number of
                          edge-connected components (``meshclean``'s labels) and, for a closed oriented mesh, the genus;
  * ``vertex_normals``    area-weighted or uniform, in double over the faces in ascending id, rounded once: what
                          ``meshio.ply_bytes(..., normals=)`` takes;
  * ``smooth_laplacian``, ``smooth_taubin``   x' = x + s (mean of the neighbours - x) as Jacobi passes over two buffers, without a host read
                          in the loop; Taubin alternates ``lam`` and the negative ``mu`` so that the volume stays.

A triangle is valid when its indices lie in [0, Nv) and differ pairwise; an index outside raises, a repeated index makes the triangle
degenerate (counted, skipped).  Integer results are exact and floating results bit-reproducible: tests/meshtopo_restate.py restates
them in numpy.

NOT tested here: vertex-manifoldness (a single fan of faces around each vertex) and self-intersection.  ``is_closed`` and
``is_oriented`` are statements about edges alone; a mesh that passes both can still pinch at a vertex or cut through itself.
Open3D's ``filter_smooth_laplacian`` / ``filter_smooth_taubin`` / ``compute_vertex_normals`` are recalled, not pinned: Open3D is not
available here.  No CPU path: tensors must live on the GPU.
"""
from __future__ import annotations

import math

import torch

from ._native import call, host_array, require_device, rows3

SENTINEL = (1 << 63) - 1                                          # include/lara_meshtopo.h
REPORT_FIELDS = ("n_vertices", "n_referenced", "n_triangles", "n_valid", "n_degenerate", "n_edges", "n_boundary", "n_manifold",
                 "n_nonmanifold", "n_inconsistent", "n_boundary_vertices", "max_degree")
CSR_NEIGHBORS, CSR_FACES = 0, 1
WEIGHTINGS = {"area": 0, "uniform": 1}


def _weighting(weighting):
    if weighting not in WEIGHTINGS:
        raise ValueError(f"lara_amd.meshtopo: weighting must be one of {sorted(WEIGHTINGS)}")
    return WEIGHTINGS[weighting]


def _steps(iterations, **factors):
    iterations = int(iterations)
    if iterations < 0:
        raise ValueError("lara_amd.meshtopo: iterations must be >= 0")
    for name, x in factors.items():
        if not math.isfinite(float(x)):
            raise ValueError(f"lara_amd.meshtopo: {name} must be finite")
    return iterations


class MeshTopology:
    """The edge table of one mesh (``vertices`` [Nv,3] fp32 on the device, ``triangles`` [T,3] of any integer type), built once on
    the current stream.  ONE host read: the number of edges, the number of valid half-edges and the error word, in one transfer;
    an index outside [0, Nv) raises there.  ``vertex_neighbors()`` and ``vertex_faces()`` add one sort each and no host read;
    ``report()`` reads its row of counts (one more), ``report(components=True)`` also what ``meshclean``'s labelling reads."""

    def __init__(self, vertices, triangles):
        if vertices.dim() != 2 or vertices.shape[1] != 3 or triangles.dim() != 2 or triangles.shape[1] != 3:
            raise RuntimeError("lara_amd.meshtopo: expected vertices [Nv,3] and triangles [T,3]")
        Nv, T = vertices.shape[0], triangles.shape[0]
        if Nv >= 2 ** 31 or 3 * T >= 2 ** 31:
            raise RuntimeError("lara_amd.meshtopo: meshes need Nv < 2^31 and 3 T < 2^31 (int32 indices)")
        require_device(vertices)
        dev = vertices.device
        V = rows3(vertices, dev, "vertices", "meshtopo")
        F = triangles.detach().to(device=dev, dtype=torch.int32).contiguous()
        self.device, self.vertices, self.triangles, self.n_vertices, self.n_triangles = dev, V, F, Nv, T
        self._neighbors = self._faces = self._report = self._boundary = self._components = None
        i32 = dict(dtype=torch.int32, device=dev)
        n = 3 * T
        E = n_valid = 0
        self.tri_edge = torch.empty(T, 3, **i32)
        if T:
            with torch.cuda.device(dev):
                err = torch.zeros(1, **i32)
                keys = torch.empty(n, dtype=torch.int64, device=dev)
                call("lara_meshtopo_halfedge_keys", dev, Nv, T, F, keys, err)
                keys, order = torch.sort(keys, stable=True)            # (stable: a run stands in ascending half-edge id)
                heads = torch.empty(n, **i32)
                call("lara_meshtopo_edge_heads", dev, n, keys, heads)
                ends = torch.cumsum(heads, 0, dtype=torch.int64)
                E, halves, e = torch.stack([ends[-1], (keys != SENTINEL).sum(), err[0].long()]).tolist()      # the host read
                if e & 1:
                    raise RuntimeError("lara_amd.meshtopo: a triangle indexes a vertex outside [0, Nv)")
                n_valid = halves // 3
        self.n_edges, self.n_valid = E, n_valid
        self.edges, self.edge_face = torch.empty(E, 2, **i32), torch.empty(E, 2, **i32)
        self.edge_n, self.edge_fwd = torch.empty(E, **i32), torch.empty(E, **i32)
        if T:
            call("lara_meshtopo_edge_rows", dev, n, E, keys, order, heads, ends, F, self.edges, self.edge_n, self.edge_fwd,
                 self.edge_face, self.tri_edge)

    # ---- adjacency ----------------------------------------------------------------------------------------------------------
    def _csr(self, keys, n, mode, width):
        dev = self.device
        offsets = torch.empty(self.n_vertices + 1, dtype=torch.int64, device=dev)
        values = torch.empty((n, 2) if width == 2 else (n,), dtype=torch.int32, device=dev)
        if n:
            with torch.cuda.device(dev):
                keys = torch.sort(keys).values[:n].contiguous()          # (unique keys: any sort gives this order)
        call("lara_meshtopo_csr", dev, self.n_vertices, n, keys if n else None, mode, offsets, values)
        return offsets, values

    def vertex_neighbors(self):
        """(offsets [Nv+1] int64, neighbors [2E] int32): row v holds the unique neighbours of vertex v in ascending vertex id."""
        if self._neighbors is None:
            keys = torch.empty(2 * self.n_edges, dtype=torch.int64, device=self.device)
            call("lara_meshtopo_pair_keys", self.device, self.n_edges, self.edges, keys)
            self._neighbors = self._csr(keys, 2 * self.n_edges, CSR_NEIGHBORS, 1)
        return self._neighbors

    def vertex_faces(self):
        """(offsets [Nv+1] int64, faces [3 n_valid, 2] int32): row v holds (triangle, corner) of the valid triangles around vertex v
        in ascending triangle id; corner k means triangles[triangle, k] == v."""
        if self._faces is None:
            keys = torch.empty(3 * self.n_triangles, dtype=torch.int64, device=self.device)
            call("lara_meshtopo_corner_keys", self.device, self.n_vertices, self.n_triangles, self.triangles, keys)
            self._faces = self._csr(keys, 3 * self.n_valid, CSR_FACES, 2)
        return self._faces

    def boundary_vertices(self):
        """[Nv] int32: 1 for a vertex of an edge with exactly one incident triangle."""
        if self._boundary is None:
            self._boundary = torch.empty(self.n_vertices, dtype=torch.int32, device=self.device)
            call("lara_meshtopo_boundary_vertices", self.device, self.n_vertices, self.n_edges, self.edges, self.edge_n, self._boundary)
        return self._boundary

    # ---- the report ---------------------------------------------------------------------------------------------------------
    def report_row(self):
        """Device int64 [12]: ``REPORT_FIELDS`` in order.  No host read."""
        out = torch.empty(len(REPORT_FIELDS), dtype=torch.int64, device=self.device)
        work = torch.empty(2 * self.n_vertices, dtype=torch.int32, device=self.device)
        call("lara_meshtopo_report", self.device, self.n_vertices, self.n_triangles, self.n_edges, self.triangles, self.edges,
             self.edge_n, self.edge_fwd, work, out)
        return out

    def n_components(self):
        """The number of edge-connected components of the valid triangles (``lara_mesh_cluster_labels`` of ``meshclean``: two
        triangles are adjacent when they share an undirected edge)."""
        dev = self.device
        F = self.triangles[self.tri_edge[:, 0] >= 0].contiguous() if self.n_triangles else self.triangles
        T = F.shape[0]
        if T == 0:
            return 0
        i32 = dict(dtype=torch.int32, device=dev)
        cap = 1 << max(6, (6 * T - 1).bit_length())
        keys, owner = torch.empty(cap, dtype=torch.int64, device=dev), torch.empty(cap, **i32)
        adj, label, work = torch.empty(3 * T, **i32), torch.empty(T, **i32), torch.empty(2, **i32)
        call("lara_mesh_cluster_labels", dev, T, F, cap, keys, owner, adj, label, work, host_array("i", 1))
        return int((label == torch.arange(T, **i32)).sum())

    def report(self, components=False):
        """A dict: ``REPORT_FIELDS`` (ints), ``euler`` = n_referenced - n_edges + n_valid, ``is_edge_manifold`` (no edge with three
        or more faces), ``is_closed`` (no boundary edge, no non-manifold edge, at least one valid triangle), ``is_oriented``
        (closed, and the two faces of every edge run along it in opposite directions).  ``components=True`` adds ``n_components``
        and, when the mesh is closed and oriented, ``genus`` = (2 n_components - euler) / 2."""
        if self._report is None:
            r = dict(zip(REPORT_FIELDS, self.report_row().tolist()))
            r["euler"] = r["n_referenced"] - r["n_edges"] + r["n_valid"]
            r["is_edge_manifold"] = r["n_nonmanifold"] == 0
            r["is_closed"] = r["n_boundary"] == 0 and r["n_nonmanifold"] == 0 and r["n_valid"] > 0
            r["is_oriented"] = r["is_closed"] and r["n_inconsistent"] == 0
            self._report = r
        r = dict(self._report)
        if components:
            if self._components is None:
                self._components = self.n_components()
            r["n_components"] = self._components
            if r["is_oriented"]:
                twice = 2 * r["n_components"] - r["euler"]
                r["genus"] = twice // 2 if twice % 2 == 0 else twice / 2
        return r

    # ---- the per-vertex functions ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def vertex_normals(self, weighting="area", return_zero_count=False, vertices=None):
        """[Nv,3] fp32 unit normals[, device int64 [1]: the vertices without one]: the sum over the vertex's faces in ascending id
        of the raw cross product ("area") or its unit vector ("uniform"; a face without area is skipped), in double, divided by its
        norm, rounded once.  A sum without a direction (a vertex without a face, a zero, inf or NaN) gives (0, 0, 0) and is counted.
        ``vertices``: other positions for the same triangles (the smoothed ones)."""
        w = _weighting(weighting)
        V = self.vertices if vertices is None else self._positions(vertices)
        offsets, faces = self.vertex_faces()
        normals = torch.empty_like(V)
        zero = torch.empty(1, dtype=torch.int64, device=self.device)
        call("lara_meshtopo_vertex_normals", self.device, self.n_vertices, V, self.triangles, offsets, faces, w, normals, zero)
        return (normals, zero) if return_zero_count else normals

    def _positions(self, vertices):
        V = rows3(vertices, self.device, "vertices", "meshtopo")
        if V.shape[0] != self.n_vertices:
            raise RuntimeError("lara_amd.meshtopo: expected as many vertices as the topology was built from")
        return V

    def _passes(self, steps, fix_boundary):
        """The Jacobi passes with the factors ``steps`` in turn over two buffers; the input is never written."""
        offsets, neighbors = self.vertex_neighbors()
        fixed = self.boundary_vertices() if fix_boundary else None
        src, bufs = self.vertices, (torch.empty_like(self.vertices), torch.empty_like(self.vertices))
        for i, s in enumerate(steps):
            call("lara_meshtopo_smooth_pass", self.device, self.n_vertices, src, bufs[i % 2], offsets, neighbors, float(s), fixed)
            src = bufs[i % 2]
        return src if steps else src.clone()

    @torch.no_grad()
    def smooth_laplacian(self, iterations, lam=0.5, fix_boundary=False):
        """New [Nv,3] fp32 positions after ``iterations`` passes x' = x + lam (mean of the neighbours - x), the mean in double over the
        neighbours in ascending id.  A vertex without a neighbour keeps its bits; with ``fix_boundary`` so does a vertex of a boundary
        edge.  Shrinks the mesh; NaN and inf propagate."""
        n = _steps(iterations, lam=lam)
        return self._passes([lam] * n, fix_boundary)

    @torch.no_grad()
    def smooth_taubin(self, iterations, lam=0.5, mu=-0.53, fix_boundary=False):
        """As ``smooth_laplacian`` with two passes per iteration: ``lam``, then ``mu`` (negative, a little larger in size), which
        undoes the shrinkage: the volume stays while the noise goes."""
        n = _steps(iterations, lam=lam, mu=mu)
        return self._passes([lam, mu] * n, fix_boundary)


def topology_report(vertices, triangles, components=False):
    """``MeshTopology(vertices, triangles).report(components)``."""
    return MeshTopology(vertices, triangles).report(components)


def vertex_normals(vertices, triangles, weighting="area", return_zero_count=False):
    """``MeshTopology(vertices, triangles).vertex_normals(...)``."""
    _weighting(weighting)
    return MeshTopology(vertices, triangles).vertex_normals(weighting, return_zero_count)


def smooth_laplacian(vertices, triangles, iterations, lam=0.5, fix_boundary=False):
    """``MeshTopology(vertices, triangles).smooth_laplacian(...)``."""
    _steps(iterations, lam=lam)
    return MeshTopology(vertices, triangles).smooth_laplacian(iterations, lam, fix_boundary)


def smooth_taubin(vertices, triangles, iterations, lam=0.5, mu=-0.53, fix_boundary=False):
    """``MeshTopology(vertices, triangles).smooth_taubin(...)``."""
    _steps(iterations, lam=lam, mu=mu)
    return MeshTopology(vertices, triangles).smooth_taubin(iterations, lam, mu, fix_boundary)
