"""include/lara_meshtopo.h restated in numpy, int64 and float64: the validity rule, the table of unique edges, the report,
the two CSR adjacency tables, the two per-vertex functions with the header's order of operations, and the smoothing loops.  Written
from the header, not from the kernels: unique edges come from ``np.unique`` over (lo, hi) pairs, the adjacency from ``np.lexsort``.
The per-vertex sums run over the rank inside a row, one vector addition per rank, so every vertex adds its terms one by one in the
stored order, as the header demands; float64 ``+ - * /`` and ``sqrt`` are IEEE operations, so the results are the kernels' bits."""
import numpy as np

F32 = np.float32
REPORT_FIELDS = ("n_vertices", "n_referenced", "n_triangles", "n_valid", "n_degenerate", "n_edges", "n_boundary", "n_manifold",
                 "n_nonmanifold", "n_inconsistent", "n_boundary_vertices", "max_degree")
AREA, UNIFORM = 0, 1


def kinds(Nv, F):
    """[T]: 2 valid, 1 degenerate (in range, an index repeated), 0 an index outside [0, Nv)."""
    F = np.asarray(F, np.int64).reshape(-1, 3)
    inside = np.all((F >= 0) & (F < Nv), axis=1)
    distinct = (F[:, 0] != F[:, 1]) & (F[:, 1] != F[:, 2]) & (F[:, 0] != F[:, 2])
    return np.where(inside, np.where(distinct, 2, 1), 0)


class Topology:
    """The edge table: ``edges`` [E,2], ``edge_n``, ``edge_fwd`` [E], ``edge_face`` [E,2], ``tri_edge`` [T,3]; ``bad``: an index was
    outside [0, Nv) (python raises on it)."""

    def __init__(self, Nv, F):
        F = np.asarray(F, np.int64).reshape(-1, 3)
        self.Nv, self.F, self.T = int(Nv), F, len(F)
        self.kind = kinds(Nv, F)
        self.bad = bool((self.kind == 0).any())
        valid = self.kind == 2
        self.n_valid = int(valid.sum())
        t = np.repeat(np.nonzero(valid)[0], 3)                       # the valid half-edges in ascending h = 3 t + k
        k = np.tile(np.arange(3), self.n_valid)
        a, b = F[t, k], F[t, (k + 1) % 3]
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        self.edges, inverse = np.unique(np.stack([lo, hi], 1), axis=0, return_inverse=True) if len(t) else (np.zeros((0, 2), np.int64), np.zeros(0, np.int64))
        inverse = inverse.reshape(-1)
        E = self.E = len(self.edges)
        self.edge_n = np.bincount(inverse, minlength=E).astype(np.int64)
        self.edge_fwd = np.bincount(inverse[a == lo], minlength=E).astype(np.int64)
        self.edge_face = np.full((E, 2), -1, np.int64)
        by_edge = np.lexsort((t, inverse))                            # per edge, ascending triangle id
        e_sorted, t_sorted = inverse[by_edge], t[by_edge]
        rank = np.arange(len(t)) - np.searchsorted(e_sorted, e_sorted)
        for r in (0, 1):
            self.edge_face[e_sorted[rank == r], r] = t_sorted[rank == r]
        self.tri_edge = np.full((self.T, 3), -1, np.int64)
        self.tri_edge[t, k] = inverse

    def report(self):
        E = self.edges
        deg = np.bincount(E.reshape(-1), minlength=self.Nv) if self.E else np.zeros(self.Nv, np.int64)
        boundary = self.edge_n == 1
        r = {"n_vertices": self.Nv, "n_referenced": len(np.unique(self.F[self.kind == 2])), "n_triangles": self.T,
             "n_valid": self.n_valid, "n_degenerate": int((self.kind == 1).sum()), "n_edges": self.E, "n_boundary": int(boundary.sum()),
             "n_manifold": int((self.edge_n == 2).sum()), "n_nonmanifold": int((self.edge_n >= 3).sum()),
             "n_inconsistent": int(((self.edge_n == 2) & (self.edge_fwd != 1)).sum()),
             "n_boundary_vertices": len(np.unique(E[boundary])), "max_degree": int(deg.max()) if self.Nv else 0}
        r["euler"] = r["n_referenced"] - r["n_edges"] + r["n_valid"]
        r["is_edge_manifold"] = r["n_nonmanifold"] == 0
        r["is_closed"] = r["n_boundary"] == 0 and r["n_nonmanifold"] == 0 and r["n_valid"] > 0
        r["is_oriented"] = r["is_closed"] and r["n_inconsistent"] == 0
        return r

    def report_row(self):
        r = self.report()
        return [r[k] for k in REPORT_FIELDS]

    def boundary_vertices(self):
        flag = np.zeros(self.Nv, np.int64)
        flag[self.edges[self.edge_n == 1].reshape(-1)] = 1
        return flag

    def vertex_neighbors(self):
        """(offsets [Nv+1], neighbors [2E]): ascending vertex id inside a row."""
        src = np.concatenate([self.edges[:, 0], self.edges[:, 1]])
        dst = np.concatenate([self.edges[:, 1], self.edges[:, 0]])
        o = np.lexsort((dst, src))
        return _offsets(src[o], self.Nv), dst[o]

    def vertex_faces(self):
        """(offsets [Nv+1], faces [3 n_valid, 2] = (triangle, corner)): ascending triangle id inside a row."""
        t = np.repeat(np.nonzero(self.kind == 2)[0], 3)
        k = np.tile(np.arange(3), self.n_valid)
        v = self.F[t, k]
        o = np.lexsort((t, v))
        return _offsets(v[o], self.Nv), np.stack([t[o], k[o]], 1)

    def n_components(self):
        """Edge-connected components of the valid triangles (union-find over the triangles of every edge)."""
        parent = np.arange(self.T)

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x
        first = {}
        for t in np.nonzero(self.kind == 2)[0]:
            for e in self.tri_edge[t]:
                if e in first:
                    ra, rb = find(first[e]), find(t)
                    parent[max(ra, rb)] = min(ra, rb)
                else:
                    first[e] = t
        return len({find(t) for t in np.nonzero(self.kind == 2)[0]})


def _offsets(sorted_rows, Nv):
    return np.searchsorted(sorted_rows, np.arange(Nv + 1)).astype(np.int64)


def _ranked(offsets):
    """For rank r = 0, 1, ...: (the rows longer than r, the position of their r-th entry)."""
    lengths = np.diff(offsets)
    for r in range(int(lengths.max()) if len(lengths) else 0):
        rows = np.nonzero(lengths > r)[0]
        yield rows, offsets[rows] + r


def vertex_normals(V, F, offsets, faces, weighting):
    """(normals [Nv,3] float32, zero count): lara_meshtopo_normal for every vertex."""
    V64, F = np.asarray(V, F32).astype(np.float64), np.asarray(F, np.int64)
    s = np.zeros((len(V64), 3))
    with np.errstate(all="ignore"):
        for rows, at in _ranked(offsets):
            f = F[faces[at, 0]]
            p0, p1, p2 = V64[f[:, 0]], V64[f[:, 1]], V64[f[:, 2]]
            u, w = p1 - p0, p2 - p0
            c = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                          u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
            if weighting == UNIFORM:
                l = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
                keep = l != 0.0
                rows, c = rows[keep], c[keep] / l[keep, None]
            s[rows] = s[rows] + c
        L = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
        ok = (L > 0.0) & (L < np.inf)
        out = np.zeros((len(V64), 3), F32)
        out[ok] = (s[ok] / L[ok, None]).astype(F32)
    return out, int((~ok).sum())


def smooth_pass(X, offsets, neighbors, s, fixed=None):
    """One Jacobi pass of lara_meshtopo_smooth over float32 positions ``X``: a new float32 array."""
    X = np.asarray(X, F32)
    X64 = X.astype(np.float64)
    m = np.zeros_like(X64)
    with np.errstate(all="ignore"):
        for rows, at in _ranked(offsets):
            m[rows] = m[rows] + X64[neighbors[at]]
        degree = np.diff(offsets)
        move = degree > 0
        if fixed is not None:
            move &= np.asarray(fixed) == 0
        out = X.copy()
        mean = m[move] / degree[move, None].astype(np.float64)
        out[move] = (X64[move] + np.float64(s) * (mean - X64[move])).astype(F32)
    return out


def smooth(X, topo, steps, fix_boundary=False):
    offsets, neighbors = topo.vertex_neighbors()
    fixed = topo.boundary_vertices() if fix_boundary else None
    for s in steps:
        X = smooth_pass(X, offsets, neighbors, s, fixed)
    return np.asarray(X, F32)


def smooth_laplacian(X, topo, iterations, lam=0.5, fix_boundary=False):
    return smooth(X, topo, [lam] * iterations, fix_boundary)


def smooth_taubin(X, topo, iterations, lam=0.5, mu=-0.53, fix_boundary=False):
    return smooth(X, topo, [lam, mu] * iterations, fix_boundary)


def volume(V, F):
    """sum p0 . (p1 x p2) / 6 in float64."""
    V, F = np.asarray(V, np.float64), np.asarray(F, np.int64)
    p0, p1, p2 = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    return float((p0 * np.cross(p1, p2)).sum() / 6.0)
