"""numpy restatement of the reference's mesh post-processing (tools/meshExtractor.py:116-135) and of the Open3D calls it
makes, the oracle of include/lara_meshclean.h.  Open3D is absent here and the reference pins no version of it: every
Open3D function below is [RECALLED] from its published ``TriangleMesh`` code, not run.

* crop (:116-119): a vertex is inside iff ``aabb[0] <= v <= aabb[1]`` on every axis (fp32 vertices promoted to double,
  the box in double); ``RemoveTrianglesByMask`` drops every triangle with a vertex outside and keeps the order of the rest.
* ``ClusterConnectedTriangles``: ``GetEdgeToTrianglesMap`` keys every triangle edge as the ordered pair
  (min(a,b), max(a,b)); the triangles listed under one edge are mutually adjacent; a BFS started at every not yet visited
  triangle in index order numbers the clusters.  Returns (triangle_clusters [T], cluster_n_triangles [C],
  cluster_area [C]), the area of a triangle being 0.5 |(v1 - v0) x (v2 - v0)|.
* the keep rule (:122-133): ``n = sort(counts)[-min(C, 10)]``; triangles of clusters with fewer than n triangles go.
* ``RemoveUnreferencedVertices``: the referenced vertices (and their colours) in their original order, triangles remapped.

The reference raises in ``argmax`` on an empty cluster list; here an empty mesh stays empty (C = 0)."""
from __future__ import annotations

from collections import deque

import numpy as np


def crop(vertices, triangles, box):
    """box [2,3] (lo, hi) in double -> (triangles kept, in order; their mask)."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    box = np.asarray(box, np.float64).reshape(2, 3)
    inside = (v >= box[0]).all(-1) & (v <= box[1]).all(-1)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    keep = inside[t].all(-1) if len(t) else np.zeros(0, bool)
    return t[keep], keep


def edge_to_triangles(triangles):
    """``GetEdgeToTrianglesMap``: {(min, max): [triangles in index order]}."""
    m = {}
    for ti, tri in enumerate(np.asarray(triangles, np.int64).reshape(-1, 3).tolist()):
        for e in range(3):
            a, b = tri[e], tri[(e + 1) % 3]
            m.setdefault((min(a, b), max(a, b)), []).append(ti)
    return m


def triangle_areas(vertices, triangles):
    v = np.asarray(vertices, np.float32).astype(np.float64)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    if not len(t):
        return np.zeros(0)
    return 0.5 * np.linalg.norm(np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]]), axis=1)


def cluster_bfs(vertices, triangles):
    """``ClusterConnectedTriangles`` as Open3D runs it: adjacency from the edge map, BFS in triangle order."""
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    T = len(t)
    adj = [set() for _ in range(T)]
    for tris in edge_to_triangles(t).values():
        for a in tris:
            adj[a].update(tris)
    labels = np.full(T, -1, np.int64)
    counts = []
    for start in range(T):
        if labels[start] >= 0:
            continue
        c = len(counts)
        labels[start] = c
        q, n = deque([start]), 0
        while q:
            x = q.popleft()
            n += 1
            for y in adj[x]:
                if labels[y] < 0:
                    labels[y] = c
                    q.append(y)
        counts.append(n)
    return finish_clusters(vertices, t, labels, len(counts))


def cluster_scipy(vertices, triangles):
    """The same clusters from ``scipy.sparse.csgraph.connected_components`` on the triangle graph of shared edges
    (each edge's triangles chained to its first), renumbered by smallest triangle index: the BFS's independent witness,
    and fast enough for a full-size mesh."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    T = len(t)
    if not T:
        return finish_clusters(vertices, t, np.zeros(0, np.int64), 0)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    e.sort(axis=1)
    tri_of = np.tile(np.arange(T), 3)
    _, inv = np.unique(e, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    first = np.full(inv.max() + 1, 3 * T, np.int64)
    np.minimum.at(first, inv, tri_of)
    g = coo_matrix((np.ones(3 * T), (tri_of, first[inv])), shape=(T, T))
    n, lab = connected_components(g, directed=False)
    order = np.full(n, T, np.int64)
    np.minimum.at(order, lab, np.arange(T))
    rank = np.empty(n, np.int64)
    rank[np.argsort(order, kind="stable")] = np.arange(n)
    return finish_clusters(vertices, t, rank[lab], n)


def finish_clusters(vertices, triangles, labels, C):
    counts = np.bincount(labels, minlength=C).astype(np.int64)
    area = np.zeros(C)
    np.add.at(area, labels, triangle_areas(vertices, triangles))
    return labels.astype(np.int64), counts, area


def keep_mask(labels, counts, keep=10):
    """meshExtractor.py:128-133 (True = the triangle stays)."""
    if not len(counts):
        return np.zeros(len(labels), bool)
    n = np.sort(counts)[-min(len(counts), keep)]
    return counts[labels] >= n


def remove_unreferenced(vertices, triangles, colors=None):
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    ref = np.zeros(len(vertices), bool)
    ref[t.reshape(-1)] = True
    new = np.cumsum(ref) - 1
    return (np.asarray(vertices)[ref], new[t], None if colors is None else np.asarray(colors)[ref])


def clean_mesh(vertices, triangles, colors=None, aabb=None, keep=10, clusters=cluster_bfs):
    """meshExtractor.py:116-135 minus the writer: (vertices, triangles int64, colors, info) with the cluster arrays of the
    cropped mesh in ``info``; ``aabb`` = the config's 6 numbers, scaled by 1.1 here as ``MeshExtractor.__init__`` does."""
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    if aabb is not None:
        t, _ = crop(vertices, t, np.array(aabb, np.float64).reshape(2, 3) * 1.1)
    labels, counts, area = clusters(vertices, t)
    info = {"triangle_clusters": labels, "cluster_n_triangles": counts, "cluster_area": area}
    t = t[keep_mask(labels, counts, keep)]
    v, t, c = remove_unreferenced(vertices, t, colors)
    return v, t, c, info
