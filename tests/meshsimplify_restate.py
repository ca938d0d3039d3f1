"""numpy restatement of include/lara_meshsimplify.h as lara_amd.meshsimplify composes it: fp32 cell arithmetic, fp64
everything else, integer triangle rules.  The authority the kernels are held to (tests/test_meshsimplify_gpu.py) and that
tests/test_meshsimplify.py holds to closed forms.  No GPU, no library."""
import math

import numpy as np

MAX_CELL = 1 << 21
LAMBDA = 2.0 ** -10


def spacing32(x):
    """The distance from |x| to the next larger fp32 number (elementwise)."""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def default_origin(V, h):
    h32 = np.float32(h)
    return (np.asarray(V, np.float32).min(0) - np.float32(0.5) * h32).astype(np.float32)


def cells(V, h, origin=None):
    """(cell [Nv,3] int64, origin fp32 [3], h32): floorf((v - origin) / h) in fp32.  ValueError for what the library refuses."""
    V = np.asarray(V, np.float32).reshape(-1, 3)
    h32 = np.float32(h)
    if not np.all(np.isfinite(V)):
        raise ValueError("a vertex is not finite")
    o = default_origin(V, h32) if origin is None else np.asarray(origin, np.float64).astype(np.float32).reshape(3)
    with np.errstate(over="ignore", invalid="ignore"):
        f = np.floor((V - o[None, :]) / h32)                  # fp32 subtract, fp32 divide
    assert f.dtype == np.float32
    if not np.all(f >= 0):
        raise ValueError("negative cell index")
    if np.any(f >= MAX_CELL):
        raise ValueError("voxel_size too small for this extent")
    return f.astype(np.int64), o, h32


def clusters(cell):
    """(vertex_cluster [Nv], leader [n_cells]): one cluster per occupied cell, numbered by ascending smallest member."""
    key = (cell[:, 0] << 42) | (cell[:, 1] << 21) | cell[:, 2]
    _, first, inverse = np.unique(key, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    return rank[inverse.reshape(-1)], first[order]


def triangles(F, vc):
    """(mapped [T,3] rotated, keep [T] bool, n_degenerate, n_duplicate)."""
    g = vc[F]
    degenerate = (g[:, 0] == g[:, 1]) | (g[:, 1] == g[:, 2]) | (g[:, 0] == g[:, 2])
    r = np.argmin(g, axis=1)
    rows = np.arange(len(g))
    rot = np.stack([g[rows, r], g[rows, (r + 1) % 3], g[rows, (r + 2) % 3]], 1)
    keep = np.zeros(len(g), bool)
    seen = set()
    for t in np.nonzero(~degenerate)[0]:
        k = tuple(rot[t])
        if k not in seen:
            seen.add(k)
            keep[t] = True
    return rot, keep, int(degenerate.sum()), int((~degenerate).sum() - keep.sum())


def face_cross(V, F):
    P = np.asarray(V, np.float32).astype(np.float64)
    p0, p1, p2 = P[F[:, 0]], P[F[:, 1]], P[F[:, 2]]
    a, b = p1 - p0, p2 - p0
    c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
    return p0, c


def simplify(V, F, C=None, h=None, contraction="quadric", origin=None, remove_unreferenced=True, check_exact=True):
    """The whole of ``lara_amd.meshsimplify.simplify_vertex_clustering`` as a dict: V, F, C, vertex_cluster, n_cells, n_degenerate,
    n_duplicate, n_zero_area, n_clamped, and for the tests x64 (the fp64 positions before the rounding to fp32), raw64 (before
    the clamp), lo / hi (the fp64 boxes), mean64, sums_exact / colors_exact (whether every fp64
    member sum was exact, so that the order of the additions cannot matter; None with check_exact=False), c64."""
    V = np.asarray(V, np.float32).reshape(-1, 3)
    F = np.asarray(F, np.int64).reshape(-1, 3)
    Nv = len(V)
    if F.size and (F.min() < 0 or F.max() >= Nv):
        raise ValueError("a triangle indexes a vertex outside [0, Nv)")
    if Nv == 0:
        return dict(V=V, F=F, C=None if C is None else np.zeros((0, 3), np.float32), vertex_cluster=np.zeros(0, np.int32), n_cells=0,
                    n_degenerate=0, n_duplicate=0, n_zero_area=0, n_clamped=0, x64=np.zeros((0, 3)), raw64=np.zeros((0, 3)),
                    lo=np.zeros((0, 3)), hi=np.zeros((0, 3)), mean64=np.zeros((0, 3)), sums_exact=True)
    cell, o, h32 = cells(V, h, origin)
    vc, leader = clusters(cell)
    n = len(leader)
    P = V.astype(np.float64)
    S = np.zeros((n, 3))
    np.add.at(S, vc, P)                                        # serial, ascending vertex index (the device: a fixed tree)
    cnt = np.bincount(vc, minlength=n).astype(np.float64)
    mean = S / cnt[:, None]
    exact = True
    if check_exact:                                            # (fsum: the correctly rounded sum; tools pass False, it is slow)
        by = np.argsort(vc, kind="stable")
        ends = np.cumsum(cnt.astype(np.int64))
        for g in np.nonzero(cnt > 1)[0]:
            m = P[by[ends[g] - int(cnt[g]):ends[g]]]
            exact &= all(math.fsum(m[:, a]) == S[g, a] for a in range(3))
    else:
        exact = None
    col = col64 = None
    colors_exact = None
    if C is not None:
        C64 = np.asarray(C, np.float32).astype(np.float64)
        SC = np.zeros((n, 3))
        np.add.at(SC, vc, C64)
        col64 = SC / cnt[:, None]
        col = col64.astype(np.float32)
        if check_exact:
            colors_exact = all(math.fsum(C64[by[ends[g] - int(cnt[g]):ends[g]], a]) == SC[g, a]
                               for g in np.nonzero(cnt > 1)[0] for a in range(3))
    p0, c = face_cross(V, F)
    l2 = (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]
    valid = np.isfinite(l2) & (l2 > 0)
    x = mean.copy()
    raw = mean.copy()
    o64, h64 = o.astype(np.float64), float(h32)
    lcell = cell[leader]
    lo = o64[None, :] + lcell * h64
    hi = o64[None, :] + (lcell + 1) * h64
    solved = np.zeros(n, bool)
    if contraction == "quadric":
        Fv, cv, p0v = F[valid], c[valid], p0[valid]
        l = np.sqrt(l2[valid])
        nrm = cv / l[:, None]
        w = 0.5 * l
        A = np.zeros((n, 3, 3))
        b = np.zeros((n, 3))
        gs = vc[Fv].reshape(-1)                                # ascending 3 t + corner
        rep = lambda a: np.repeat(a, 3, axis=0)
        nn, ww, pp = rep(nrm), rep(w), rep(p0v)
        dd = pp - mean[gs]
        d = (nn[:, 0] * dd[:, 0] + nn[:, 1] * dd[:, 1]) + nn[:, 2] * dd[:, 2]
        wn = ww[:, None] * nn
        np.add.at(A, gs, wn[:, :, None] * nn[:, None, :])
        np.add.at(b, gs, (ww * d)[:, None] * nn)
        tr = A[:, 0, 0] + A[:, 1, 1] + A[:, 2, 2]
        solved = tr > 0
        if solved.any():
            M = A[solved] + (LAMBDA * tr[solved])[:, None, None] * np.eye(3)[None]
            y = np.linalg.solve(M, b[solved][:, :, None])[:, :, 0]
            raw[solved] = mean[solved] + y
            x[solved] = np.minimum(np.maximum(raw[solved], lo[solved]), hi[solved])
    elif contraction != "average":
        raise ValueError(contraction)
    rot, keep, n_deg, n_dup = triangles(F, vc)
    ref = np.zeros(n, bool)
    ref[rot[keep].reshape(-1)] = True
    if not remove_unreferenced:
        ref[:] = True
    new = np.cumsum(ref) - 1
    moved = solved & np.any(x != raw, axis=1) & ref
    return dict(V=x[ref].astype(np.float32), F=new[rot[keep]].astype(np.int64).reshape(-1, 3), C=None if col is None else col[ref],
                vertex_cluster=np.where(ref[vc], new[vc], -1).astype(np.int32), n_cells=n, n_degenerate=n_deg, n_duplicate=n_dup,
                n_zero_area=int((~valid).sum()), n_clamped=int(moved.sum()), x64=x[ref], raw64=raw[ref], lo=lo[ref], hi=hi[ref],
                mean64=mean[ref], sums_exact=exact if exact is None else bool(exact), colors_exact=colors_exact,
                c64=None if col64 is None else col64[ref], solved=solved[ref], h32=h32, origin=o)


def outside_count(res, eps):
    """Output vertices whose unclamped solution leaves the box by more than eps (negative: comes within -eps of leaving)."""
    out = np.any((res["raw64"] < res["lo"] - eps) | (res["raw64"] > res["hi"] + eps), axis=1) & res["solved"]
    return int(out.sum())


def count_triangles(V, F, h, origin=None):
    cell, _, _ = cells(V, h, origin)
    vc, _ = clusters(cell)
    return int(triangles(np.asarray(F, np.int64).reshape(-1, 3), vc)[1].sum())


# ---- meshes -----------------------------------------------------------------------------------------------------------------------
def flat_grid(n, step, z=0.25):
    """(n+1)^2 vertices of the plane z = const, 2 n^2 triangles."""
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    V = np.stack([i.reshape(-1) * step, j.reshape(-1) * step, np.full(i.size, z)], 1).astype(np.float32)
    a = (i[:-1, :-1] * (n + 1) + j[:-1, :-1]).reshape(-1)
    b, c, d = a + (n + 1), a + (n + 2), a + 1
    return V, np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(np.int64)


def cube(n=32):
    """The unit cube [-1/2, 1/2]^3 with n x n quads per face, shared vertices, outward triangles."""
    ids, verts, tris = {}, [], []

    def vid(p):
        if p not in ids:
            ids[p] = len(verts)
            verts.append(p)
        return ids[p]

    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, n):
            for i in range(n):
                for j in range(n):
                    q = []
                    for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        p = [0, 0, 0]
                        p[axis], p[u], p[v] = side, i + di, j + dj
                        q.append(vid(tuple(p)))
                    if side == 0:                  # (u x v = +axis: reverse on the low side)
                        q = q[::-1]
                    tris += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    V = (np.array(verts, np.float64) / n - 0.5).astype(np.float32)
    return V, np.array(tris, np.int64)
