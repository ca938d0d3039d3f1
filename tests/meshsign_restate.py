"""include/lara_meshsign.h restated in numpy float64 (no GPU): the crossing of csrc/raycross.h on the restated ray-triangle
function of tests/meshray_restate.py, brute force over all triangles, the counting walk over the restated hierarchy of
tests/meshbvh_restate.py (with the un-inflated slab test on request, for the teeth test), the vote, the lattice in numpy fp32, the
eight counts and the mesh's volume.  tests/test_meshsign.py holds the host entries and the pruning logic to this file;
tests/test_meshsign_gpu.py holds the kernels to it."""
import numpy as np

from tests import meshdist_restate as R
from tests import meshray_restate as RR

F32 = np.float32
MAX_RAYS = 3
DIRECTIONS = np.array([[1, 3 / 8, 11 / 16], [-7 / 16, 1, 5 / 16], [9 / 16, -5 / 16, -1]], F32)
PARITY, WINDING = 0, 1


def cross(ray, p0, p1, p2):
    """(hit, orient, touch) of rays (a ``RR.setup``) against triangles, broadcast: hit exactly when the ray-triangle function
    accepts in [0, +inf); orient = +1 where det < 0, else -1; touch where one of U, V, W is exactly zero; both 0 on a miss."""
    hit = RR.raytri(ray, 0.0, np.inf, p0, p1, p2)[0]
    p0, p1, p2 = (np.asarray(x, F32).astype(np.float64) for x in (p0, p1, p2))
    with np.errstate(all="ignore"):
        Ax, Ay, _ = RR._shear(ray, p0)
        Bx, By, _ = RR._shear(ray, p1)
        Cx, Cy, _ = RR._shear(ray, p2)
        U = Cx * By - Cy * Bx
        V = Ax * Cy - Ay * Cx
        W = Bx * Ay - By * Ax
        det = (U + V) + W
        orient = np.where(det < 0, 1, -1)
        touch = (U == 0) | (V == 0) | (W == 0)
    return hit, np.where(hit, orient, 0).astype(np.int8), hit & touch


def ray_rows(o, d, V, F, chunk=256):
    """(cross [n], wind [n], touched [n]) of the rays o + t d, t >= 0, by brute force over the valid triangles: the raw counts,
    before a touching ray is declared unusable."""
    o, d = np.asarray(o, F32).reshape(-1, 3), np.asarray(d, F32).reshape(-1, 3)
    p0, p1, p2 = R.corners(V, F)
    ok = R.valid_triangles(V, F)
    p0, p1, p2 = p0[ok], p1[ok], p2[ok]
    c, w, t = np.zeros(len(o), np.int64), np.zeros(len(o), np.int64), np.zeros(len(o), bool)
    for s in range(0, len(o), chunk):
        ray = RR.setup(o[s:s + chunk, None, :], d[s:s + chunk, None, :])
        hit, orient, touch = cross(ray, p0[None], p1[None], p2[None])
        c[s:s + chunk], w[s:s + chunk], t[s:s + chunk] = hit.sum(1), orient.astype(np.int64).sum(1), touch.any(1)
    return c, w, t


def usable_rows(c, w, touched, finite):
    """The rows as the entry writes them: cross = -1, wind = 0 for a touching ray and for a point that is not finite."""
    bad = touched | ~finite
    return np.where(bad, -1, c).astype(np.int32), np.where(bad, 0, w).astype(np.int32)


def rows(P, K, V, F):
    """(cross [N, K] int32, wind [N, K] int32) of the points under the first K directions, by brute force."""
    P = np.asarray(P, F32).reshape(-1, 3)
    finite = np.isfinite(P).all(1)
    out = [usable_rows(*ray_rows(P, np.broadcast_to(DIRECTIONS[k], P.shape), V, F), finite) for k in range(K)]
    return np.stack([x[0] for x in out], 1), np.stack([x[1] for x in out], 1)


def walk(bvh, o, d, margin=True):
    """(cross, wind, touched, stats) of one ray by the header's walk over ``bvh`` (a tests/meshbvh_restate.BVH): the stored
    sibling order, a slot entered exactly when it is non-empty and the entry parameter of [0, +inf) is finite.  ``margin=False``
    prunes with the plain slab test: the mistake the tests must be able to see."""
    stats = {"tests": 0, "nodes": 0}
    ray = RR.setup(np.asarray(o, F32), np.asarray(d, F32))
    c = w = 0
    touched = False
    if not ray["ok"] or bvh.n_valid == 0:
        return c, w, touched, stats
    r = RR.scalar_ray(ray)
    top = len(bvh.levels) - 1
    level, pos = top, 0
    while True:
        stats["nodes"] += 1
        e = np.inf
        if pos < len(bvh.levels[level]):          # (beyond n_k: a padding slot, empty)
            box = bvh.levels[level][pos]
            if margin:
                e = RR.box_entry(r, box[:3], box[3:], 0.0, np.inf)
            else:
                e = float(RR.box_entries(ray, box[:3], box[3:], F32(0), F32(np.inf), margin=False))
        descend = False
        if e < np.inf:
            if level > 0:
                level, pos, descend = level - 1, pos << 3, True
            else:
                ids = bvh.rec_id[8 * pos:min(8 * pos + 8, bvh.T)]
                ids = ids[ids >= 0]
                if len(ids):
                    hit, orient, touch = cross(ray, bvh.p[0][ids], bvh.p[1][ids], bvh.p[2][ids])
                    stats["tests"] += len(ids)
                    c, w, touched = c + int(hit.sum()), w + int(orient.astype(np.int64).sum()), touched or bool(touch.any())
        if descend:
            continue
        pos += 1
        while level < top and pos & 7 == 0:
            pos, level = pos >> 3, level + 1
        if level == top:
            break
    return c, w, touched, stats


def vote(cross_rows, wind_rows, rule, dist=None):
    """(inside [N] uint8, status [N] uint8, sdf [N] fp32 or None): the header's vote."""
    cr, wi = np.asarray(cross_rows, np.int64), np.asarray(wind_rows, np.int64)
    K = cr.shape[1]
    usable = cr >= 0
    votes = usable & ((wi != 0) if rule == WINDING else (cr & 1) == 1)
    n_u, n_v = usable.sum(1), votes.sum(1)
    inside = 2 * n_v > n_u
    status = ((n_v != 0) & (n_v != n_u)) * 1 + (n_u < K) * 2 + (n_u == 0) * 4
    sdf = None
    if dist is not None:
        dist = np.asarray(dist, F32)
        sdf = np.where(inside, -dist, dist).astype(F32)
    return inside.astype(np.uint8), status.astype(np.uint8), sdf


def lattice(lo, hi, resolution):
    """([R, R, R, 3] fp32 cell centres, step [3] fp32): every operation in fp32, as `lara_amd.meshsign.lattice`."""
    lo, hi = np.asarray(lo, F32).reshape(3), np.asarray(hi, F32).reshape(3)
    step = ((hi - lo).astype(F32) / F32(resolution)).astype(F32)
    half = (np.arange(resolution, dtype=F32) + F32(0.5)).astype(F32)
    axes = [(lo[a] + (half * step[a]).astype(F32)).astype(F32) for a in range(3)]
    return np.stack(np.meshgrid(*axes, indexing="ij"), -1).astype(F32), step


def counts(inside_a, status_a, inside_b, status_b):
    a, b = np.asarray(inside_a) != 0, np.asarray(inside_b) != 0
    sa, sb = np.asarray(status_a, np.int64), np.asarray(status_b, np.int64)
    return [int(a.sum()), int(b.sum()), int((a & b).sum()), int((a | b).sum()), int((sa & 1).sum()), int((sb & 1).sum()),
            int((sa >> 2 & 1).sum()), int((sb >> 2 & 1).sum())]


def box(V, F):
    """(lo, hi) fp32 of the valid triangles' vertices."""
    ok = R.valid_triangles(V, F)
    P = np.stack(R.corners(V, F), 1)[ok]
    return P.min((0, 1)), P.max((0, 1))


def volume(V, F):
    """(signed volume, area, valid triangles, sum of |volume terms| / 6, sum of area terms / 2) in float64, about the centre of
    the box as the header has it; the last two carry the summation-order bar."""
    ok = R.valid_triangles(V, F)
    p0, p1, p2 = (x[ok].astype(np.float64) for x in R.corners(V, F))
    if not ok.any():
        return 0.0, 0.0, 0, 0.0, 0.0
    lo, hi = box(V, F)
    c = 0.5 * lo.astype(np.float64) + 0.5 * hi.astype(np.float64)
    a, b, e = p0 - c, p1 - c, p2 - c
    term = R._dot(a, R._cross(b, e))
    n = R._cross(p1 - p0, p2 - p0)
    ar = np.sqrt(R._dot(n, n))
    return float(term.sum() / 6), float(ar.sum() / 2), int(ok.sum()), float(np.abs(term).sum() / 6), float(ar.sum() / 2)
