"""include/lara_meshwind.h restated in numpy float64 (no GPU): the term of csrc/solidangle.h in the header's operation order
(with the `num == 0` rule, and without it on request, for the teeth test), brute force over all valid triangles, the moments over
the restated hierarchy of tests/meshbvh_restate.py in the header's summation order, the walk with its counters -- all points in
lockstep, each with a state of its own, so a point's sum is added in its walk's order -- and the classification.
tests/test_meshwind.py holds the host entries and the approximation to this file; tests/test_meshwind_gpu.py holds the kernels to it."""
import numpy as np

from tests import meshbvh_restate as RB
from tests import meshdist_restate as R

F32 = np.float32
FOUR_PI = 4.0 * np.pi
U64 = 2.0 ** -53
SLOT_BYTES, HEADER_BYTES = 64, 256


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def solid(q, p0, p1, p2, rule=True, return_num=False):
    """Omega of the triangles seen from the points, broadcast, float64 on the fp32 inputs in the header's order.  ``rule=False``:
    a bare atan2, the mistake the tests must be able to see."""
    q, p0, p1, p2 = (np.asarray(x, F32).astype(np.float64) for x in (q, p0, p1, p2))
    with np.errstate(all="ignore"):
        a, b, c = p0 - q, p1 - q, p2 - q
        num = _dot(a, _cross(b, c))
        la, lb, lc = np.sqrt(_dot(a, a)), np.sqrt(_dot(b, b)), np.sqrt(_dot(c, c))
        den = (la * (lb * lc) + _dot(b, c) * la) + (_dot(a, b) * lc + _dot(c, a) * lb)
        omega = 2.0 * np.arctan2(num, den)
    if rule:
        omega = np.where(num == 0, 0.0, omega)
    return (omega, num) if return_num else omega


def triangles(V, F):
    """(p0, p1, p2) fp32 of the valid triangles, in id order."""
    if len(F) == 0:
        z = np.zeros((0, 3), F32)
        return z, z, z
    ok = R.valid_triangles(V, F)
    return tuple(x[ok] for x in R.corners(V, F))


def brute(P, V, F, rule=True, chunk=128):
    """(w [N], sum of |terms| [N]) float64 by brute force over the valid triangles; NaN for a point that is not finite."""
    P = np.asarray(P, F32).reshape(-1, 3)
    p0, p1, p2 = triangles(V, F)
    w, mag = np.zeros(len(P)), np.zeros(len(P))
    for s in range(0, len(P), chunk):
        om = solid(P[s:s + chunk, None, :], p0[None], p1[None], p2[None], rule)
        w[s:s + chunk], mag[s:s + chunk] = om.sum(1), np.abs(om).sum(1)
    fin = np.isfinite(P).all(1)
    return np.where(fin, w / FOUR_PI, np.nan), np.where(fin, mag, 0.0)


def layout(T):
    """([(byte offset, stored slots) per level], total bytes) of the moments buffer."""
    out, o = [], HEADER_BYTES
    for n in RB.level_counts(T):
        stored = (n + 7) // 8 * 8
        out.append((o, stored))
        o += SLOT_BYTES * stored
    return out, o


class Moments:
    """The header's per-node data over ``bvh`` (a tests/meshbvh_restate.BVH): levels, a list of [stored_k, 8] float64 arrays
    {N, A, c, r2}; ``flat`` is their concatenation and ``first[k]`` level k's first row in it."""

    def __init__(self, bvh):
        self.bvh, T = bvh, bvh.T
        lay, self.nbytes = layout(T)
        v = bvh.rec_id >= 0
        p = [bvh.records[:, 3 * k:3 * k + 3].astype(np.float64) for k in range(3)]
        n = _cross(p[1] - p[0], p[2] - p[0])
        At = np.where(v, 0.5 * np.sqrt(_dot(n, n)), 0.0)
        ct = ((p[0] + p[1]) + p[2]) / 3.0
        stored = lay[0][1]

        def padded(x, rows):
            out = np.zeros((rows,) + x.shape[1:])
            out[:len(x)] = x
            return out
        half_n = padded(np.where(v[:, None], 0.5 * n, 0.0), 8 * stored).reshape(stored, 8, 3)
        a = padded(At, 8 * stored).reshape(stored, 8)
        ac = padded(np.where(v[:, None], At[:, None] * ct, 0.0), 8 * stored).reshape(stored, 8, 3)
        use = padded(v.astype(np.float64), 8 * stored).reshape(stored, 8) > 0
        self.levels = []
        for k, (_, stored) in enumerate(lay):
            if k > 0:
                child = self.levels[-1]                          # the children below n_{k-1}, as they are stored
                half_n, a = child[:, :3].reshape(-1, 8, 3), child[:, 3].reshape(-1, 8)
                ac = (child[:, 3:4] * child[:, 4:7]).reshape(-1, 8, 3)
                assert len(a) <= stored
                half_n, a, ac = (padded(x, stored) for x in (half_n, a, ac))
                use = np.arange(8 * stored).reshape(stored, 8) < len(bvh.levels[k - 1])
            N, A, S = np.zeros((stored, 3)), np.zeros(stored), np.zeros((stored, 3))
            for j in range(8):                                   # in stored order, one addition each
                N = np.where(use[:, j, None], N + half_n[:, j], N)
                A = np.where(use[:, j], A + a[:, j], A)
                S = np.where(use[:, j, None], S + ac[:, j], S)
            boxes = np.full((stored, 6), np.nan)
            boxes[:len(bvh.levels[k])] = bvh.levels[k].astype(np.float64)
            any_ = A > 0
            with np.errstate(all="ignore"):
                c = np.where(any_[:, None], S / np.where(any_, A, 1.0)[:, None], 0.0)
                below, above = c - boxes[:, :3], boxes[:, 3:] - c
                m = np.maximum(below * below, above * above)
                r2 = np.where(any_, (m[:, 0] + m[:, 1]) + m[:, 2], 0.0)
            lev = np.concatenate([np.where(any_[:, None], N, 0.0), np.where(any_, A, 0.0)[:, None], c, r2[:, None]], 1)
            self.levels.append(lev)
        self.flat = np.concatenate(self.levels)
        self.first = np.cumsum([0] + [len(x) for x in self.levels])[:-1]

    def buffer_slots(self):
        """The buffer's slot region as int64 bit patterns, [all stored slots, 8]."""
        return np.ascontiguousarray(self.flat).view(np.int64)


def walk(M, P, beta):
    """(w [N], n_tri [N] int32, n_far [N] int32, sum of |terms| [N]) of the points by the header's walk over the moments ``M``."""
    bvh = M.bvh
    P = np.asarray(P, F32).reshape(-1, 3)
    n = len(P)
    q = P.astype(np.float64)
    fin = np.isfinite(P).all(1)
    total, mag = np.zeros(n), np.zeros(n)
    n_tri, n_far = np.zeros(n, np.int32), np.zeros(n, np.int32)
    top = len(M.levels) - 1
    level, pos = np.full(n, top), np.zeros(n, np.int64)
    active = fin.copy()
    with np.errstate(all="ignore"):
        bb = np.float64(beta) * np.float64(beta)
    rec_p = [bvh.records[:, 3 * k:3 * k + 3] for k in range(3)]
    while active.any():
        idx = np.nonzero(active)[0]
        lv, ps = level[idx], pos[idx]
        m = M.flat[M.first[lv] + ps]
        d = m[:, 4:7] - q[idx]
        d2 = _dot(d, d)
        with np.errstate(all="ignore"):
            live = m[:, 3] > 0
            far = live & (d2 > bb * m[:, 7])
            term = _dot(d, m[:, :3]) / (d2 * np.sqrt(d2))
        f = idx[far]
        total[f] += term[far]
        mag[f] += np.abs(term[far])
        n_far[f] += 1
        leaf = live & ~far & (lv == 0)
        li, lp = idx[leaf], ps[leaf]
        for k in range(8):
            r = 8 * lp + k
            ok = r < bvh.T
            ok[ok] = bvh.rec_id[r[ok]] >= 0
            i, r = li[ok], r[ok]
            om = solid(P[i], rec_p[0][r], rec_p[1][r], rec_p[2][r])
            total[i] += om
            mag[i] += np.abs(om)
            n_tri[i] += 1
        down = live & ~far & (lv > 0)
        level[idx[down]] -= 1
        pos[idx[down]] <<= 3
        step = idx[~down]
        pos[step] += 1
        while True:
            up = step[(level[step] < top) & (pos[step] & 7 == 0)]
            if len(up) == 0:
                break
            pos[up] >>= 3
            level[up] += 1
        active[step[level[step] == top]] = False
    return np.where(fin, total / FOUR_PI, np.nan), n_tri, n_far, mag


def winding(V, F, P, beta):
    """``walk`` from the mesh: zeros for T = 0 (there is no hierarchy to walk), NaN for the points that are not finite."""
    P = np.asarray(P, F32).reshape(-1, 3)
    if len(F) == 0:
        z = np.zeros(len(P), np.int32)
        return np.where(np.isfinite(P).all(1), 0.0, np.nan), z, z, np.zeros(len(P))
    return walk(Moments(RB.BVH(V, F)), P, beta)


def bar(n_terms, mag):
    """The summation bar of the issue on w: (n + 4) 2^-53 sum |term| / 4 pi."""
    return (np.asarray(n_terms, np.float64) + 4) * U64 * mag / FOUR_PI


def classify(w, threshold=0.5, band=0.05, dist=None):
    """(inside [N] uint8, status [N] uint8, sdf [N] fp32 or None): the header's classification."""
    w = np.asarray(w, np.float64)
    with np.errstate(invalid="ignore"):
        inside = w > threshold
        status = (np.abs(w - threshold) < band) * 1 + (~np.isfinite(w)) * 4
    sdf = None
    if dist is not None:
        dist = np.asarray(dist, F32)
        sdf = np.where(inside, -dist, dist).astype(F32)
    return inside.astype(np.uint8), status.astype(np.uint8), sdf
