"""include/lara_meshbvh.h restated in numpy (no GPU): the keys with the fp32 cell rule, the sorted order, the records, every
level's boxes, the margined bound in float64, and the walk itself -- seed, fixed order, strict skip rule -- on the float64 distance
of tests/meshdist_restate.py.  tests/test_meshbvh.py holds the host entry and the pruning logic to this file;
tests/test_meshbvh_gpu.py holds the kernels to it."""
import numpy as np

from tests import meshdist_restate as R

F32 = np.float32
MAX_LEVELS = 9
REL, ABS = 2.0 ** -12, 2.0 ** -40
INVALID = 1 << 62
NONE = 2 ** 31 - 1


def spread(x):
    """Bit b of the low 10 bits -> bit 3 b."""
    x = np.asarray(x, np.uint64)
    return sum(((x >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b) for b in range(10))


def cells(c, lo, inv):
    """clamp(floor((c - lo) inv), 0, 1023) per axis in fp32; a NaN goes to cell 0."""
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor(((np.asarray(c, F32) - lo).astype(F32) * inv).astype(F32))
    return np.where(f >= 0, np.where(f < 1024, f, 1023), 0).astype(np.int64)      # (a NaN fails f >= 0)


def morton(c, lo, inv):
    k = cells(c, lo, inv)
    return spread(k[..., 0]) | (spread(k[..., 1]) << np.uint64(1)) | (spread(k[..., 2]) << np.uint64(2))


def level_counts(T):
    n, out = (T + 7) // 8, []
    while True:
        out.append(n)
        if n == 1:
            return out
        n = (n + 7) // 8


def nbytes(T):
    """The header's formula."""
    def A(x):
        return (x + 255) // 256 * 256
    return 256 + A(8 * T) + A(48 * T) + A(24 * 1024) + sum(A(24 * ((n + 7) // 8 * 8)) for n in level_counts(T))


def bound(q, lo, hi, margin=True):
    """The margined bound of csrc/boxbound.h for one (query, box), float64 in its operation order; ``margin=False``: s alone."""
    q, lo, hi = (np.asarray(x, F32).astype(np.float64) for x in (q, lo, hi))
    if not lo[0] <= hi[0]:
        return np.inf
    g = np.maximum(np.maximum(lo - q, q - hi), 0.0)
    s = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
    if not margin:
        return s
    M = max(np.abs(q).max(), np.abs(lo).max(), np.abs(hi).max())
    b = s - (REL * s + ABS * (M * M))
    return b if b > 0.0 else 0.0


def bounds(q, lo, hi, margin=True):
    """``bound`` over [n,3] arrays."""
    q, lo, hi = (np.asarray(x, F32).astype(np.float64) for x in (q, lo, hi))
    g = np.maximum(np.maximum(lo - q, q - hi), 0.0)
    s = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
    if margin:
        M = np.maximum(np.abs(q).max(1), np.maximum(np.abs(lo).max(1), np.abs(hi).max(1)))
        s = np.maximum(s - (REL * s + ABS * (M * M)), 0.0)
    return np.where(lo[:, 0] <= hi[:, 0], s, np.inf)


class BVH:
    """The header's build in numpy.  keys (unsorted, int64), order (the sorted position -> key), records [T,12] fp32 with the id's
    bits in column 9, levels: a list of [n_k, 6] fp32 boxes (lo, hi), counts [bad, valid, T, levels]."""

    def __init__(self, V, F):
        V, F = np.asarray(V, F32), np.asarray(F, np.int64)
        self.T = T = len(F)
        self.ok = ok = R.valid_triangles(V, F)
        self.p = p = R.corners(V, F)
        P = np.stack(p, 1)                              # [T, 3 corners, 3]
        self.lo, self.inv = np.zeros(3, F32), np.zeros(3, F32)
        if ok.any():
            lo, hi = P[ok].min((0, 1)), P[ok].max((0, 1))
            with np.errstate(over="ignore", divide="ignore"):
                ext = (hi - lo).astype(F32)
                inv = np.where(ext > 0, F32(1024) / np.where(ext > 0, ext, F32(1)), F32(0)).astype(F32)
            self.lo, self.inv = lo.astype(F32), np.where(inv < np.inf, inv, F32(0)).astype(F32)
        mn, mx = P.min(1), P.max(1)
        with np.errstate(invalid="ignore", over="ignore"):
            centre = (F32(0.5) * mn + F32(0.5) * mx).astype(F32)
        ids = np.arange(T, dtype=np.uint64)
        keys = np.where(ok, (morton(centre, self.lo, self.inv) << np.uint64(26)) | ids, np.uint64(INVALID) | ids)
        self.keys = keys.astype(np.int64)
        self.sorted_keys = np.sort(self.keys)
        self.order = (self.sorted_keys & ((1 << 26) - 1)).astype(np.int64)      # sorted position -> triangle id
        self.n_valid = int(ok.sum())
        rec = np.zeros((T, 12), F32)
        v = ok[self.order]
        rec[:, :9] = np.where(v[:, None], P[self.order].reshape(T, 9), F32(0))
        rec[:, 9] = np.where(v, self.order, -1).astype(np.int32).view(F32)
        self.records = rec
        self.rec_id = np.where(v, self.order, -1)
        self.counts = [int((~ok).sum()), self.n_valid, T, len(level_counts(T))]
        # level 0 from the valid records, level k + 1 from level k; an empty slot is (+inf, -inf)
        self.levels = []
        n0 = (T + 7) // 8
        lo_r = np.full((8 * n0, 3), np.inf, F32)
        hi_r = np.full((8 * n0, 3), -np.inf, F32)
        Ps = P[self.order]
        lo_r[:T][v], hi_r[:T][v] = Ps[v].min(1), Ps[v].max(1)
        boxes = np.concatenate([lo_r.reshape(n0, 8, 3).min(1), hi_r.reshape(n0, 8, 3).max(1)], 1)
        self.levels.append(boxes)
        while len(boxes) > 1:
            n = (len(boxes) + 7) // 8
            pad = np.concatenate([boxes, np.tile(np.array([np.inf] * 3 + [-np.inf] * 3, F32), (8 * n - len(boxes), 1))])
            boxes = np.concatenate([pad[:, :3].reshape(n, 8, 3).min(1), pad[:, 3:].reshape(n, 8, 3).max(1)], 1)
            self.levels.append(boxes)
        assert [len(b) for b in self.levels] == level_counts(T)

    def _leaf(self, best, q, leaf, stats):
        ids = self.rec_id[8 * leaf:min(8 * leaf + 8, self.T)]
        ids = ids[ids >= 0]
        if len(ids) == 0:
            return best
        d2 = R.point_triangle(q[None], self.p[0][ids], self.p[1][ids], self.p[2][ids])[0]
        stats["tests"] += len(ids)
        for d, i in zip(d2.tolist(), ids.tolist()):          # in record order, as the kernel meets them
            if d < best[0] or (d == best[0] and i < best[1]):
                best = (d, i)
        return best

    def search(self, q, margin=True, strict=True):
        """(face, d2, stats) of one query by the header's walk.  ``margin=False`` prunes with the unmargined s, ``strict=False``
        also skips a node whose bound EQUALS the best d2: the two mistakes the tests must be able to see."""
        q = np.asarray(q, F32)
        stats = {"tests": 0, "nodes": 0}
        if not np.isfinite(q).all() or self.n_valid == 0:
            return -1, np.inf, stats
        best = (np.inf, NONE)
        want = int(morton(q, self.lo, self.inv)) << 26
        a = int(np.searchsorted(self.sorted_keys[:self.n_valid], want, side="left"))
        best = self._leaf(best, q, min(a, self.n_valid - 1) >> 3, stats)
        top = len(self.levels) - 1
        level, idx = top, 0
        while True:
            stats["nodes"] += 1
            b = np.inf
            if idx < len(self.levels[level]):          # (beyond n_k: a padding slot, empty)
                box = self.levels[level][idx]
                b = bound(q, box[:3], box[3:], margin)
            if b < np.inf and not (b > best[0] or (not strict and b == best[0])):
                if level > 0:
                    level, idx = level - 1, idx << 3
                    continue
                best = self._leaf(best, q, idx, stats)
            idx += 1
            while level < top and idx & 7 == 0:
                idx, level = idx >> 3, level + 1
            if level == top:
                break
        return (best[1] if best[1] != NONE else -1), best[0], stats
