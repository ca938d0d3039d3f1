"""include/lara_meshray.h restated in numpy float64 (no GPU): the ray-triangle function of csrc/raytri.h in its operation
order, the unsheared triple-product form it replaces (for the teeth test), the margined entry parameter of csrc/raybox.h and an
un-inflated slab test, brute force over all triangles, and the walk over the restated hierarchy of tests/meshbvh_restate.py with
both sibling orders, counting triangle tests.  tests/test_meshray.py holds the host entries and the pruning logic to this file;
tests/test_meshray_gpu.py holds the kernels to it."""
import numpy as np

from tests import meshdist_restate as R

F32 = np.float32
SANITY, INFLATE, REL = 2.0 ** -20, 2.0 ** -19, 2.0 ** -40
NONE = 2 ** 31 - 1
MAX_EYES = 64
EPS = 2.0 ** -18          # the ambiguous band of the visibility cut, as tests/depthsurface_restate.py


def _pick(a, k):
    return np.take_along_axis(a, np.broadcast_to(np.asarray(k), a.shape[:-1])[..., None], -1)[..., 0]


def setup(o, d):
    """The per-ray constants of [..., 3] fp32 origins and directions: a dict of float64 arrays (o, d, inv [..., 3]; Sx, Sy, Sz),
    int arrays kx, ky, kz and ok."""
    o, d = np.asarray(o, F32).astype(np.float64), np.asarray(d, F32).astype(np.float64)
    ok = np.isfinite(o).all(-1) & np.isfinite(d).all(-1)
    ad = np.abs(np.where(np.isnan(d), 0.0, d))
    kz = ad.argmax(-1)                                   # the first of the largest
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    dz = _pick(d, kz)
    with np.errstate(invalid="ignore"):
        swap = dz < 0
    kx, ky = np.where(swap, ky, kx), np.where(swap, kx, ky)
    with np.errstate(invalid="ignore"):
        ok = ok & (dz != 0)
    den = np.where(ok, dz, 1.0)
    with np.errstate(all="ignore"):
        Sx, Sy, Sz = _pick(d, kx) / den, _pick(d, ky) / den, 1.0 / den
        inv = 1.0 / np.where((d != 0) & ok[..., None], d, 1.0)
    return {"o": o, "d": d, "inv": inv, "Sx": Sx, "Sy": Sy, "Sz": Sz, "kx": kx, "ky": ky, "kz": kz, "ok": ok}


def _at(ray, idx):
    return {k: v[idx] for k, v in ray.items()}


def _shear(ray, p):
    a = p - ray["o"]
    az = _pick(a, ray["kz"])
    return _pick(a, ray["kx"]) - ray["Sx"] * az, _pick(a, ray["ky"]) - ray["Sy"] * az, ray["Sz"] * az


def raytri(ray, t_min, t_max, p0, p1, p2, sanity=True):
    """(hit, t, bary [..., 3], rejected) of rays against triangles, broadcast over leading axes (the ray's arrays against
    p[..., 3]); t = +inf and bary = NaN on a miss.  ``rejected``: everything held but the sanity clause.  ``sanity=False``
    leaves the clause out."""
    p0, p1, p2 = (np.asarray(x, F32).astype(np.float64) for x in (p0, p1, p2))
    t_min, t_max = np.asarray(t_min, F32).astype(np.float64), np.asarray(t_max, F32).astype(np.float64)
    with np.errstate(all="ignore"):
        Ax, Ay, Az = _shear(ray, p0)
        Bx, By, Bz = _shear(ray, p1)
        Cx, Cy, Cz = _shear(ray, p2)
        U = Cx * By - Cy * Bx
        V = Ax * Cy - Ay * Cx
        W = Bx * Ay - By * Ax
        side = ((U >= 0) & (V >= 0) & (W >= 0)) | ((U <= 0) & (V <= 0) & (W <= 0))
        det = (U + V) + W
        t = ((U * Az + V * Bz) + W * Cz) / det
        pre = ray["ok"] & side & (det != 0) & (t_min <= t) & (t <= t_max)
        mn, mx = np.minimum(np.minimum(p0, p1), p2), np.maximum(np.maximum(p0, p1), p2)
        m = SANITY * np.maximum(np.abs(ray["o"]), np.maximum(np.abs(mn), np.abs(mx)))
        x = ray["o"] + t[..., None] * ray["d"]
        inside = ((x >= mn - m) & (x <= mx + m)).all(-1)
        hit = pre & inside if sanity else pre
        b = np.stack([U / det, V / det, W / det], -1)
    return hit, np.where(hit, t, np.inf), np.where(hit[..., None], b, np.nan), pre & ~inside


def triple_product_hits(o, d, p0, p1, p2):
    """The unsheared form: the signs of d . (b x c), d . (c x a), d . (a x b) of the vertices relative to o, both sides, zeros
    inclusive, t > 0 by the plane: the test a ray can slip through.  Broadcast; float64 on fp32 inputs."""
    o, d, p0, p1, p2 = (np.asarray(x, F32).astype(np.float64) for x in (o, d, p0, p1, p2))
    a, b, c = p0 - o, p1 - o, p2 - o
    U, V, W = R._dot(d, R._cross(b, c)), R._dot(d, R._cross(c, a)), R._dot(d, R._cross(a, b))
    side = ((U >= 0) & (V >= 0) & (W >= 0)) | ((U <= 0) & (V <= 0) & (W <= 0))
    det = (U + V) + W
    n = R._cross(p1 - p0, p2 - p0)
    with np.errstate(all="ignore"):
        t = R._dot(a, n) / R._dot(d, n)
    return side & (det != 0) & (t >= 0)


def box_entries(ray, lo, hi, t_min, t_hi, margin=True):
    """The entry parameter of csrc/raybox.h, broadcast; ``margin=False``: the plain slab test, neither inflated nor widened."""
    lo32, hi32 = np.asarray(lo, F32), np.asarray(hi, F32)
    lo, hi = lo32.astype(np.float64), hi32.astype(np.float64)
    near = np.asarray(t_min, F32).astype(np.float64) + np.zeros(np.broadcast(ray["ok"], lo[..., 0]).shape)
    far = np.asarray(t_hi, F32).astype(np.float64) + np.zeros(near.shape)
    beside = np.zeros(near.shape, bool)
    with np.errstate(all="ignore"):
        for a in range(3):
            o, d, inv = ray["o"][..., a], ray["d"][..., a], ray["inv"][..., a]
            e = INFLATE * np.maximum(np.abs(o), np.maximum(np.abs(lo[..., a]), np.abs(hi[..., a]))) if margin else 0.0
            l, h = lo[..., a] - e, hi[..., a] + e
            t1, t2 = (l - o) * inv, (h - o) * inv
            n, f = np.where(t1 < t2, t1, t2), np.where(t1 < t2, t2, t1)
            if margin:
                n, f = n - REL * np.abs(n), f + REL * np.abs(f)
            zero = d == 0
            beside |= zero & ~((o >= l) & (o <= h))
            near = np.where(~zero & (n > near), n, near)
            far = np.where(~zero & (f < far), f, far)
        ok = (lo32[..., 0] <= hi32[..., 0]) & ray["ok"] & ~beside & (near <= far)
    return np.where(ok, near, np.inf)


def box_entry(r, lo, hi, t_min, t_hi):
    """``box_entries`` for one ray (``r``: python floats, from ``scalar_ray``) and one box: the walk's inner function."""
    if not lo[0] <= hi[0] or not r["ok"]:
        return np.inf
    near, far = t_min, t_hi
    for a in range(3):
        o, d, l0, h0 = r["o"][a], r["d"][a], float(lo[a]), float(hi[a])
        e = INFLATE * max(abs(o), abs(l0), abs(h0))
        l, h = l0 - e, h0 + e
        if d == 0.0:
            if not (l <= o <= h):
                return np.inf
            continue
        t1, t2 = (l - o) * r["inv"][a], (h - o) * r["inv"][a]
        n, f = (t1, t2) if t1 < t2 else (t2, t1)
        n, f = n - REL * abs(n), f + REL * abs(f)
        near, far = (n if n > near else near), (f if f < far else far)
    return near if near <= far else np.inf


def scalar_ray(ray):
    """A one-ray ``setup`` as python floats and lists, for ``box_entry``."""
    return {"o": ray["o"].tolist(), "d": ray["d"].tolist(), "inv": ray["inv"].tolist(), "ok": bool(ray["ok"])}


def _windows(t_min, t_max, n):
    return (np.broadcast_to(np.asarray(t_min, F32), (n,)), np.broadcast_to(np.asarray(t_max, F32), (n,)))


def all_hits(o, d, V, F, t_min=0.0, t_max=np.inf, chunk=256, sanity=True):
    """(t [R, T] float64, +inf where the ray does not hit or the triangle is invalid; bary [R, T, 3]; rejected [R, T])."""
    o, d = np.asarray(o, F32).reshape(-1, 3), np.asarray(d, F32).reshape(-1, 3)
    p0, p1, p2 = R.corners(V, F)
    ok = R.valid_triangles(V, F)
    lo, hi = _windows(t_min, t_max, len(o))
    t, b, rej = np.empty((len(o), len(p0))), np.empty((len(o), len(p0), 3)), np.empty((len(o), len(p0)), bool)
    for s in range(0, len(o), chunk):
        ray = setup(o[s:s + chunk, None, :], d[s:s + chunk, None, :])
        _, t[s:s + chunk], b[s:s + chunk], rej[s:s + chunk] = raytri(ray, lo[s:s + chunk, None], hi[s:s + chunk, None], p0[None], p1[None],
                                                                      p2[None], sanity)
    t[:, ~ok], b[:, ~ok], rej[:, ~ok] = np.inf, np.nan, False
    return t, b, rej


def brute(o, d, V, F, t_min=0.0, t_max=np.inf):
    """(t [R] fp32 = (float)t, face [R] int32, bary [R,3] fp32, t [R] float64, hits per ray, rejections per ray): the first
    minimum of t = the smallest face id on a tie; +inf, -1, NaN without a hit."""
    t, b, rej = all_hits(o, d, V, F, t_min, t_max)
    face = t.argmin(1) if t.shape[1] else np.zeros(len(t), np.int64)
    k = np.arange(len(t))
    best = t[k, face] if t.shape[1] else np.full(len(t), np.inf)
    hit = np.isfinite(best)
    bary = np.where(hit[:, None], b[k, face] if t.shape[1] else np.nan, np.nan)
    with np.errstate(over="ignore"):          # (a t beyond fp32's range rounds to +inf, as the kernel's (float)t does)
        return (best.astype(F32), np.where(hit, face, -1).astype(np.int32), bary.astype(F32), best, np.isfinite(t).sum(1), rej.sum(1))


def visibility(points, eyes, V, F, skip=None, shrink=2.0 ** -10):
    """(seen [N] int64, ambiguous [N, E] bool): bit e is set when no triangle but ``skip[i]`` is hit by the ray from eye e with
    d = fl32(p - eye) inside [0, fl32(1 - shrink)].  ``ambiguous``: some such triangle is hit, with any window, at a t within a
    relative 2^-18 of the cut."""
    P, E = np.asarray(points, F32).reshape(-1, 3), np.asarray(eyes, F32).reshape(-1, 3)
    cut = F32(1) - F32(shrink)
    seen, amb = np.zeros(len(P), np.int64), np.zeros((len(P), len(E)), bool)
    fin = np.isfinite(P).all(1)
    for e in range(len(E)):
        with np.errstate(all="ignore"):
            d = (P - E[e]).astype(F32)
        o = np.broadcast_to(E[e], P.shape)
        t = all_hits(o, d, V, F, -np.inf, np.inf)[0]
        if skip is not None:
            s = np.asarray(skip, np.int64)
            has = (s >= 0) & (s < t.shape[1])
            t[np.nonzero(has)[0], s[has]] = np.inf
        inside = (t >= 0) & (t <= np.float64(cut))
        amb[:, e] = fin & (np.abs(t - np.float64(cut)) <= EPS * np.float64(cut)).any(1)
        seen |= np.where(fin & ~inside.any(1), np.int64(1) << np.int64(e), np.int64(0))
    return seen, amb


def pixel_rays(k, pose, H, W):
    """(origins, directions) [V, H, W, 3] fp32 of the rays through the pixel centres of cameras (k [V,4] fp32, pose [V,16] fp32 =
    c2w, as ``depthsurface.cameras`` returns them): float64 in the written order, rounded once; d has view-space z = 1, so t is
    the view-space depth."""
    k, M = np.asarray(k, F32).astype(np.float64), np.asarray(pose, F32).astype(np.float64).reshape(-1, 4, 4)
    x, y = np.arange(W, dtype=np.float64)[None, None, :], np.arange(H, dtype=np.float64)[None, :, None]
    a = ((x + 0.5) - k[:, 2, None, None]) / k[:, 0, None, None] + 0.0 * y
    b = ((y + 0.5) - k[:, 3, None, None]) / k[:, 1, None, None] + 0.0 * x
    d = np.stack([(M[:, j, 0, None, None] * a + M[:, j, 1, None, None] * b) + M[:, j, 2, None, None] for j in range(3)], -1)
    o = np.broadcast_to(M[:, None, None, :3, 3], d.shape)
    return o.astype(F32), d.astype(F32)


def walk(bvh, o, d, t_min=0.0, t_max=np.inf, masked=True, strict=True, margin=True, any_hit=False, skip=-1):
    """(face, t, stats) of one ray by the header's walk over ``bvh`` (a tests/meshbvh_restate.BVH).  ``masked``: sibling c is slot
    c ^ mask, else the stored order.  ``strict=False`` also skips a slot whose entry EQUALS the best t, ``margin=False`` prunes
    with the plain slab test: the two mistakes the tests must be able to see.  ``any_hit``: ends at the first accepted triangle
    (face = that triangle)."""
    stats = {"tests": 0, "nodes": 0}
    ray = setup(np.asarray(o, F32), np.asarray(d, F32))
    lo, hi = float(np.float64(F32(t_min))), float(np.float64(F32(t_max)))
    if not ray["ok"] or bvh.n_valid == 0:
        return -1, np.inf, stats
    r = scalar_ray(ray)
    dd = r["d"]
    mask = ((dd[0] < 0) | (dd[1] < 0) << 1 | (dd[2] < 0) << 2) if masked else 0
    best = (np.inf, NONE)
    top = len(bvh.levels) - 1
    level, pos = top, 0
    while True:
        stats["nodes"] += 1
        slot = pos ^ mask if level < top else pos
        e = np.inf
        if slot < len(bvh.levels[level]):          # (beyond n_k: a padding slot, empty)
            box = bvh.levels[level][slot]
            if margin:
                e = box_entry(r, box[:3], box[3:], lo, hi)
            else:
                e = float(box_entries(ray, box[:3], box[3:], F32(t_min), F32(t_max), margin=False))
        if e < np.inf and not (e > best[0] or (not strict and e == best[0])):
            if level > 0:
                level, pos = level - 1, slot << 3
                continue
            ids = bvh.rec_id[8 * slot:min(8 * slot + 8, bvh.T)]
            ids = ids[(ids >= 0) & (ids != skip)]
            if len(ids):
                hit, t, _, _ = raytri(ray, F32(t_min), F32(t_max), bvh.p[0][ids], bvh.p[1][ids], bvh.p[2][ids])
                for k, (h, tt, i) in enumerate(zip(hit.tolist(), t.tolist(), ids.tolist())):          # in record order
                    stats["tests"] += 1
                    if not h:
                        continue
                    if any_hit:
                        return i, tt, stats
                    if tt < best[0] or (tt == best[0] and i < best[1]):
                        best = (tt, i)
        pos += 1
        while level < top and pos & 7 == 0:
            parent, level = (pos >> 3) - 1, level + 1
            pos = (parent ^ mask if level < top else parent) + 1
        if level == top:
            break
    return (best[1] if best[1] != NONE else -1), best[0], stats
