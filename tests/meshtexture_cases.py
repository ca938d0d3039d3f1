"""The (mesh, layout, views) cases tests/test_meshtexture.py replays through the host entries and tests/test_meshtexture_gpu.py through
the kernels, each held to tests/meshtexture_restate.py.  Meshes: the 1 280-face icosphere, the 8 x 64 UV sphere with its pole
slivers, the soups with triangles without area and with invalid triangles (unowned patches), one triangle, an odd T = 11, T = 0, and
two layers (the icosphere around a copy scaled by 0.5).  Layouts: S = 3, 4, 7, 8, C such that the last row is partly empty, one
C = 1.  Views (48 x 64): four on an orbit with two focal lengths, one inside the sphere looking out, one whose image border cuts the
sphere; V = 0 and V = 64 on the small mesh.  The source images are made here: a float64 ray cast of the ICOSPHERE (every triangle whose
bounding ball the ray meets is tested, so it is brute force with the misses left out), coloured by an analytic field of the hit
point; the other meshes are baked from the same images, which is all the bit comparisons need.  Everything is computed once, shared
by the tests, and read-only."""
import numpy as np

from tests import meshdist_cases as C
from tests import meshdist_restate as R
from tests import meshtexture_restate as X

F32 = np.float32
H, W = 48, 64
_cache = {}


def field(p, wave):
    """The analytic colour of a point: one sine per channel along one axis each, in [0, 1]."""
    p = np.asarray(p, np.float64)
    return 0.5 + 0.5 * np.sin(wave * p + np.array([0.0, 1.0, 2.0]))


def look_at(eye, target=(0, 0, 0), up=(0, 0, 1)):
    """c2w [4,4] float64: view-space z forward, x right, y down (``depthsurface.cameras``' convention)."""
    eye = np.asarray(eye, np.float64)
    z = np.asarray(target, np.float64) - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, np.asarray(up, np.float64))
    x /= np.linalg.norm(x)
    M = np.eye(4)
    M[:3, 0], M[:3, 1], M[:3, 2], M[:3, 3] = x, np.cross(z, x), z, eye
    return M


def intrinsics(focal, h=H, w=W):
    return np.array([[focal, 0, w / 2], [0, focal, h / 2], [0, 0, 1]], np.float64)


def orbit(n, radius=3.0, focals=(60.0, 75.0), h=H, w=W, phase=0.3):
    ang = phase + 2 * np.pi * np.arange(n) / max(n, 1)
    c2w = [look_at((radius * np.cos(a), radius * np.sin(a), radius * 0.4 * (-1) ** i)) for i, a in enumerate(ang)]
    ixt = [intrinsics(focals[i % len(focals)] * h / H, h, w) for i in range(n)]
    return np.array(ixt, F32).reshape(-1, 3, 3), np.array(c2w, F32).reshape(-1, 4, 4)


def views():
    """(ixt [6,3,3], c2w [6,4,4]) fp32: four orbit views, one inside the sphere looking out (index 4), one whose border cuts the
    sphere (index 5)."""
    ixt, c2w = orbit(4)
    inside = look_at((0.1, 0.05, 0.0), (1.0, 0.3, 0.2))
    cut = look_at((0.0, -3.0, 0.5), (0.9, 0.0, 0.0))
    return (np.concatenate([ixt, intrinsics(40.0)[None].astype(F32), intrinsics(60.0)[None].astype(F32)]),
            np.concatenate([c2w, inside[None].astype(F32), cut[None].astype(F32)]))


def camera_arrays(ixt, c2w):
    """(k [V,4], w2c [V,16], eyes [V,3]) fp32: the arrays the bake takes."""
    ixt, c2w = np.asarray(ixt, np.float64).reshape(-1, 3, 3), np.asarray(c2w, np.float64).reshape(-1, 4, 4)
    k = np.stack([ixt[:, 0, 0], ixt[:, 1, 1], ixt[:, 0, 2], ixt[:, 1, 2]], 1).astype(F32)
    w2c = (np.linalg.inv(c2w) if len(c2w) else c2w).reshape(-1, 16).astype(F32)
    return k, w2c, np.ascontiguousarray(c2w[:, :3, 3]).astype(F32)


def pixel_rays(ixt, c2w, h, w):
    """Float64 (origins, directions) [h w, 3] of one camera through the pixel centres, view-space z = 1."""
    K, M = np.asarray(ixt, np.float64), np.asarray(c2w, np.float64)
    x, y = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5)
    a, b = (x.ravel() - K[0, 2]) / K[0, 0], (y.ravel() - K[1, 2]) / K[1, 1]
    d = a[:, None] * M[:3, 0] + b[:, None] * M[:3, 1] + M[:3, 2]
    return np.broadcast_to(M[:3, 3], d.shape).copy(), d


def cast(o, d, V, F, chunk=4096):
    """(face [R] int64 or -1, bary [R,3] float64, hit [R,3] float64) of the first hit with t > 0, float64 Moeller-Trumbore on every
    valid triangle whose bounding ball the ray's line meets."""
    V, F = np.asarray(V, F32).astype(np.float64), np.asarray(F, np.int64)
    ok = R.valid_triangles(V, F)
    Fs = np.where(ok[:, None], F, 0)
    p0, p1, p2 = V[Fs[:, 0]], V[Fs[:, 1]], V[Fs[:, 2]]
    c = (p0 + p1 + p2) / 3
    r2 = np.max([((p - c) ** 2).sum(1) for p in (p0, p1, p2)], 0) * (1 + 1e-6) + 1e-12
    face, bary, hit = np.full(len(o), -1, np.int64), np.full((len(o), 3), np.nan), np.full((len(o), 3), np.nan)
    for s in range(0, len(o), chunk):
        oo, dd = o[s:s + chunk], d[s:s + chunk]
        dn = dd / np.linalg.norm(dd, axis=1, keepdims=True)
        along = dn @ c.T - (dn * oo).sum(1)[:, None]
        dist2 = (c * c).sum(1)[None] - 2 * (oo @ c.T) + (oo * oo).sum(1)[:, None] - along * along
        ri, ti = np.nonzero((dist2 <= r2[None]) & ok[None])
        e1, e2, D, O = p1[ti] - p0[ti], p2[ti] - p0[ti], dd[ri], oo[ri]
        h = np.cross(D, e2)
        det = (e1 * h).sum(1)
        with np.errstate(all="ignore"):
            sv = O - p0[ti]
            u = (sv * h).sum(1) / det
            q = np.cross(sv, e1)
            v, t = (D * q).sum(1) / det, (e2 * q).sum(1) / det
        good = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)
        ri, ti, u, v, t = ri[good], ti[good], u[good], v[good], t[good]
        order = np.lexsort((ti, t, ri))
        ri, ti, u, v, t = ri[order], ti[order], u[order], v[order], t[order]
        first = np.ones(len(ri), bool)
        first[1:] = ri[1:] != ri[:-1]
        ri, ti, u, v = ri[first] + s, ti[first], u[first], v[first]
        face[ri], bary[ri] = ti, np.stack([1 - u - v, u, v], 1)
        hit[ri] = bary[ri, 0, None] * p0[ti] + bary[ri, 1, None] * p1[ti] + bary[ri, 2, None] * p2[ti]
    return face, bary, hit


def render(V, F, ixt, c2w, h, w, wave, background=0.25):
    """[V,h,w,3] fp32 images of the mesh coloured by ``field``."""
    out = np.full((len(ixt), h * w, 3), background, np.float64)
    for e in range(len(ixt)):
        o, d = pixel_rays(ixt[e], c2w[e], h, w)
        face, _, hit = cast(o, d, V, F)
        out[e, face >= 0] = field(hit[face >= 0], wave)
    return out.reshape(len(ixt), h, w, 3).astype(F32)


def source_images():
    """The six 48 x 64 views of the icosphere under the field of wave number 6."""
    if "images" not in _cache:
        V, F = R.icosphere(3)
        ixt, c2w = views()
        _cache["images"] = (ixt, c2w, render(V, F, ixt, c2w, H, W, 6.0))
        for a in _cache["images"]:
            a.setflags(write=False)
    return _cache["images"]


def two_layer():
    V, F = R.icosphere(3)
    return np.concatenate([V, (V * F32(0.5)).astype(F32)]), np.concatenate([F, F + len(V)])


def _odd():
    V, F = R.icosphere(3)
    return V, F[:11]


MESHES = {
    "icosphere": lambda: R.icosphere(3), "uv_sphere": lambda: C.case_uv_sphere()[1:], "degenerate": lambda: C.case_degenerate()[1:],
    "bad_triangles": lambda: C.case_bad_triangles()[1:], "one_triangle": lambda: C.case_one_triangle()[1:], "odd": _odd,
    "empty": lambda: (np.zeros((3, 3), F32), np.zeros((0, 3), np.int64)), "two_layer": two_layer,
}
# key: (mesh, S, C or None for the default, number of views or None for the six)
CASES = {
    "icosphere S8": ("icosphere", 8, None, None), "icosphere S3 C37": ("icosphere", 3, 37, None),
    "uv_sphere S4 C50": ("uv_sphere", 4, 50, None), "degenerate S7 C10": ("degenerate", 7, 10, None),
    "bad_triangles S4 C5": ("bad_triangles", 4, 5, None), "one_triangle S3 C1": ("one_triangle", 3, 1, None),
    "odd S7 C4": ("odd", 7, 4, None), "odd S8 C1": ("odd", 8, 1, None), "odd S4 V0": ("odd", 4, 4, 0), "odd S3 V64": ("odd", 3, 4, 64),
    "empty S4 C2": ("empty", 4, 2, None), "two_layer S3 C40": ("two_layer", 3, 40, None),
}
KEYS = tuple(CASES)
# bake settings every case is run under: (name, keyword arguments; "mask": a pseudo-random one on the CPU, visibility's on the GPU)
VARIANTS = (
    ("weighted", dict(blend="weighted")), ("best", dict(blend="best")),
    ("weighted masked colours", dict(blend="weighted", mask=True, colours=True)),
    ("best masked fill two-sided", dict(blend="best", mask=True, fill=(0.2, 0.5, 0.9), two_sided=True, power=3)),
    ("weighted power 0 loose", dict(blend="weighted", power=0, min_cos=-1.0, near=2.5, colours=True)),
)


def case(key):
    """{"V", "F", "layout", "ixt", "c2w", "images", "k", "w2c", "eyes", "colours" [Nv,3] fp32, "mask" [Ha,Wa] int64 pseudo-random}."""
    if key not in _cache:
        name, S, Cc, nv = CASES[key]
        V, F = MESHES[name]()
        V, F = np.asarray(V, F32), np.asarray(F, np.int64).reshape(-1, 3)
        layout = X.atlas(len(F), S, None if Cc is None else Cc * (S + 1))
        ixt, c2w, images = source_images()
        if nv is not None:
            pick = np.arange(nv) % len(ixt)
            ixt, c2w, images = ixt[pick], c2w[pick], images[pick]
        k, w2c, eyes = camera_arrays(ixt, c2w)
        g = np.random.default_rng(len(key) + 31 * S)
        with np.errstate(invalid="ignore"):
            colours = np.nan_to_num(field(V, 3.0)).astype(F32)
        out = {"V": V, "F": F, "ixt": ixt, "c2w": c2w, "images": images, "k": k, "w2c": w2c, "eyes": eyes, "colours": colours,
               "mask": g.integers(-2 ** 63, 2 ** 63 - 1, (layout[3], layout[2]), dtype=np.int64)}
        for a in out.values():
            a.setflags(write=False)
        out["layout"] = layout
        _cache[key] = out
    return _cache[key]


def bake_arguments(c, kw, mask=None):
    """The restatement's keyword arguments of a variant on case ``c``; ``mask``: the one to use where the variant asks for one."""
    kw = dict(kw)
    use_mask, use_colours = kw.pop("mask", False), kw.pop("colours", False)
    kw["mask"] = (c["mask"] if mask is None else mask) if use_mask else None
    kw["vertex_colors"] = c["colours"] if use_colours else None
    return kw


def restated(key, variant):
    """(texture, weight, view) of the restatement under the variant with the case's pseudo-random mask."""
    k = ("bake", key, variant)
    if k not in _cache:
        c = case(key)
        _cache[k] = X.bake(c["layout"], c["V"], c["F"], c["images"], c["k"], c["w2c"], c["eyes"], **bake_arguments(c, dict(VARIANTS)[variant]))
    return _cache[k]


def dense_bary(n=24):
    """Barycentrics of a triangle on a lattice of step 1 / n and at off-lattice points, corners and edges included: [m,3] fp32."""
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1))
    keep = i + j <= n
    b1, b2 = i[keep] / n, j[keep] / n
    g = np.random.default_rng(3)
    r = g.random((400, 2))
    r = np.where((r.sum(1) > 1)[:, None], 1 - r, r)
    b1, b2 = np.concatenate([b1, r[:, 0]]), np.concatenate([b2, r[:, 1]])
    return np.stack([1 - b1 - b2, b1, b2], 1).astype(F32)


# ---- the tooth ------------------------------------------------------------------------------------------------------------------------
TOOTH_WAVE, TOOTH_SOURCE, TOOTH_HELD_OUT, TOOTH_CAP, TOOTH_PERFECT = 20.0, 96, 64, 0.25, 0.059


def tooth():
    """The icosphere under the field of wave number 20: 8 orbit views of TOOTH_SOURCE^2 pixels to bake from, and one held-out view
    of TOOTH_HELD_OUT^2: its rays' faces and barycentrics (fp32), the analytic colour of their hit points, and the barycentric blend of
    the analytic vertex colours there."""
    if "tooth" not in _cache:
        V, F = R.icosphere(3)
        n = TOOTH_SOURCE
        ixt, c2w = orbit(8, focals=(1.25 * n, 1.4 * n), h=H, w=W)
        ixt = ixt.copy()
        ixt[:, 0, 2] = ixt[:, 1, 2] = n / 2
        images = render(V, F, ixt, c2w, n, n, TOOTH_WAVE)
        m = TOOTH_HELD_OUT
        held_ixt = np.array([[1.3 * m, 0, m / 2], [0, 1.3 * m, m / 2], [0, 0, 1]], F32)
        held_c2w = look_at((1.9, -1.7, 1.5)).astype(F32)
        o, d = pixel_rays(held_ixt, held_c2w, m, m)
        face, bary, hit = cast(o, d, V, F)
        hits = face >= 0
        vc = field(V, TOOTH_WAVE)
        blend = (bary[hits, :, None] * vc[F[face[hits]]]).sum(1)
        _cache["tooth"] = {"V": V, "F": F, "ixt": ixt, "c2w": c2w, "images": images, "held_ixt": held_ixt, "held_c2w": held_c2w,
                           "face": face[hits].astype(np.int32), "bary": bary[hits].astype(F32), "truth": field(hit[hits], TOOTH_WAVE),
                           "vertex_blend": blend, "vertex_colors": vc.astype(F32), "hits": hits, "res": (n, m)}
    return _cache["tooth"]


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))
