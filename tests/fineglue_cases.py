"""The cases tests/test_fineglue_f64.py (CPU) and tests/test_fineglue_f64_gpu.py (MI355X) hold the point sampler, the surface maps
and the activations to, with the conditions each case must meet (`*_self_check`, from the reference alone) and the comparison
both files apply (`worst`: |got - ref| / (4 A + 2^-23 |ref|), element by element, oracle/fineglue_f64.py).

Everything is float32 numpy, generated from fixed seeds; nothing here touches a device.
"""
import functools

import numpy as np
import torch

from oracle import fineglue_f64 as fg

F32 = np.float32
MAP_KEYS = ("image", "depth", "acc_map", "rend_normal", "depth_normal", "rend_dist")      # the kernels' order of the six maps
GRAD_KEYS = ("d_image", "d_acc_map", "d_depth")


def worst(got, ref, keys):
    """{key: largest |got - ref| / limit}; `ref[key]` a B object or, for an exact copy, a plain array (then: equal bits)"""
    out = {}
    for k in keys:
        r = ref[k] if isinstance(ref[k], fg.B) else fg.B(ref[k])
        assert np.asarray(got[k]).shape == r.shape, (k, np.asarray(got[k]).shape, r.shape)
        out[k] = float(fg.ratio(got[k], r).max()) if r.v.size else 0.0
    return out


def as_f32(x):
    """a reference value as the fp32 array an exact evaluation gives"""
    with np.errstate(over="ignore", invalid="ignore"):
        return fg.val(x).astype(F32)


def same_bits(a, b):
    """equal bits (the sign of a zero included); two NaNs count as equal"""
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def pattern_for(t, salt=0):
    """a dyadic non-zero fill for the three gradient maps the backward accumulates into"""
    out = {}
    for j, (k, src) in enumerate((("d_image", "image"), ("d_acc_map", "acc_map"), ("d_depth", "depth"))):
        i = np.arange(t[src].size, dtype=np.int64).reshape(t[src].shape)
        out[k] = ((1 + (i + j + salt) % 7) * 0.5).astype(F32)
    return out


# ---------------------------------------------------------------------------------------------- exact-arithmetic sampler cases

EX_H, EX_W, EX_V = 10, 12, 3
EX_CLUSTER = 2000


def _axis_positions(size):
    return [-1.25, -1.0, -0.5, 0.0, 0.25, size - 1.25, size - 1.0, size - 0.5, float(size), size + 1.0, size + 2.0, 3.0 * 2 ** 20]


@functools.lru_cache(maxsize=None)
def exact_inputs(variant="edges"):
    """Signed-permutation cameras that share the depth axis (q.z = p.z in {+-0.5, +-1, +-2}: every division is by a power of two),
    dyadic translations, power-of-two focals, dyadic principal points, points on a 2^-6 lattice chosen so that view 0 samples
    every combination of the edge positions; 2000 points on one position; four points at the +-2^31 scale.  Dyadic maps and small-
    integer g_out: every sum is exact below 2^24.  variant "kink": q.z = 1 everywhere, the depth map constant 1 (= z: the kink of
    | s - z |), gradient on channel 7 alone."""
    h, w, V = EX_H, EX_W, EX_V
    rng = np.random.default_rng(7)
    w2c = np.zeros((V, 4, 4), F32)
    w2c[:, 3, 3] = w2c[:, 2, 2] = 1
    w2c[0, 0, 0], w2c[0, 1, 1], w2c[0, :2, 3] = 1, 1, (0.25, -0.5)
    w2c[1, 0, 1], w2c[1, 1, 0], w2c[1, :2, 3] = -1, 1, (0.5, 0.75)
    w2c[2, 0, 0], w2c[2, 1, 1], w2c[2, :2, 3] = -1, -1, (0.0, 0.5)
    ixt = np.zeros((V, 3, 3), F32)
    ixt[:, 2, 2] = 1
    for v, (f, px, py) in enumerate(((8, 6, 5), (16, 4, 3.5), (4, 6.25, 4.75))):
        ixt[v, 0, 0] = ixt[v, 1, 1] = f
        ixt[v, 0, 2], ixt[v, 1, 2] = px, py
    zs = [0.5, -0.5, 1.0, -1.0, 2.0, -2.0]
    pos, k = [], 0
    for X in _axis_positions(w):
        for Y in _axis_positions(h):
            pos.append((X, Y, 1.0 if variant == "kink" else zs[k % 6]))
            k += 1
    pos += [(3.0, 4.0, 1.0), (7.0, 2.0, 1.0 if variant == "kink" else -2.0)]          # interior integer positions: wx = wy = 0
    n_edge = len(pos)
    pos += [(2.25, 3.5, 1.0)] * EX_CLUSTER                                            # one pixel receives 2000 atomics per channel
    pos = np.array(pos, dtype=np.float64)
    cz = pos[:, 2]
    cx, cy = (pos[:, 0] - 6) * cz / 8, (pos[:, 1] - 5) * cz / 8                      # view 0: x = 8 cx / cz + 6, y = 8 cy / cz + 5
    pts = np.stack([cx - 0.25, cy + 0.5, cz], 1)
    far = np.array([[2.0 ** 28, 0.5, 1], [-2.0 ** 28, 0.5, 1], [0.5, 2.0 ** 28, -1], [0.25, -2.0 ** 28, 1]])   # +-2^31-scale positions
    pts = np.concatenate([pts, far]).astype(F32)
    n = len(pts)
    dy = lambda *s: (rng.integers(-4, 5, size=s) / 4).astype(F32)
    t = {"points": pts, "w2c": w2c, "ixt": ixt, "img_ref": dy(V, 3, h, w), "image": dy(V, h, w, 3), "acc_map": dy(V, h, w),
         "depth": (rng.integers(0, 13, size=(V, h, w, 1)) / 4).astype(F32), "g_out": rng.integers(-2, 3, size=(V, 8, n)).astype(F32)}
    if variant == "kink":
        t["depth"] = np.ones((V, h, w, 1), F32)
        t["g_out"][:, :7] = 0
        t["g_out"][:, 7] = rng.integers(1, 3, size=(V, n))
    t["n_edge"], t["n_lattice"], t["variant"] = n_edge, n - 4, variant
    return t


def exact_self_check(t):
    """the conditions of the exact cases, from the two evaluations of the reference alone"""
    h, w = EX_H, EX_W
    a, b = fg.project(t, "f32"), fg.project(t, "f64")
    lat = slice(0, t["n_lattice"])
    for p32, p64 in zip(a, b):
        assert same_bits(p32[:, lat], p64.v[:, lat].astype(F32)) and np.array_equal(p32[:, lat].astype(np.float64), p64.v[:, lat]), \
            "an fp32 and an fp64 evaluation of the projection differ on the lattice points"
    x0, y0 = b[0].v[0], b[1].v[0]
    have = set(zip(x0[:t["n_edge"]].tolist(), y0[:t["n_edge"]].tolist()))
    for X in _axis_positions(w):
        for Y in _axis_positions(h):
            assert (X, Y) in have, f"view 0 does not sample ({X}, {Y})"
    for corner in ((0.0, 0.0), (w - 1.0, 0.0), (0.0, h - 1.0), (w - 1.0, h - 1.0), (-1.0, -1.0), (float(w), float(h))):
        assert corner in have
    assert (3.0, 4.0) in have and (t["variant"] == "kink" or (b[2].v[:, :t["n_edge"]] < 0).any())
    far = slice(t["n_lattice"], None)          # the +-2^31-scale points: far outside in every view, in both evaluations
    for px, py in ((a[0], a[1]), (b[0].v, b[1].v)):
        size = np.maximum(np.abs(px[:, far]), np.abs(py[:, far]))
        assert (size > 2.0 ** 20).all() and (size.max(axis=0) >= 2.0 ** 30).all()
    assert (b[0].v[0, t["n_edge"]:t["n_lattice"]] == 2.25).all() and (b[1].v[0, t["n_edge"]:t["n_lattice"]] == 3.5).all()


def exact_reference(t, pattern):
    """fp32 arrays every exact evaluation must reproduce bit for bit: the fp64 reference, which the fp32 evaluation equals"""
    r64 = fg.point_feats(t, "f64", pattern=pattern)
    r32 = fg.point_feats(t, "f32", pattern=pattern)
    out = {}
    for k in ("out", "d_points") + GRAD_KEYS:
        out[k] = as_f32(r64[k])
        assert np.array_equal(out[k].astype(np.float64), r64[k].v, equal_nan=True), f"{k}: the reference is not representable in fp32"
        assert same_bits(out[k], r32[k]), f"{k}: the fp32 evaluation rounds somewhere: the case is not exact"
    out["resid"] = r64["resid"].v
    return out


# ---------------------------------------------------------------------------------------------- general-position sampler cases

GEN_H, GEN_W = 20, 28
FRAC_LO, FRAC_HI, RESID_MIN = 1.0 / 16, 15.0 / 16, 0.25


def _smooth(rng, lead, h, w):
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    ph = rng.random(lead + (3, 1, 1)) * 6.28
    fr = rng.random(lead + (3, 1, 1)) * 5 + 1
    return 0.5 + 0.15 * (np.sin(fr[..., 0, :, :] * xx + ph[..., 0, :, :]) + np.sin(fr[..., 1, :, :] * yy + ph[..., 1, :, :])
                         + np.sin(fr[..., 2, :, :] * (xx + yy) + ph[..., 2, :, :]))


def _margins(t, r):
    """per (view, point): is the position far outside (no tap inside, by half a pixel), are the fractional parts inside
    [1/16, 15/16], is | s_7 - z | >= 0.25"""
    h, w = t["img_ref"].shape[2:]
    x, y = r["x"].v, r["y"].v
    with np.errstate(invalid="ignore"):
        far = (x <= -1.5) | (x >= w + 0.5) | (y <= -1.5) | (y >= h + 0.5)
        fx, fy = x - np.floor(x), y - np.floor(y)
        frac = (fx >= FRAC_LO) & (fx <= FRAC_HI) & (fy >= FRAC_LO) & (fy <= FRAC_HI)
        resid = np.abs(r["resid"].v) >= RESID_MIN
        small = (4 * r["x"].A <= 1.0 / 64) & (4 * r["y"].A <= 1.0 / 64) & (4 * r["resid"].A <= 1.0 / 64)
    return far, frac, resid, small


@functools.lru_cache(maxsize=None)
def general_inputs(V, n, seed=0, noise=False, cams="turntable"):
    """Cameras from cameras.turntable_c2w; points back-projected in fp64 from chosen pixel positions (fractional parts in
    [1/16, 15/16], some outside every frustum) and depths, rounded to fp32, and kept when they meet the kink margins in EVERY
    view -- a condition on the inputs, evaluated by the reference alone.  cams = "mixed": view 1 is an axis-aligned camera at
    distance 2 (the non-finite cases put a point exactly on its plane)."""
    from lara_amd import cameras
    h, w = GEN_H, GEN_W
    rng = np.random.default_rng(1000 * V + n + 77 * seed)
    c2w = cameras.turntable_c2w(8)[:V].double()
    w2c = torch.linalg.inv(c2w).numpy()
    if cams == "mixed":
        w2c[1] = np.eye(4)
        w2c[1, 2, 3] = 2.0
    w2c = w2c.astype(F32)
    ixt = np.tile(np.array([[30.0, 0, w / 2], [0, 30.0, h / 2], [0, 0, 1.0]], F32), (V, 1, 1))
    maps = (lambda lead: rng.random(lead + (h, w))) if noise else (lambda lead: _smooth(rng, lead, h, w))
    t = {"w2c": w2c, "ixt": ixt, "img_ref": maps((V, 3)).astype(F32), "image": maps((V, 3)).transpose(0, 2, 3, 1).astype(F32).copy(),
         "acc_map": maps((V,)).astype(F32), "depth": (3.0 + maps((V,)))[..., None].astype(F32)}
    m = max(60 * n, 4000)
    v = rng.integers(0, V, size=m)
    outside = rng.random(m) < 0.15
    X = np.where(outside, rng.choice([-1, 1], m) * rng.uniform(60, 900, m), rng.integers(-3, w + 3, m) + rng.uniform(FRAC_LO, FRAC_HI, m))
    Y = np.where(outside & (rng.random(m) < 0.5), rng.choice([-1, 1], m) * rng.uniform(60, 900, m), rng.integers(-3, h + 3, m) + rng.uniform(FRAC_LO, FRAC_HI, m))
    zc = rng.uniform(1.2, 2.6, m)
    K64, W64 = ixt.astype(np.float64), w2c.astype(np.float64)
    c = zc[:, None] * np.einsum("mij,mj->mi", np.linalg.inv(K64)[v], np.stack([X, Y, np.ones(m)], 1))
    pts = np.einsum("mji,mj->mi", W64[v, :3, :3], c - W64[v, :3, 3]).astype(F32)
    cand = dict(t, points=pts)
    far, frac, resid, small = _margins(cand, fg.point_feats(cand, "f64"))
    keep = np.flatnonzero(((far | (frac & small)) & resid).all(axis=0))
    assert len(keep) >= n, (V, n, len(keep))
    t["points"] = pts[keep[:n]]
    t["g_out"] = rng.standard_normal((V, 8, n)).astype(F32)
    return t


def general_self_check(t, r):
    """both margins, for every (view, point) pair: none is excluded"""
    far, frac, resid, small = _margins(t, r)
    assert (far | (frac & small)).all() and resid.all()
    return {"pairs": int(far.size), "outside": int(far.sum())}


LANE_CASES = [(V, n) for V in range(1, 9) for n in (1, 63, 64, 65, 333)]
GENERAL_CASES = [("smooth", 4, 1500), ("noise", 4, 1500), ("smooth", 3, 4096)]


def general_case(kind, V, n):
    return general_inputs(V, n, seed=1, noise=kind == "noise")


def nonfinite_inputs():
    """V = 3 ("mixed" cameras), n = 65: point 5 lies exactly on the plane of camera 1 (q.z = -2 + 2 = 0, fused or not), point 9
    has a NaN coordinate.  -> (inputs, bad point indices)"""
    t = dict(general_inputs(3, 65, seed=2, cams="mixed"))
    pts = t["points"].copy()
    pts[5] = (0.3, 0.2, -2.0)
    pts[9, 0] = np.nan
    t["points"] = pts
    return t, [5, 9]


def to_side_by_side(t, R, fill=np.nan):
    """the three render-derived maps of a [V, h, w, c] case as [h, R*w, c] maps whose views >= V hold `fill`"""
    V, h, w = t["acc_map"].shape
    out = {}
    for k in ("image", "acc_map", "depth"):
        x = t[k].reshape(V, h, w, -1)
        wide = np.full((h, R, w, x.shape[-1]), fill, F32)
        wide[:, :V] = x.transpose(1, 0, 2, 3)
        out[k] = wide.reshape((h, R * w) + ((x.shape[-1],) if k != "acc_map" else ()))
    return out


def from_side_by_side(x, V, R):
    """[h, R*w, (c)] -> the first V views as [V, h, w, (c)] and the rest as [h, R - V, w, (c)]"""
    h = x.shape[0]
    w = x.shape[1] // R
    y = x.reshape((h, R, w) + x.shape[2:])
    return np.ascontiguousarray(np.moveaxis(y[:, :V], 1, 0)), y[:, V:]


# ---------------------------------------------------------------------------------------------- rows

def voxel_rows_case(width):
    """ascending voxel indices over 40 voxels: runs that start at row 0 and end at row n - 1, voxels without a row, and one run of
    1000 rows on the last voxel"""
    rng = np.random.default_rng(width)
    n_vox = 40
    vox = np.sort(np.concatenate([[0, 0, 0], rng.integers(0, n_vox - 1, 300), np.full(1000, n_vox - 1)])).astype(np.int64)
    vox = vox[(vox != 7) & (vox != 20)]
    return {"n_vox": n_vox, "vox": vox, "src": rng.standard_normal((n_vox, width)).astype(F32),
            "g": rng.standard_normal((len(vox), width)).astype(F32)}


TAKE_WIDTHS = (1, 2, 3, 4, 12, 1, 2, 4)


# ---------------------------------------------------------------------------------------------- surface maps

SURFACE_SIZES = ((3, 3), (3, 300), (17, 16), (33, 31))
SURFACE_CASES = [(H, W, n, ratio) for H, W in SURFACE_SIZES for n in (1, 3) for ratio in (0.0, 0.25, 1.0)]
SPECIAL_SIZES = ((17, 16), (33, 31))
SINE_MIN = 1e-3
SLOTS = [(y, x) for y in (2, 6, 10, 14) for x in (2, 6, 10, 14)]
SPECIALS = ("alpha_zero", "alpha_minus_zero", "c0_nan", "md_nan", "md_pinf", "md_ninf", "flat_patch", "collinear_patch")
COLOURS = (0.0, 1.0, -2.0 ** -149, 1.0 + 2.0 ** -23)


@functools.lru_cache(maxsize=None)
def surface_inputs(H, W, n, special=False):
    """Ordinary pixels: alpha in [1e-3, 1], a smooth depth field seen through pinhole rays (|a x b| >= 1e-3 |a| |b|), colours in
    [-0.2, 1.2].  special: the pixels of SPECIALS on SLOTS (view 0 and the last view), the four colours of COLOURS in row 0."""
    rng = np.random.default_rng(H * 1000 + W * 10 + n)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    f = 1.5 * max(H, W)
    d = np.stack([(xx - W / 2) / f, (yy - H / 2) / f, np.ones_like(xx)], -1)
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    rays = np.zeros((n, H, W, 6))
    rays[..., :3] = rng.uniform(-0.3, 0.3, (n, 1, 1, 3))
    rays[..., 3:] = d
    E = 2.0 + _smooth(rng, (n,), H, W)
    alpha = np.exp(rng.uniform(np.log(1e-3), 0.0, (n, H, W)))
    allmap = rng.standard_normal((n, 7, H, W))
    allmap[:, 1], allmap[:, 0], allmap[:, 5] = alpha, E * alpha, 2.0 + _smooth(rng, (n,), H, W)
    color = rng.random((n, 3, H, W)) * 1.4 - 0.2
    rots = np.stack([np.linalg.qr(rng.standard_normal((3, 3)))[0] for _ in range(n)]).reshape(n, 9)
    t = {"color": color.astype(F32), "allmap": allmap.astype(F32), "rays": rays.astype(F32), "rots": rots.astype(F32)}
    t["where"] = {}
    if special:
        for v in sorted({0, n - 1}):
            for name, (y, x) in zip(SPECIALS, SLOTS[v:] + SLOTS[:v]):
                a, r = t["allmap"][v], t["rays"][v]
                if name == "alpha_zero":
                    a[1, y, x], a[0, y, x] = 0.0, 0.5
                elif name == "alpha_minus_zero":
                    a[1, y, x], a[0, y, x] = -0.0, 0.5
                elif name == "c0_nan":
                    a[0, y, x] = np.nan
                elif name in ("md_nan", "md_pinf", "md_ninf"):
                    a[5, y, x] = {"md_nan": np.nan, "md_pinf": np.inf, "md_ninf": -np.inf}[name]
                else:
                    box = np.s_[y - 1:y + 2, x - 1:x + 2]
                    a[(0,) + box], a[(1,) + box], a[(5,) + box] = 1.25, 0.5, 2.5
                    r[box] = (0, 0, 0, 0, 0, 1) if name == "flat_patch" else (0, 0, 0, 1, 0, 0)
                    if name == "collinear_patch":      # parallel rays from collinear origins: a = (0, 0, 1/4) || b = (0, 0, 1/2)
                        r[box + (2,)] = (yy[box] + 2 * xx[box]) / 8
                t["where"][(v, name)] = (y, x)
            for c, (x, value) in enumerate(zip((0, 1, 2, 3), COLOURS)):
                t["color"][v, c % 3, 0, x] = F32(value)
    return t


def surface_grads(t, which, seed=0, scale=1.0):
    """gradients of the six outputs ([H, n*W, C]); which: "all" or one of MAP_KEYS (the others None)"""
    n, _, H, W = t["color"].shape
    rng = np.random.default_rng(seed + H + W)
    shapes = {"image": (H, n * W, 3), "depth": (H, n * W, 1), "acc_map": (H, n * W), "rend_normal": (H, n * W, 3),
              "depth_normal": (H, n * W, 3), "rend_dist": (H, n * W)}
    g = {k: (scale * rng.standard_normal(shapes[k])).astype(F32) for k in MAP_KEYS}
    return {k: (g[k] if which in ("all", k) else None) for k in MAP_KEYS}


def surface_self_check(t, r, special):
    n, _, H, W = t["color"].shape
    a = t["allmap"]
    if not special:
        assert (a[:, 1] >= 1e-3 * (1 - 1e-6)).all() and (a[:, 1] <= 1).all() and np.isfinite(a).all()
        if H > 2 and W > 2:
            assert (r["sine"] >= SINE_MIN).all(), float(r["sine"].min())
        return
    w = t["where"]
    for v in sorted({0, n - 1}):
        y, x = w[(v, "alpha_zero")]
        assert a[v, 1, y, x] == 0 and not np.signbit(a[v, 1, y, x])
        y, x = w[(v, "alpha_minus_zero")]
        assert a[v, 1, y, x] == 0 and np.signbit(a[v, 1, y, x])
        assert np.isnan(a[v, 0][w[(v, "c0_nan")]]) and np.isnan(a[v, 5][w[(v, "md_nan")]])
        assert a[v, 5][w[(v, "md_pinf")]] == np.inf and a[v, 5][w[(v, "md_ninf")]] == -np.inf
        for name in ("flat_patch", "collinear_patch"):       # the cross product at the patch centre is exactly 0, with bound 0
            y, x = w[(v, name)]
            dn = r["depth_normal"]
            assert (dn.v[y, v * W + x] == 0).all() and (dn.A[y, v * W + x] == 0).all() and r["len"][v, y - 1, x - 1] == 0
        cs = [t["color"][v, c % 3, 0, x] for c, x in enumerate((0, 1, 2, 3))]
        assert cs[0] == 0 and cs[1] == 1 and cs[2] < 0 and cs[3] > 1
    pts = [p for (v, _), p in w.items() if v == 0]
    assert all(max(abs(p[0] - q[0]), abs(p[1] - q[1])) >= 3 for i, p in enumerate(pts) for q in pts[:i])


# ---------------------------------------------------------------------------------------------- activations

ACT_P = (1, 255, 257)
OPACITIES = (0.0, -0.0, 20.0, -20.0, 88.0, -88.0, 104.0, -104.0)
SCALES = (-104.0, -87.0, 0.0, 88.0)


def _quaternions():
    e = np.float64(F32(1e-12))
    half = np.full(4, 0.5)
    return [np.zeros(4), 1e-13 * np.array([0.6, 0.0, -0.8, 0.0]), e * (1 + 2.0 ** -20) * half, e * (1 - 2.0 ** -20) * half,
            np.array([0, 0, 3.0, 0]), np.array([-0.25, 0, 0, 0]), np.array([1e18, -1e18, 1e18, 1e18]) * 0.999, np.array([0, 9.9e17, 0, -9.9e17])]


@functools.lru_cache(maxsize=None)
def activation_inputs(P, shift=0):
    """Domain: |q| < 1e18 per component (the squared norm stays finite in fp32).  The named values cycle through the rows
    (`shift` rotates them, so that P = 1 meets each), the rest is random."""
    rng = np.random.default_rng(P)
    o, s, q = rng.standard_normal(P) * 3, rng.standard_normal((P, 2)) - 4, rng.standard_normal((P, 4))
    qs = _quaternions()
    for i in range(min(P, 64)):
        o[i] = OPACITIES[(i + shift) % 8]
        s[i] = (SCALES[(i + shift) % 4], SCALES[(i // 4 + shift) % 4])
        q[i] = qs[(i + shift) % 8]
    t = {"opacity": o.astype(F32), "scales": s.astype(F32), "rotations": q.astype(F32)}
    t["g_opacity"], t["g_scales"], t["g_rotations"] = (rng.standard_normal(x.shape).astype(F32) for x in (o, s, q))
    return t


def activation_self_check(t):
    q = t["rotations"].astype(np.float64)
    assert (np.abs(q) < 1e18).all()
    ln = np.sqrt((q * q).sum(1))
    rel = np.abs(ln / np.float64(fg.EPS12) - 1)
    assert (rel >= 2.0 ** -21).all(), "a quaternion's length is within fp32 rounding of the 1e-12 threshold"
    return ln
