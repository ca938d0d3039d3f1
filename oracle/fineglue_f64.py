"""fp64 reference of the fp32 kernels between the learned blocks of the fine pass -- TEST INFRASTRUCTURE ONLY (the checker of
tests/test_fineglue_f64.py and tests/test_fineglue_f64_gpu.py; nothing under lara_amd/ imports it):

    include/lara_pointfeat.h   projection, bilinear gather of the 8-channel stack, depth residual, their backward (coordinate
                               gradient summed over the views, atomic scatter into the three map gradients), voxel_rows, take_rows
    include/lara_surface.h     the six surface maps, their backward (depth normals with the 4-neighbour VJP), the three activations

The formulas are written ONCE, from the two headers, over a number type: `mode="f64"` evaluates them on `B` objects -- an fp64
value and, beside it, the fp32 error bound A of that element from the reference's own operands -- and `mode="f32"` on plain
float32 numpy arrays, which is the "straightforward fp32 evaluation" tests/test_fineglue_f64.py holds to the same checks the
device gets (numpy does not contract a * b + c into an FMA; every bound below is a bound on |rounded - exact| per operation, and
a fused operation rounds once where the unfused one rounds twice, so the bounds cover both forms).  Pixel positions are the
header's: pixel i is centred at i, the sample position is (x, y) itself; no grid_sample round trip.

Bounds, first order (the acceptance test's factor 4 absorbs the rest):
    one operation                 2^-24 |result| (+ 2^-150 for a denormal result); nothing when the operands are exact and the
                                  result is representable in fp32
    a sum of K terms              K 2^-24 sum|terms| + the terms' own bounds (any order); nothing when at most one term is non-zero
    an atomic sum of N terms      N 2^-24 sum|terms| + the terms' own bounds: holds for any order of the atomics
    expf                          one ulp, 2^-23 |result| (ROCm's documented bound), plus 2^-149 for a denormal result
    through f(a, b, ..)           |df/da| A_a + ...   (a factor that is exactly 0 passes nothing on, whatever the other's bound)
fp32 is emulated where the result depends on it: every result beyond FLT_MAX becomes +-inf as it does on the device (so that
nan_to_num(-inf) = -FLT_MAX and what follows it overflow, or not, as the kernel's do), the nan_to_num classes are taken from the
fp32 quotient, and the 1e-12 clamps compare the fp32 length.

The acceptance test, element by element: |got - ref| <= 4 A + 2^-23 |ref|  (`ratio`); A = 0 and ref = 0: exactly 0; where the
reference is inf or NaN the class must agree.

`defect=` evaluates a WRONG version (the list DEFECTS); tests/test_fineglue_f64.py shows that each is caught by some case.
"""
import numpy as np

U = 2.0 ** -24
F32_MAX = float(np.finfo(np.float32).max)
EPS12 = np.float32(1e-12)          # F.normalize's eps as the kernels hold it
BIG12 = np.float32(1e12)           # ... and the clamped branch's factor
DEFECTS = ("tap_clamped_to_border", "weights_swapped_at_minus_one", "last_view_dropped", "sign_of_zero_is_one",
           "scatter_overwrites", "unpack_assigns", "stencil_crosses_views", "vjp_sign_flipped", "neg_inf_to_zero",
           "clamp_excludes_bounds", "rot_transposed", "clamped_quaternion_zero")


# ---------------------------------------------------------------------------------------------- values with bounds

def _representable(v):
    with np.errstate(over="ignore", invalid="ignore"):
        return v.astype(np.float32).astype(np.float64) == v


def _overflow(v):
    """a result beyond FLT_MAX (by more than half an ulp) is inf in fp32"""
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(v) > F32_MAX * (1 + 2.0 ** -25), np.sign(v) * np.inf, v)


def _p(x, A):
    """|x| A, with an exact zero factor passing nothing on (0 * inf = 0 here)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where((x == 0) | (A == 0), 0.0, np.abs(x) * A)


def _clean(A):
    return np.where(np.isnan(A), np.inf, A)


class B:
    """fp64 value `v` and fp32 error bound `A`, element by element"""
    __slots__ = ("v", "A")
    __array_ufunc__ = None

    def __init__(self, v, A=None):
        self.v = np.asarray(v, dtype=np.float64)
        self.A = np.zeros_like(self.v) if A is None else np.broadcast_to(np.asarray(A, dtype=np.float64), self.v.shape)

    @staticmethod
    def of(x):
        return x if isinstance(x, B) else B(x)

    def _done(self, v, A, exact_in):
        with np.errstate(invalid="ignore", over="ignore"):
            v = _overflow(v)
            A = A + np.where(exact_in & _representable(v), 0.0, U * np.abs(v) + np.where((v != 0) & (np.abs(v) < 2.0 ** -126), 2.0 ** -150, 0.0))
        return B(v, _clean(np.where(np.isfinite(v), A, 0.0)))

    def __add__(self, o):
        o = B.of(o)
        with np.errstate(invalid="ignore"):
            return self._done(self.v + o.v, self.A + o.A, (self.A == 0) & (o.A == 0))
    __radd__ = __add__

    def __neg__(self):
        return B(-self.v, self.A)

    def __sub__(self, o):
        return self + (-B.of(o))

    def __rsub__(self, o):
        return B.of(o) + (-self)

    def __mul__(self, o):
        o = B.of(o)
        with np.errstate(invalid="ignore", over="ignore"):
            return self._done(self.v * o.v, _p(self.v, o.A) + _p(o.v, self.A), (self.A == 0) & (o.A == 0))
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = B.of(o)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            v = self.v / o.v
            A = np.where(np.isinf(o.v), 0.0, (self.A + _p(v, o.A)) / np.abs(o.v))
            return self._done(v, A, (self.A == 0) & (o.A == 0))

    def __rtruediv__(self, o):
        return B.of(o) / self

    def __getitem__(self, k):
        return B(self.v[k], self.A[k])

    @property
    def shape(self):
        return self.v.shape


def lift(x, mode):
    """an exact fp32 operand in the evaluation's number type"""
    return B(np.asarray(x, dtype=np.float64)) if mode == "f64" else np.asarray(x, dtype=np.float32)


def val(x):
    return x.v if isinstance(x, B) else x


def fsum(terms):
    """a sum of K terms in any order"""
    if not isinstance(terms[0], B):
        out = terms[0]
        for t in terms[1:]:
            out = out + t
        return out
    with np.errstate(invalid="ignore", over="ignore"):
        v = _overflow(sum(t.v for t in terms))
        mag = sum(np.abs(t.v) for t in terms)
        nz = sum((t.v != 0).astype(np.int64) for t in terms)
        A = sum(t.A for t in terms) + np.where(nz > 1, len(terms) * U * mag, 0.0)
    return B(v, _clean(np.where(np.isfinite(v), A, 0.0)))


def fsqrt(x):
    if not isinstance(x, B):
        return np.sqrt(x)
    with np.errstate(invalid="ignore", divide="ignore"):
        v = np.sqrt(x.v)
        A = np.where((x.A == 0) | np.isinf(v), 0.0, x.A / (2 * v))
        return x._done(v, A, x.A == 0)


def fabs(x):
    return B(np.abs(x.v), x.A) if isinstance(x, B) else np.abs(x)


def fwhere(c, a, b):
    if isinstance(a, B) or isinstance(b, B):
        a, b = B.of(a), B.of(b)
        return B(np.where(c, a.v, b.v), np.where(c, a.A, b.A))
    return np.where(c, a, b)


def fexp(x):
    """expf: one ulp of the result (and 2^-149 where the result is denormal), besides the argument's own bound"""
    if not isinstance(x, B):
        return np.exp(x)
    with np.errstate(over="ignore"):
        v = _overflow(np.exp(x.v))
    return B(v, np.where(np.isfinite(v), v * x.A + 2 * U * v + 2.0 ** -149, 0.0))


def fstack(xs, axis=-1):
    if isinstance(xs[0], B):
        return B(np.stack([x.v for x in xs], axis), np.stack([x.A for x in xs], axis))
    return np.stack(xs, axis)


def f32_of(x):
    """the value as the device would hold it, for the decisions that compare an fp32 number"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(val(x)).astype(np.float32)


def limit(ref, A):
    return 4 * A + 2.0 ** -23 * np.abs(ref)


def ratio(got, ref):
    """|got - ref| / (4 A + 2^-23 |ref|) per element of the B object `ref`.  A = 0 and ref = 0: got must be 0 (else inf).
    Where ref is NaN or +-inf, got must be of the same class (0, else inf)."""
    got = np.asarray(got, dtype=np.float64)
    r, A = ref.v, ref.A
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        # (what the device holds of a finite reference beyond half an ulp of FLT_MAX is inf: `_overflow` made it so already)
        d = np.abs(got - r)
        lim = limit(r, A)
        out = np.where(lim > 0, d / lim, np.where(d > 0, np.inf, 0.0))
        out = np.where(np.isfinite(got), out, np.inf)
        same = np.where(np.isnan(r), np.isnan(got), got == r)
        out = np.where(np.isfinite(r), out, np.where(same, 0.0, np.inf))
    return np.where(np.isnan(out), np.inf, out)


# ---------------------------------------------------------------------------------------------- the point sampler

def pack_stack(t):
    """[V, h, w, 8] = [input image (3) | coarse render (3) | acc_map | depth], channel-last"""
    return np.concatenate([np.transpose(t["img_ref"], (0, 2, 3, 1)), t["image"], t["acc_map"][..., None], t["depth"]], axis=-1).astype(np.float32)


def _project(t, mode):
    """-> x, y, z of every (view, point), each [V, n]"""
    p = [lift(t["points"][None, :, k], mode) for k in range(3)]
    m = lambda r, c: lift(t["w2c"][:, r, c][:, None], mode)
    k = lambda r, c: lift(t["ixt"][:, r, c][:, None], mode)
    c = [fsum([m(r, 0) * p[0], m(r, 1) * p[1], m(r, 2) * p[2], m(r, 3)]) for r in range(3)]
    q = [fsum([k(r, 0) * c[0], k(r, 1) * c[1], k(r, 2) * c[2]]) for r in range(3)]
    with np.errstate(divide="ignore", invalid="ignore"):
        return q[0] / q[2], q[1] / q[2], q[2]


def project(t, mode="f64"):
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        return _project(t, mode)


def _taps(x, y, h, w, mode, defect):
    """the header's taps: (y0 + dy, x0 + dx) with weight (wx | 1 - wx)(wy | 1 - wy); a tap outside the image contributes zero;
    a position far outside, inf or nan has no tap inside"""
    fx, fy = np.floor(val(x)), np.floor(val(y))
    with np.errstate(invalid="ignore"):
        okx, oky = (fx >= -2) & (fx <= w + 1), (fy >= -2) & (fy <= h + 1)
    x0 = np.where(okx, fx, -2).astype(np.int64)
    y0 = np.where(oky, fy, -2).astype(np.int64)
    wx, wy = x - lift(fx, mode), y - lift(fy, mode)
    ax = [1.0 - wx, wx]
    ay = [1.0 - wy, wy]
    if defect == "weights_swapped_at_minus_one":
        ax = [fwhere(x0 == -1, ax[1], ax[0]), fwhere(x0 == -1, ax[0], ax[1])]
    tap = []
    for k in range(4):
        xi, yi = x0 + (k & 1), y0 + (k >> 1)
        inside = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
        if defect == "tap_clamped_to_border":
            inside = okx & oky & (xi >= -1) & (xi <= w) & (yi >= -1) & (yi <= h)
            xi, yi = np.clip(xi, 0, w - 1), np.clip(yi, 0, h - 1)
        tap.append((inside, np.where(inside, yi, 0), np.where(inside, xi, 0), ax[k & 1] * ay[k >> 1]))
    return tap, wx, wy


def point_feats(t, mode="f64", defect=None, pattern=None):
    """t: points [n,3], w2c [V,4,4], ixt [V,3,3], img_ref [V,3,h,w], image [V,h,w,3], acc_map [V,h,w], depth [V,h,w,1], g_out
    [V,8,n] (float32 numpy) -> out [V,8,n], d_points [n,3], d_image, d_acc_map, d_depth (= `pattern[name]` + the gradient), and
    x, y, z, wx, wy, resid = s_7 - z of every (view, point) for the cases' margins"""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        return _point_feats(t, mode, defect, pattern)


def _point_feats(t, mode, defect, pattern):
    V, _, h, w = t["img_ref"].shape
    n = t["points"].shape[0]
    stack = pack_stack(t)
    x, y, z = _project(t, mode)
    tap, wx, wy = _taps(x, y, h, w, mode, defect)
    vi = np.arange(V)[:, None]
    vals = [lift(np.where(ins[..., None], stack[vi, yi, xi], 0), mode) for ins, yi, xi, _ in tap]      # [V, n, 8] each
    zero = lift(np.zeros((V, n, 8)), mode)
    s = fsum([fwhere(ins[..., None], wg[..., None] * vl, zero) for (ins, _, _, wg), vl in zip(tap, vals)])
    resid = s[..., 7] - z
    out = fstack([s[..., c] for c in range(7)] + [fabs(resid)], axis=1)                                  # [V, 8, n]
    res = {"out": out, "x": x, "y": y, "z": z, "wx": wx, "wy": wy, "resid": resid}
    if "g_out" not in t:
        return res
    g = np.transpose(t["g_out"], (0, 2, 1)).astype(np.float64)                                          # [V, n, 8]
    sg = np.sign(val(resid)).astype(np.float64)
    if defect == "sign_of_zero_is_one":
        sg = np.where(val(resid) == 0, 1.0, sg)
    sg = np.where(np.isnan(sg), 0.0, sg)         # (d > 0 ? 1 : d < 0 ? -1 : 0 of a NaN)
    gc = g.copy()
    gc[..., 7] = g[..., 7] * sg
    gz = lift(-gc[..., 7], mode)
    gl = lift(gc, mode)
    omx, omy = 1.0 - wx, 1.0 - wy
    gx = fsum([gl[..., c] * ((vals[1][..., c] - vals[0][..., c]) * omy + (vals[3][..., c] - vals[2][..., c]) * wy) for c in range(8)])
    gy = fsum([gl[..., c] * ((vals[2][..., c] - vals[0][..., c]) * omx + (vals[3][..., c] - vals[1][..., c]) * wx) for c in range(8)])
    inv = 1.0 / z
    dq = [gx * inv, gy * inv, gz - fsum([gx * x, gy * y]) * inv]
    m = lambda r, c: lift(t["w2c"][:, r, c][:, None], mode)
    k = lambda r, c: lift(t["ixt"][:, r, c][:, None], mode)
    dc = [fsum([k(0, j) * dq[0], k(1, j) * dq[1], k(2, j) * dq[2]]) for j in range(3)]
    dp = [fsum([m(0, j) * dc[0], m(1, j) * dc[1], m(2, j) * dc[2]]) for j in range(3)]                 # [V, n] each
    views = range(V - 1 if (defect == "last_view_dropped" and V & (V - 1)) else V)
    res["d_points"] = fstack([fsum([d[v] for v in views]) if len(views) else lift(np.zeros(n), mode) for d in dp], axis=1)
    # the scatter: every tap inside the image adds weight * gradient to its pixel, channels 3 .. 7
    acc = {key: np.zeros((V, h, w, 5), dtype=np.float32 if mode == "f32" else np.float64) for key in ("v", "mag", "A", "n")}
    for ins, yi, xi, wg in tap:
        term = wg[..., None] * gl[..., 3:]
        where = (np.broadcast_to(vi, ins.shape)[ins], yi[ins], xi[ins])
        tv = val(term)[ins]
        if defect == "scatter_overwrites":
            acc["v"][where] = tv
        else:
            np.add.at(acc["v"], where, tv)
        if mode == "f64":
            np.add.at(acc["mag"], where, np.abs(tv))
            np.add.at(acc["A"], where, term.A[ins])
            np.add.at(acc["n"], where, (tv != 0).astype(np.float64))
    if mode == "f64":
        grad = B(acc["v"], acc["A"] + np.where(acc["n"] > 1, acc["n"] * U * acc["mag"], 0.0))
    else:
        grad = acc["v"]
    for name, sl, shape in (("d_image", slice(0, 3), (V, h, w, 3)), ("d_acc_map", 3, (V, h, w)), ("d_depth", slice(4, 5), (V, h, w, 1))):
        gpart = grad[..., sl]
        if pattern is not None and defect != "unpack_assigns":
            gpart = lift(pattern[name], mode) + gpart
        res[name] = gpart
    return res


def voxel_rows_backward(vox, g, n_vox):
    """dst[v] = sum of the rows r with vox[r] == v: -> (fp64 sum with its bound, the sequential fp32 sum in row order)"""
    vox = np.asarray(vox)
    v64, mag, cnt = (np.zeros((n_vox, g.shape[1])) for _ in range(3))
    np.add.at(v64, vox, g.astype(np.float64))
    np.add.at(mag, vox, np.abs(g.astype(np.float64)))
    np.add.at(cnt, vox, 1.0)
    seq = np.zeros((n_vox, g.shape[1]), dtype=np.float32)
    for r in range(len(vox)):
        seq[vox[r]] = seq[vox[r]] + g[r]
    return B(v64, np.where(cnt > 1, cnt * U * mag, 0.0)), seq


# ---------------------------------------------------------------------------------------------- the surface maps

def _nan_to_num00(x, x32, defect, mode):
    """torch.nan_to_num(x, 0, 0) of an fp32 number: nan, +inf -> 0, -inf -> -FLT_MAX (`x32`: the fp32 value that is classified)"""
    low = 0.0 if defect == "neg_inf_to_zero" else -F32_MAX
    zero = np.isnan(x32) | (x32 == np.inf)
    return fwhere(zero, lift(np.zeros(x32.shape), mode), fwhere(x32 == -np.inf, lift(np.full(x32.shape, low), mode), x))


def _cross(a, b):
    return [fsum([a[1] * b[2], -(a[2] * b[1])]), fsum([a[2] * b[0], -(a[0] * b[2])]), fsum([a[0] * b[1], -(a[1] * b[0])])]


def _same_operands(arrs, sl_a, sl_b):
    """both pixels of a difference have identical operands: the two points are the same bits, their difference is exactly 0"""
    with np.errstate(invalid="ignore"):
        return np.logical_and.reduce([np.all((x[sl_a] == x[sl_b]) | (np.isnan(x[sl_a]) & np.isnan(x[sl_b])), axis=-1) for x in arrs])


def surface_maps(t, ratio_, mode="f64", defect=None, grads=None):
    """t: color [n,3,H,W], allmap [n,7,H,W], rays [n,H,W,6], rots [n,9] (float32 numpy) -> the six maps side by side ([H, n*W, C]);
    with grads = {name: [H, n*W, C] or None} also d_color [n,3,H,W] and d_allmap [n,7,H,W]; `len`: the cross products' lengths
    and `sine` = |a x b| / (|a| |b|) at the interior pixels [n,H-2,W-2] for the cases' conditions"""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        return _surface_maps(t, ratio_, mode, defect, grads)


def _wide(x, n, W):
    """[n, H, W, ...] -> [H, n*W, ...]"""
    if isinstance(x, B):
        return B(_wide(x.v, n, W), _wide(x.A, n, W))
    return np.moveaxis(x, 0, 1).reshape((x.shape[1], n * W) + x.shape[3:])


def _narrow(x, n, W):
    """[H, n*W, ...] -> [n, H, W, ...]"""
    return np.moveaxis(x.reshape((x.shape[0], n, W) + x.shape[2:]), 1, 0)


def _surface_maps(t, ratio_, mode, defect, grads):
    color, allmap, rays = t["color"], t["allmap"], t["rays"]
    n, _, H, W = color.shape
    rot = t["rots"].reshape(n, 3, 3)
    L = lambda a: lift(a, mode)
    r, omr = L(np.float32(ratio_)), L(np.float32(1.0) - np.float32(ratio_))
    c0, alpha, md_raw = L(allmap[:, 0]), L(allmap[:, 1]), L(allmap[:, 5])
    e_raw = c0 / alpha
    e32, md32 = f32_of(e_raw), allmap[:, 5]
    e = _nan_to_num00(e_raw, e32, defect, mode)
    md = _nan_to_num00(md_raw, md32, defect, mode)
    depth = fsum([e * omr, r * md])                                                         # [n, H, W]
    P = [L(rays[..., j]) + depth * L(rays[..., 3 + j]) for j in range(3)]
    res = {"image": np.clip(color, 0, 1).transpose(0, 2, 3, 1), "acc_map": allmap[:, 1], "rend_dist": allmap[:, 6]}
    res["rend_normal"] = fstack([fsum([L(allmap[:, 2 + i]) * L(rot[:, i, j][:, None, None]) for i in range(3)]) for j in range(3)], -1)
    res["depth"] = depth[..., None]

    # the depth normals, on the views one by one -- or, the defect, on the side-by-side image as if it were one view
    cross_views = defect == "stencil_crosses_views"
    nn, WW = (1, n * W) if cross_views else (n, W)
    widen = (lambda a: _wide(a, n, W)[None]) if cross_views else (lambda a: a)
    Pw = [B(widen(p.v), widen(p.A)) if isinstance(p, B) else widen(p) for p in P]
    shared = [widen(a) for a in (allmap[:, 0, ..., None], allmap[:, 1, ..., None], allmap[:, 5, ..., None])]
    operands = [shared + [widen(rays[..., j:j + 1]), widen(rays[..., 3 + j:4 + j])] for j in range(3)]      # of component j of a point
    alpha_w = widen(allmap[:, 1])
    up, down, left, right = (np.s_[:, 2:, 1:-1], np.s_[:, :-2, 1:-1], np.s_[:, 1:-1, 2:], np.s_[:, 1:-1, :-2])
    mid = np.s_[:, 1:-1, 1:-1]
    a = [p[up] - p[down] for p in Pw]
    b = [p[left] - p[right] for p in Pw]
    if mode == "f64":
        same_a = [_same_operands(o, up, down) for o in operands]
        same_b = [_same_operands(o, left, right) for o in operands]
        a = [B(np.where(m, 0.0, q.v), np.where(m, 0.0, q.A)) for q, m in zip(a, same_a)]
        b = [B(np.where(m, 0.0, q.v), np.where(m, 0.0, q.A)) for q, m in zip(b, same_b)]
    c = _cross(a, b)
    ln = fsqrt(fsum([q * q for q in c]))
    ln32 = f32_of(ln)
    clamped = ~(ln32 > EPS12)
    inv = 1.0 / fwhere(clamped, L(np.full(ln32.shape, EPS12)), ln)
    al = L(alpha_w[mid])
    dn_mid = [q * inv * al for q in c]
    dn = [np.zeros((nn, H, WW), dtype=np.float32 if mode == "f32" else np.float64) for _ in range(3)]
    dnA = [np.zeros((nn, H, WW)) for _ in range(3)]
    for j in range(3):
        dn[j][mid] = val(dn_mid[j])
        if mode == "f64":
            dnA[j][mid] = dn_mid[j].A
    dn_full = fstack([B(v, A) if mode == "f64" else v for v, A in zip(dn, dnA)], -1)          # [nn, H, WW, 3]
    res["depth_normal"] = dn_full[0] if cross_views else _wide(dn_full, n, W)
    for k in ("image", "acc_map", "rend_dist", "rend_normal", "depth"):
        res[k] = _wide(res[k], n, W)
    la = fsqrt(fsum([q * q for q in a]))
    lb = fsqrt(fsum([q * q for q in b]))
    res["len"], res["sine"] = val(ln), val(ln) / (val(la) * val(lb))
    if grads is None:
        return res

    G = lambda k: None if grads.get(k) is None else _narrow(np.asarray(grads[k], dtype=np.float32), n, W)   # -> [n, H, W, (C)]
    zero = np.zeros((n, H, W), dtype=np.float32)
    # d_color: the clamp passes the gradient inside [0, 1], bounds included
    gi = G("image")
    if defect == "clamp_excludes_bounds":
        passes = (color > 0) & (color < 1)
    else:
        passes = (color >= 0) & (color <= 1)
    res["d_color"] = np.where(passes, gi.transpose(0, 3, 1, 2), 0).astype(np.float32) if gi is not None else np.zeros_like(color)
    gs = L(G("depth")[..., 0] if G("depth") is not None else zero)
    if G("depth_normal") is not None:
        gdn_w = np.asarray(grads["depth_normal"], dtype=np.float32)
        gdn = gdn_w[None] if cross_views else _narrow(gdn_w, n, W)
        g = [L(gdn[mid + (j,)]) * al for j in range(3)]
        live = ~clamped
        safe_ln = fwhere(live, ln, L(np.ones(ln32.shape)))
        iv = 1.0 / safe_ln
        nh = [q * iv for q in c]
        dot = fsum([nh[j] * g[j] for j in range(3)])
        gcr = [fwhere(live, (g[j] - nh[j] * dot) * iv, g[j] * L(BIG12)) for j in range(3)]
        ga, gb = _cross(b, gcr), _cross(gcr, a)

        def padded(q):      # [nn, H-2, WW-2] -> zero-padded [nn, H+2, WW+2], the interior at [2:-2, 2:-2]
            if isinstance(q, B):
                return B(np.pad(q.v, ((0, 0), (2, 2), (2, 2))), np.pad(q.A, ((0, 0), (2, 2), (2, 2))))
            return np.pad(q, ((0, 0), (2, 2), (2, 2)))
        gp = []
        flip = -1.0 if defect == "vjp_sign_flipped" else 1.0
        for j in range(3):
            pa, pb = padded(ga[j]), padded(gb[j])
            # pixel (y, x) is P(y+1, x) of the normal at (y-1, x), P(y-1, x) of the one at (y+1, x), likewise in x
            t1, t2 = pa[:, 0:H, 1:WW + 1], pa[:, 2:H + 2, 1:WW + 1]
            t3, t4 = pb[:, 1:H + 1, 0:WW], pb[:, 1:H + 1, 2:WW + 2]
            gp.append(fsum([t1, -(t2 * flip) if flip < 0 else -t2, t3, -t4]))
        if cross_views:
            gp = [B(_narrow(q.v[0], n, W), _narrow(q.A[0], n, W)) if isinstance(q, B) else _narrow(q[0], n, W) for q in gp]
        gs = fsum([gs] + [gp[j] * L(rays[..., 3 + j]) for j in range(3)])
    a32 = allmap[:, 1]
    e_ok = np.isfinite(e32) & (a32 != 0)
    md_ok = np.isfinite(md32)
    zl = L(zero)
    ge = gs * omr
    safe_alpha = fwhere(e_ok, alpha, L(np.ones_like(a32)))
    d = [fwhere(e_ok, ge / safe_alpha, zl)]
    g_acc = L(G("acc_map") if G("acc_map") is not None else zero)
    d.append(g_acc + fwhere(e_ok, (-ge) * c0 / (safe_alpha * safe_alpha), zl))
    grn = G("rend_normal")
    for i in range(3):
        if grn is None:
            d.append(zl)
        else:
            rr = rot.transpose(0, 2, 1) if defect == "rot_transposed" else rot
            d.append(fsum([L(rr[:, i, j][:, None, None]) * L(grn[..., j]) for j in range(3)]))
    d.append(fwhere(md_ok, gs * r, zl))
    d.append(L(G("rend_dist") if G("rend_dist") is not None else zero))
    res["d_allmap"] = fstack(d, 1)
    return res


# ---------------------------------------------------------------------------------------------- the activations

def activate_forward(opacity, scales, rotations, mode="f64"):
    """opacity [P], scales [P,2], rotations [P,4] (float32 numpy; the last two may be None) -> sigmoid, exp, x / max(|x|, 1e-12)"""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        L = lambda a: lift(a, mode)
        res = {"opacity": 1.0 / (1.0 + fexp(-L(opacity)))}
        if scales is not None:
            res["scales"] = fexp(L(scales))
        if rotations is not None:
            q = [L(rotations[:, j]) for j in range(4)]
            ln = fsqrt(fsum([x * x for x in q]))
            nrm = fwhere(f32_of(ln) > EPS12, ln, L(np.full(len(rotations), EPS12)))
            res["rotations"] = fstack([x / nrm for x in q], -1)
        return res


def activate_backward(o_act, s_act, rotations, g_o, g_s, g_r, mode="f64", defect=None):
    """the derivative formed from the ACTIVATED opacity and scales handed in (the device's own saved outputs) and the raw
    rotations; a None gradient is zero"""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        L = lambda a: lift(a, mode)
        res = {}
        if o_act is not None:
            y = L(o_act)
            res["d_opacity"] = L(g_o) * (1.0 - y) * y if g_o is not None else L(np.zeros_like(o_act))
        if s_act is not None:
            res["d_scales"] = L(g_s) * L(s_act) if g_s is not None else L(np.zeros_like(s_act))
        if rotations is not None:
            g = [L(g_r[:, j] if g_r is not None else np.zeros(len(rotations), dtype=np.float32)) for j in range(4)]
            q = [L(rotations[:, j]) for j in range(4)]
            ln = fsqrt(fsum([x * x for x in q]))
            live = f32_of(ln) > EPS12
            iv = 1.0 / fwhere(live, ln, L(np.ones(len(rotations))))
            y = [x * iv for x in q]
            dot = fsum([y[j] * g[j] for j in range(4)])
            big = L(np.float32(0.0)) if defect == "clamped_quaternion_zero" else L(BIG12)
            res["d_rotations"] = fstack([fwhere(live, (g[j] - y[j] * dot) * iv, g[j] * big) for j in range(4)], -1)
        return res
