"""The cases of tests/test_featvol_faithful.py and tests/test_featvol_faithful_gpu.py: shapes at the edges csrc/featvol.hip has
code for, seeded inputs, cameras fixed so that the position condition of oracle/featvol_bf16.py holds, and the reference's
results (computed once per case and regime, shared, never modified).

Cameras.  Focal lengths are powers of two; every translation is a multiple of 2^-10.  The kinds:
    frustum  looks down an axis of the volume from where the outermost grid columns of one grid plane project onto the map's
             borders: that plane straddles all four borders (and the corners), the nearer planes fall outside, the farther inside
    generic  a seeded rotation, focal length = the image size, an off-centre principal point
    inside   generic from twice as far in image terms (focal length = half the image size): every point inside the map
    corner   every point in the map's top-left half texel: one tap each, all on texel 0
    blind    generic, moved 8 units sideways: sees no point at all
`cameras` nudges each view's translation by multiples of 2^-10, in a fixed order, until the reference reports no point of that
view whose rounding could go the other way on the device (`position_checks`).
"""
import functools
import math

import torch

from oracle import featvol_bf16 as fb

# (B, V, C, E, h, w, R), the input image's (img_w, img_h) and the kind of every view
CASES = {
    "a": ((1, 1, 64, 0, 1, 1, 1), (16, 16), [["single"]]),
    "b": ((2, 3, 320, 4, 5, 7, 5), (64, 32), [["frustum", "generic", "blind"], ["generic", "frustum", "generic"]]),
    "c": ((1, 8, 64, 32, 3, 2, 6), (32, 32), [["frustum", "inside", "inside", "generic", "inside", "corner", "inside", "blind"]]),
    "d": ((1, 2, 1024, 256, 9, 15, 4), (128, 128), [["frustum", "blind"]]),
    "e": ((1, 4, 128, 32, 64, 128, 3), (512, 512), [["frustum", "generic", "blind", "generic"]]),
}
REGIMES = ("A", "B")
EPS = 1e-6
STEP = 2.0 ** -10
_PERMS = [((0, 1), (1, 1), (2, 1)), ((1, 1), (0, -1), (2, 1)), ((2, -1), (1, 1), (0, 1)), ((0, 1), (2, 1), (1, -1))]


def _q(v):
    return round(v / STEP) * STEP


def _rotation(g):
    a, b, c = (float(t) for t in (torch.rand(3, generator=g, dtype=torch.float64) - 0.5) * 1.6)
    rx = torch.tensor([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]], dtype=torch.float64)
    ry = torch.tensor([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]], dtype=torch.float64)
    rz = torch.tensor([[math.cos(c), -math.sin(c), 0], [math.sin(c), math.cos(c), 0], [0, 0, 1]], dtype=torch.float64)
    return rz @ ry @ rx


def _camera(kind, n, R, img_w, img_h, g):
    """-> (w2c [4, 4], ixt [3, 3]) fp32 of view number n of its case"""
    w2c, ixt = torch.eye(4, dtype=torch.float64), torch.eye(3, dtype=torch.float64)
    u = torch.rand(4, generator=g, dtype=torch.float64)
    if kind == "frustum":
        for row, (col, sign) in enumerate(_PERMS[n % len(_PERMS)]):
            w2c[row, :3] = 0.0
            w2c[row, col] = sign
        coords = sorted({float(v) for v in fb.dense_grid(R)[:, 0]})
        edge, plane = coords[-1], coords[-2] if R > 1 else 0.0
        # f = 2 * size and the principal point at the image's centre: the column at +-edge of the plane at depth tz + plane
        # projects to 2 * size * edge / (tz + plane) = size / 2 from the centre, the image's border
        w2c[2, 3] = _q(4 * edge - plane)
        ixt[0, 0], ixt[1, 1], ixt[0, 2], ixt[1, 2] = 2 * img_w, 2 * img_h, img_w / 2 - 0.5, img_h / 2 - 0.5
        return w2c.float(), ixt.float()
    if kind == "single":          # case (a): the one point at the origin, at map position (-0.25, 0.125) of the 1 x 1 map
        w2c[:3, :3] = _rotation(g)
        w2c[:3, 3] = torch.tensor([-0.5, 0.25, 2.0], dtype=torch.float64)
        ixt[0, 0], ixt[1, 1], ixt[0, 2], ixt[1, 2] = img_w, img_h, img_w / 2 - 0.5, img_h / 2 - 0.5
        return w2c.float(), ixt.float()
    w2c[:3, :3] = _rotation(g)
    if kind == "corner":
        ixt[0, 0], ixt[1, 1], ixt[0, 2], ixt[1, 2] = img_w / 8, img_h / 8, -0.5, -0.5
        w2c[:3, 3] = torch.tensor([0.0, 0.0, 2.0], dtype=torch.float64)
        return w2c.float(), ixt.float()
    zoom = 0.5 if kind == "inside" else 1.0
    ixt[0, 0], ixt[1, 1] = zoom * img_w, zoom * img_h
    ixt[0, 2] = img_w / 2 - 0.5 + math.floor((float(u[0]) - 0.5) * img_w / 4)
    ixt[1, 2] = img_h / 2 - 0.5 + math.floor((float(u[1]) - 0.5) * img_h / 4)
    spread = 0.2 if kind == "inside" else 0.6
    w2c[:3, 3] = torch.tensor([_q((float(u[2]) - 0.5) * spread), _q((float(u[3]) - 0.5) * spread), 2.0], dtype=torch.float64)
    if kind == "blind":
        w2c[0, 3] += 8.0
    return w2c.float(), ixt.float()


def _nudges():
    """(0, 0, 0), then +-1, +-2, ... steps along x, y, z in turn"""
    yield (0, 0, 0)
    for m in range(1, 64):
        for sign in (1, -1):
            for axis in range(3):
                yield tuple(sign * m if i == axis else 0 for i in range(3))


@functools.lru_cache(maxsize=None)
def cameras(case):
    """-> (w2c [B, V, 4, 4], ixt [B, V, 3, 3], the nudge each view took)"""
    (B, V, C, E, h, w, R), (img_w, img_h), kinds = CASES[case]
    g = torch.Generator().manual_seed(1000 + ord(case))
    grid = fb.dense_grid(R)
    w2cs, ixts, taken = [], [], []
    for b in range(B):
        for v in range(V):
            w2c, ixt = _camera(kinds[b][v], b * V + v, R, img_w, img_h, g)
            for nudge in _nudges():
                cand = w2c.clone()
                cand[:3, 3] += torch.tensor(nudge, dtype=torch.float32) * STEP
                _, _, info = fb.positions(grid, cand[None], ixt[None], img_w, img_h, h, w)
                if not bool(fb.position_checks(info).any()) and float(info["qz"].abs().min()) > 1e-3:
                    break
            else:
                raise AssertionError(f"case {case}, view {b}/{v}: no translation within 63 steps of 2^-10 satisfies the position condition")
            w2cs.append(cand); ixts.append(ixt); taken.append(nudge)
    return torch.stack(w2cs).view(B, V, 4, 4), torch.stack(ixts).view(B, V, 3, 3), taken


@functools.lru_cache(maxsize=None)
def inputs(case, regime):
    """fp32 tensors, as the device gets them (x as rows [B V, h w, C]: the layouts are views of it), and the fp64 dict the
    reference takes"""
    (B, V, C, E, h, w, R), (img_w, img_h), _ = CASES[case]
    g = torch.Generator().manual_seed(ord(case))
    T, S = B * V * h * w, R ** 3
    # rows whose mean and scale vary per row, so that LayerNorm's statistics matter
    rows = torch.randn(T, C, generator=g) * (0.5 + 1.5 * torch.rand(T, 1, generator=g)) + torch.randn(T, 1, generator=g)
    t = {"rows": rows.view(B * V, h * w, C), "rays": torch.randn(B, V, h, w, 6, generator=g),
         "ln_w": 1 + 0.3 * torch.randn(C, generator=g), "ln_b": 0.2 * torch.randn(C, generator=g),
         "mlp_w": 0.3 * torch.randn(2 * C, 32, generator=g), "mlp_b": 0.3 * torch.randn(2 * C, generator=g),
         "embed": torch.randn(V, E, generator=g) * (1.0 / max(E, 1)) ** 0.5 if E else None,
         "grad": torch.randn(B, V, C + E, S, generator=g)}
    if regime == "A":
        t["mlp_w"] = torch.zeros(2 * C, 32)
    t["w2c"], t["ixt"], _ = cameras(case)
    ref = {k: (None if t[k] is None else t[k].double()) for k in ("rays", "w2c", "ixt", "ln_w", "ln_b", "mlp_w", "mlp_b", "embed")}
    ref["x"] = t["rows"].double().view(B * V, h, w, C).permute(0, 3, 1, 2)
    ref.update(R=R, img_w=img_w, img_h=img_h, eps=EPS)
    return t, ref


@functools.lru_cache(maxsize=None)
def reference(case, regime):
    """(faithful, unrounded) results of oracle.featvol_bf16.backward; `unrounded` keeps the position roundings (the yardstick's
    noise is that of the modulation: the positions are the device's bit for bit)"""
    t, ref = inputs(case, regime)
    grad = t["grad"].double()
    return fb.backward(ref, grad, True, True), fb.backward(ref, grad, False, True)


def rel(a, b, ref):
    """(l2, max-norm) of a - b relative to ref"""
    a, b, ref = a.double().reshape(-1), b.double().reshape(-1), ref.double().reshape(-1)
    return float((a - b).norm() / ref.norm()), float((a - b).abs().max() / ref.abs().max())


def yardstick_tensors(case, regime):
    """{name: (faithful, unrounded)} of the tensors the noise yardstick is used on: everything in regime B, the Linear's
    gradients in both (d_view_embed is a plain fp32 sum in either)"""
    fa, un = reference(case, regime)
    names = ("d_mlp_w", "d_mlp_b") if regime == "A" else ("out", "tokens", "dx", "d_ln_w", "d_ln_b", "d_mlp_w", "d_mlp_b")
    get = lambda r, k: r["fwd"][k] if k in ("out", "tokens") else r[k]
    return {k: (get(fa, k), get(un, k)) for k in names}
