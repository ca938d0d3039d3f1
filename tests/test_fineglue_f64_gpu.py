"""The fp32 kernels between the learned blocks of the fine pass -- csrc/pointfeat.hip (projection, bilinear gather, atomic scatter,
lane-shuffle view sum, take_rows / voxel_rows) and csrc/surface.hip (surface maps, depth normals with their 4-neighbour VJP, the
three activations) -- through the entry points of include/lara_pointfeat.h and include/lara_surface.h (`lara_amd._native.call`
and `query`, buffers the test owns), against the fp64 reference (oracle/fineglue_f64.py) at the cases of tests/fineglue_cases.py.
tests/test_fineglue_f64.py shows (without a GPU) that every case meets its condition, that a plain fp32 evaluation passes every
check below, and that twelve wrong ones do not.

Exact-arithmetic sampler cases (every intermediate representable in fp32, sums exact below 2^24): out, d_points and the three map
gradients equal the reference BIT FOR BIT, in any atomic order -- samples on every combination of x, y in {-1.25, -1, -0.5, 0,
0.25, w-1.25, w-1, w-0.5, w, w+1, w+2, 3 * 2^20}, q.z < 0, integer positions, 2000 points on one position, +-2^31-scale
positions, the | s - z | kink; gradient maps pre-filled with a pattern (the result is pattern + gradient), each of the three
pointers NULL in turn and all three; the [V,h,w,c] layout and the side-by-side layout with row_views = V and V + 3 (views >= V
keep the pattern's bits, their source columns are NaN).  Everything else, element by element, nothing exempted:
        |got - ref| <= 4 A + 2^-23 |ref|
with A the fp32 error bound of THAT element from the reference's own operands; A = 0 and ref = 0: exactly 0; a reference that is
inf or NaN: the same class.

Memory discipline, in every test: every output sits NaN-filled (the accumulated maps: pattern-filled) between two NaN guards that
are intact afterwards; the sampler's workspace is 0xFF-filled in one run and zero-filled in the next, with the same bits out;
two runs give the same bits wherever no float atomic is involved; n = 0, P = 0, n_views = 0 write nothing.

Every worst |diff| / limit, per tensor and case, goes to fineglue_f64_errors.json in the directory LARA2DGS_TEST_OUT names
(default: test_out/ in the repository root, kept out of git).

Measured on an MI355X (first clean run, all 75 tests; the whole file takes 8 s).  The exact-arithmetic cases came out bit for
bit in all 30 runs (two variants, three layouts, five NULL combinations).  The largest |diff| / limit anywhere is 0.188
(d_scales, P = 257: one product).  Per tensor -- sampler: out 0.074, d_points 0.162 (V = 1, n = 65), d_image 0.076, d_acc_map
0.057, d_depth 0.062 (white-noise maps, 4 views, 1500 points; the smooth cases and the 40 lane cases stay below 0.03 on the
maps), voxel_rows' sum 0.095; surface maps: depth 0.127, rend_normal 0.116, depth_normal 0.094, d_allmap 0.182 (3 x 300, three
views, g_depth alone), image, acc_map, rend_dist, d_color 0 (copies and the clamp), the special pixels no higher than the
ordinary ones; activations: opacity 0.140, scales 0.122 (of a limit of five ulps: the device's expf is within 0.61 ulp),
rotations 0.115, d_opacity 0.177, d_scales 0.188, d_rotations 0.159.  The fp32 CPU stand-in of tests/test_fineglue_f64.py lands
at the same level (0.06 - 0.21 per tensor).  d_points of a point with a non-finite position is NaN in all three components (both bad
points).  These cases found no defect in csrc/pointfeat.hip or csrc/surface.hip, nor in their wrappers: every test passed on
the kernels as they were.
"""
import json
import os

import numpy as np
import pytest
import torch

from lara_amd._native import RowsItem, call, query
from oracle import fineglue_f64 as fg
from tests import fineglue_cases as fc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SAMPLER_KEYS = ("out", "d_points") + fc.GRAD_KEYS
SURFACE_KEYS = fc.MAP_KEYS + ("d_color", "d_allmap")
_LOG = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_errors():
    yield
    if not _LOG:
        return
    out = os.environ.get("LARA2DGS_TEST_OUT") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "test_out")
    os.makedirs(out, exist_ok=True)
    per_tensor = {}
    for key, v in _LOG.items():
        name = key.rsplit("/", 1)[1]
        if v > per_tensor.get(name, (-1.0, ""))[0]:
            per_tensor[name] = (v, key)
    with open(os.path.join(out, "fineglue_f64_errors.json"), "w") as f:
        json.dump({"max_diff_over_limit": max(_LOG.values()), "per_tensor": {k: {"worst": v, "at": at} for k, (v, at) in per_tensor.items()},
                   "worst_diff_over_limit": _LOG}, f, indent=1)


# ---------------------------------------------------------------------------------------------- device plumbing

class Guarded:
    """fp32 tensors inside NaN-filled allocations with a NaN guard on either side; `check()` finds a write outside any of them"""

    def __init__(self):
        self.items = []

    def out(self, shape, fill=None):
        """an output: NaN-filled, or holding `fill` (a numpy array)"""
        k = int(np.prod(shape))
        whole = torch.full((GUARD + k + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
        x = whole[GUARD:GUARD + k].view(tuple(shape))
        if fill is not None:
            x.copy_(torch.from_numpy(np.ascontiguousarray(fill, dtype=np.float32)).view(tuple(shape)))
        self.items.append((whole, k))
        return x

    def inp(self, a):
        """an input inside a larger NaN-filled allocation: a read beyond it shows"""
        return self.out(np.shape(a), fill=a)

    def check(self):
        torch.cuda.synchronize()
        for whole, k in self.items:
            assert bool(torch.isnan(whole[:GUARD]).all()) and bool(torch.isnan(whole[GUARD + k:]).all()), "written outside a tensor"


def _workspace(nbytes, fill):
    whole = torch.full((nbytes + 2 * GUARD,), fill, dtype=torch.uint8, device=DEV)
    return whole, whole[GUARD:GUARD + nbytes]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_sampler(t, R=0, pattern=None, null=(), ws_fill=0xFF, backward=True, concat=False):
    """lara_point_feats_forward / _backward (R = 0: the plain entry points, or `_concat` with row_views = 0; R > 0: `_concat` with
    row_views = R, the maps side by side with NaN in the views >= V) -> {name: numpy}, the map gradients in the layout they were
    written in"""
    V, _, h, w = t["img_ref"].shape
    n = t["points"].shape[0]
    gd = Guarded()
    maps = fc.to_side_by_side(t, R) if R else {k: t[k] for k in ("image", "acc_map", "depth")}
    d = {k: gd.inp(t[k]) for k in ("points", "w2c", "ixt", "img_ref")}
    d.update({k: gd.inp(v) for k, v in maps.items()})
    ins = [d[k] for k in ("points", "w2c", "ixt", "img_ref", "image", "acc_map", "depth")]
    nbytes = query("lara_point_feats_workspace_bytes", V, h, w)
    assert nbytes == V * h * w * 64
    ws_whole, ws = _workspace(nbytes, ws_fill)
    out = gd.out((V, 8, n))
    head = (n, V, R, h, w) if R or concat else (n, V, h, w)
    suffix = "_concat" if R or concat else ""
    call("lara_point_feats_forward" + suffix, DEV, *head, *ins, out, ws)
    res = {"out": out}
    if backward:
        res["d_points"] = gd.out((n, 3))
        pat = pattern if pattern is not None else {k: np.zeros_like(t[src]) for k, src in zip(fc.GRAD_KEYS, ("image", "acc_map", "depth"))}
        if R:      # the pattern side by side as well; the views >= V hold 0.375, which must still be there afterwards
            wide = fc.to_side_by_side({"image": pat["d_image"], "acc_map": pat["d_acc_map"], "depth": pat["d_depth"]}, R, fill=0.375)
            pat = {"d_image": wide["image"], "d_acc_map": wide["acc_map"], "d_depth": wide["depth"]}
        grads = {k: (None if k in null else gd.out(pat[k].shape, fill=pat[k])) for k in fc.GRAD_KEYS}
        call("lara_point_feats_backward" + suffix, DEV, *head, *ins, gd.inp(t["g_out"]), res["d_points"], grads["d_image"], grads["d_acc_map"],
             grads["d_depth"], ws)
        res.update({k: v for k, v in grads.items() if v is not None})
    gd.check()
    assert bool((ws_whole[:GUARD] == ws_fill).all()) and bool((ws_whole[GUARD + nbytes:] == ws_fill).all()), "written outside the workspace"
    return {k: v.cpu().numpy() for k, v in res.items()}


def _stacked(res, V, R):
    """the map gradients of a side-by-side run as ([V,h,w,(c)] of the first V views, the untouched rest)"""
    if not R:
        return res, {}
    out, rest = dict(res), {}
    for k in fc.GRAD_KEYS:
        if k in res:
            out[k], rest[k] = fc.from_side_by_side(res[k], V, R)
    return out, rest


def _record(prefix, res):
    for k, v in res.items():
        key = f"{prefix}/{k}"
        _LOG[key] = max(v, _LOG.get(key, 0.0))
        print(f"{key:56s} worst |diff| / limit = {v:.4f}")
    return [f"{prefix}/{k}: worst |diff| / limit = {v:.3f}" for k, v in res.items() if not v <= 1.0]


# ---------------------------------------------------------------------------------------------- the point sampler

@pytest.mark.parametrize("R", [0, fc.EX_V, fc.EX_V + 3])
@pytest.mark.parametrize("variant", ["edges", "kink"])
def test_sampler_exact_cases_bit_for_bit(hip_lib, variant, R):
    """forward, d_points and the three map gradients (pattern + gradient) of the exact-arithmetic cases, with every combination
    of NULL gradient pointers the header allows, a 0xFF-filled and a zero-filled workspace: the reference's bits"""
    t = fc.exact_inputs(variant)
    V = fc.EX_V
    pat = fc.pattern_for(t)
    ref = fc.exact_reference(t, pat)
    fails = []
    for i, null in enumerate(((), ("d_image",), ("d_acc_map",), ("d_depth",), fc.GRAD_KEYS)):
        got, rest = _stacked(run_sampler(t, R, pat, null, ws_fill=0xFF if i % 2 == 0 else 0, concat=i % 2 == 1), V, R)
        assert set(got) == set(SAMPLER_KEYS) - set(null)
        for k in got:
            if not fc.same_bits(got[k], ref[k]):
                bad = np.flatnonzero(got[k].ravel() != ref[k].ravel())
                fails.append(f"{k} (NULL: {null}): {len(bad)} elements differ, first at {bad[:3]}: got {got[k].ravel()[bad[:3]]}, want {ref[k].ravel()[bad[:3]]}")
        for k, x in rest.items():
            assert (x == 0.375).all(), f"{k}: a view >= V received something"
    if variant == "kink":
        cluster = slice(t["n_edge"], t["n_lattice"])
        assert (got["out"][:, 7, cluster] == 0).all() and not got["d_points"][cluster].any()
    assert not fails, "; ".join(fails)


@pytest.mark.parametrize("case", fc.GENERAL_CASES, ids=lambda c: "-".join(map(str, c)))
def test_sampler_general_position(hip_lib, case):
    """every element of out, d_points and the three accumulated map gradients within its bound, in both layouts"""
    t = fc.general_case(*case)
    V = case[1]
    pat = fc.pattern_for(t, salt=3)
    ref = fg.point_feats(t, "f64", pattern=pat)
    fc.general_self_check(t, ref)
    fails = []
    for R in (0, V + 3):
        got, rest = _stacked(run_sampler(t, R, pat), V, R)
        fails += _record(f"general-{case[0]}-V{V}-n{case[2]}-R{R}", fc.worst(got, ref, SAMPLER_KEYS))
        assert all((x == 0.375).all() for x in rest.values())
    assert not fails, "; ".join(fails)


@pytest.mark.parametrize("V", range(1, 9))
def test_sampler_lanes(hip_lib, V):
    """V = 1 .. 8 (VP = 1, 2, 4, 8 with padding lanes) at n = 1, 63, 64, 65, 333: the last wave of the last workgroup is part-empty
    on every path; d_points is the sum over exactly V views.  Position independence at n = 333: the rows rotated by 37, and the
    first 100 rows run alone, give the same bits in out and d_points."""
    fails = []
    for n in (1, 63, 64, 65, 333):
        t = fc.general_inputs(V, n)
        ref = fg.point_feats(t, "f64")
        got = run_sampler(t)
        fails += _record(f"lanes-V{V}-n{n}", fc.worst(got, ref, SAMPLER_KEYS))
        again = run_sampler(t, ws_fill=0)
        assert fc.same_bits(again["out"], got["out"]) and fc.same_bits(again["d_points"], got["d_points"]), "two runs differ"
    rolled = run_sampler(dict(t, points=np.roll(t["points"], 37, 0), g_out=np.roll(t["g_out"], 37, 2)))
    head = run_sampler(dict(t, points=t["points"][:100], g_out=np.ascontiguousarray(t["g_out"][:, :, :100])))
    assert fc.same_bits(np.roll(rolled["out"], -37, 2), got["out"]) and fc.same_bits(np.roll(rolled["d_points"], -37, 0), got["d_points"]), \
        "a point's bits change with its row"
    assert fc.same_bits(head["out"], got["out"][:, :, :100]) and fc.same_bits(head["d_points"], got["d_points"][:100]), "a point's bits change with n"
    assert not fails, "; ".join(fails)


def test_sampler_non_finite_positions(hip_lib):
    """A point on a camera's plane (q.z = 0) and a NaN coordinate.  Forward: every tap is outside, channels 0..6 are 0, channel 7
    is |0 - z|.  Backward: the maps receive nothing from that (point, view) and stay finite; out and d_points of every other
    point are the bits of a run without the bad points.  d_points of the bad points themselves is NaN (0 * inf and NaN weights
    in the coordinate gradient), as the torch restatement's is: recorded in the header, not held to a value."""
    t, bad = fc.nonfinite_inputs()
    ref = fg.point_feats(t, "f64")
    got = run_sampler(t, concat=True)
    for v, i in ((1, bad[0]), (0, bad[1]), (1, bad[1]), (2, bad[1])):
        assert not got["out"][v, :7, i].any(), (v, i)
    assert got["out"][1, 7, bad[0]] == 0 and np.isnan(got["out"][:, 7, bad[1]]).all()
    res = fc.worst(got, ref, ("out",) + fc.GRAD_KEYS)
    keep = np.setdiff1d(np.arange(len(t["points"])), bad)
    clean = run_sampler(dict(t, points=t["points"][keep], g_out=np.ascontiguousarray(t["g_out"][:, :, keep])))
    assert fc.same_bits(clean["out"], got["out"][:, :, keep]) and fc.same_bits(clean["d_points"], got["d_points"][keep])
    res["d_points"] = float(fg.ratio(got["d_points"][keep], ref["d_points"][keep]).max())
    print("d_points of the bad points:", got["d_points"][bad].tolist())
    assert np.isnan(got["d_points"][bad]).all()
    fails = _record("nonfinite", res)
    assert not fails, "; ".join(fails)


def test_sampler_no_points(hip_lib):
    t = fc.general_inputs(3, 1)
    gd = Guarded()
    d = {k: _dev(t[k]) for k in ("points", "w2c", "ixt", "img_ref", "image", "acc_map", "depth", "g_out")}
    ins = [d[k] for k in ("points", "w2c", "ixt", "img_ref", "image", "acc_map", "depth")]
    outs = [gd.out((16,)) for _ in range(5)]
    _, ws = _workspace(query("lara_point_feats_workspace_bytes", 3, fc.GEN_H, fc.GEN_W), 0xFF)
    call("lara_point_feats_forward", DEV, 0, 3, fc.GEN_H, fc.GEN_W, *ins, outs[0], ws)
    call("lara_point_feats_backward", DEV, 0, 3, fc.GEN_H, fc.GEN_W, *ins, d["g_out"], *outs[1:], ws)
    call("lara_point_feats_backward_concat", DEV, 0, 3, 5, fc.GEN_H, fc.GEN_W, *ins, d["g_out"], *outs[1:], ws)
    gd.check()
    assert all(bool(torch.isnan(o).all()) for o in outs) and bool((ws == 0xFF).all()), "n = 0 wrote something"


@pytest.mark.parametrize("width", [4, 80])
def test_voxel_rows(hip_lib, width):
    """forward: the rows of the voxels, bit for bit; backward: the sequential fp32 sum in row order, bit for bit, and within the
    bound of the fp64 sum; runs at row 0 and row n - 1, 1000 rows on the last voxel, voxels without a row keep the caller's zeros"""
    c = fc.voxel_rows_case(width)
    n, gd = len(c["vox"]), Guarded()
    vox, src, g = _dev(c["vox"]), gd.inp(c["src"]), gd.inp(c["g"])
    rows, dst = gd.out((n, width)), gd.out((c["n_vox"], width), fill=np.zeros((c["n_vox"], width)))
    call("lara_voxel_rows", DEV, n, width, vox, src, rows, 0)
    call("lara_voxel_rows", DEV, n, width, vox, g, dst, 1)
    untouched = gd.out((16,))
    call("lara_voxel_rows", DEV, 0, width, vox, g, untouched, 1)
    call("lara_voxel_rows", DEV, 0, width, vox, g, untouched, 0)
    gd.check()
    assert bool(torch.isnan(untouched).all())
    assert fc.same_bits(rows.cpu().numpy(), c["src"][c["vox"]])
    ref, seq = fg.voxel_rows_backward(c["vox"], c["g"], c["n_vox"])
    assert fc.same_bits(dst.cpu().numpy(), seq), "not the sum in row order"
    fails = _record(f"voxel_rows-{width}", {"dst": float(fg.ratio(dst.cpu().numpy(), ref).max())})
    assert not fails, fails


@pytest.mark.parametrize("n", [1, 300])
def test_take_rows(hip_lib, n):
    """count = 8 with widths {1, 2, 3, 4, 12, 1, 2, 4}: the gather, and the scatter into zero-filled tensors"""
    rng = np.random.default_rng(n)
    rows, gd = 500, Guarded()
    idx = np.sort(rng.permutation(rows)[:n]).astype(np.int64)
    idx[-1] = rows - 1
    srcs = [rng.standard_normal((rows, w)).astype(np.float32) for w in fc.TAKE_WIDTHS]
    gs = [rng.standard_normal((n, w)).astype(np.float32) for w in fc.TAKE_WIDTHS]

    def items(src, dst):
        arr = (RowsItem * 8)()
        for k in range(8):
            arr[k].src, arr[k].dst, arr[k].width = src[k].data_ptr(), dst[k].data_ptr(), fc.TAKE_WIDTHS[k]
        return arr
    d_src, d_g = [gd.inp(x) for x in srcs], [gd.inp(x) for x in gs]
    taken = [gd.out((n, w)) for w in fc.TAKE_WIDTHS]
    spread = [gd.out((rows, w), fill=np.zeros((rows, w))) for w in fc.TAKE_WIDTHS]
    didx = _dev(idx)
    call("lara_take_rows", DEV, n, didx, 8, items(d_src, taken), 0)
    call("lara_take_rows", DEV, n, didx, 8, items(d_g, spread), 1)
    untouched = [gd.out((4, w)) for w in fc.TAKE_WIDTHS]
    call("lara_take_rows", DEV, 0, didx, 8, items(d_src, untouched), 0)
    call("lara_take_rows", DEV, n, didx, 0, items(d_src, untouched), 0)
    gd.check()
    assert all(bool(torch.isnan(u).all()) for u in untouched)
    for k in range(8):
        assert fc.same_bits(taken[k].cpu().numpy(), srcs[k][idx]), k
        want = np.zeros((rows, fc.TAKE_WIDTHS[k]), np.float32)
        want[idx] = gs[k]
        assert fc.same_bits(spread[k].cpu().numpy(), want), k


# ---------------------------------------------------------------------------------------------- the surface maps

SHAPES = {"image": 3, "depth": 1, "acc_map": 0, "rend_normal": 3, "depth_normal": 3, "rend_dist": 0}


def run_surface(t, ratio, grads=None, single=False, d_allmap=True):
    """lara_surface_maps_forward_views / _backward_views (single: the one-view entry points) -> {name: numpy}"""
    n, _, H, W = t["color"].shape
    gd = Guarded()
    ins = [gd.inp(t[k]) for k in ("color", "allmap", "rays", "rots")]
    outs = {k: gd.out((H, n * W) + ((c,) if c else ())) for k, c in SHAPES.items()}
    head = (H, W) if single else (n, H, W)
    suffix = "" if single else "_views"
    call("lara_surface_maps_forward" + suffix, DEV, *head, *ins, float(ratio), *(outs[k] for k in fc.MAP_KEYS))
    res = dict(outs)
    if grads is not None:
        res["d_color"] = gd.out((n, 3, H, W))
        if d_allmap:
            res["d_allmap"] = gd.out((n, 7, H, W))
        gs = [None if grads[k] is None else gd.inp(grads[k]) for k in fc.MAP_KEYS]
        call("lara_surface_maps_backward" + suffix, DEV, *head, *ins, float(ratio), *gs, res["d_color"], res.get("d_allmap"))
    gd.check()
    return {k: v.cpu().numpy() for k, v in res.items()}


def _surface_case(t, ratio, whiches, prefix, special):
    fails = []
    for which in whiches:
        g = fc.surface_grads(t, which)
        ref = fg.surface_maps(t, ratio, "f64", grads=g)
        fc.surface_self_check(t, ref, special)
        got = run_surface(t, ratio, g)
        fails += _record(f"{prefix}-{which}", fc.worst(got, ref, SURFACE_KEYS))
        again = run_surface(t, ratio, g, single=t["color"].shape[0] == 1)
        assert all(fc.same_bits(again[k], got[k]) for k in got), "two runs (n = 1: the two entry points) differ"
        if which == "image":      # only g_image: d_allmap may be NULL, d_color has the same bits
            assert fc.same_bits(run_surface(t, ratio, g, d_allmap=False)["d_color"], got["d_color"])
    return fails


@pytest.mark.parametrize("H,W,n,ratio", fc.SURFACE_CASES)
def test_surface_maps_ordinary_pixels(hip_lib, H, W, n, ratio):
    """every element of the six outputs, d_color and d_allmap, with the gradient of each output alone (the other five pointers
    NULL) and of all six together"""
    fails = _surface_case(fc.surface_inputs(H, W, n), ratio, ("all",) + fc.MAP_KEYS, f"surface-{H}x{W}-n{n}-r{ratio}", False)
    assert not fails, "; ".join(fails)


@pytest.mark.parametrize("H,W", fc.SPECIAL_SIZES)
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("ratio", [0.0, 0.25, 1.0])
def test_surface_maps_special_pixels(hip_lib, H, W, n, ratio):
    """alpha in {0, -0.0}, allmap[0] NaN, median depth in {NaN, +inf, -inf}, a constant-depth patch under parallel rays with a
    single origin (cross product, normal and gradient exactly 0) and with collinear origins (cross product exactly 0 with a, b
    non-zero: the backward is g * 1e12 through cross3), colours 0, 1, -2^-149, 1 + 2^-23: these pixels and their stencil
    neighbours under the same limit as every other element"""
    fails = _surface_case(fc.surface_inputs(H, W, n, special=True), ratio, ("all", "depth_normal", "depth", "image"),
                          f"special-{H}x{W}-n{n}-r{ratio}", True)
    assert not fails, "; ".join(fails)


def test_surface_maps_view_borders(hip_lib):
    """a huge g_depth_normal on view 1's border columns leaves d_allmap bit-identical to a run where that gradient is 0"""
    t = fc.surface_inputs(17, 16, 3)
    g = fc.surface_grads(t, "all")
    huge = {k: v.copy() for k, v in g.items()}
    huge["depth_normal"][:, [16, 31]] = 1e30
    zero = {k: v.copy() for k, v in g.items()}
    zero["depth_normal"][:, [16, 31]] = 0
    a, b = run_surface(t, 0.25, huge)["d_allmap"], run_surface(t, 0.25, zero)["d_allmap"]
    assert fc.same_bits(a, b)


def test_surface_maps_nothing_to_do(hip_lib):
    t = fc.surface_inputs(3, 3, 1)
    gd = Guarded()
    ins = [_dev(t[k]) for k in ("color", "allmap", "rays", "rots")]
    outs = [gd.out((16,)) for _ in range(8)]
    for head in ((0, 3, 3), (1, 0, 3), (1, 3, 0)):
        call("lara_surface_maps_forward_views", DEV, *head, *ins, 0.25, *outs[:6])
        call("lara_surface_maps_backward_views", DEV, *head, *ins, 0.25, *outs[:6], outs[6], outs[7])
    gd.check()
    assert all(bool(torch.isnan(o).all()) for o in outs)


# ---------------------------------------------------------------------------------------------- the activations

def run_activations(t, scales=True, rotations=True, g=(True, True, True), d=(True, True, True)):
    P = len(t["opacity"])
    gd = Guarded()
    o, s, r = gd.inp(t["opacity"]), gd.inp(t["scales"]), gd.inp(t["rotations"])
    res = {"opacity": gd.out((P,)), "scales": gd.out((P, 2)) if scales else None, "rotations": gd.out((P, 4)) if rotations else None}
    call("lara_activate_gaussians_forward", DEV, P, o, s if scales else None, r if rotations else None, res["opacity"], res["scales"], res["rotations"])
    if scales and rotations:
        gs = [gd.inp(t[k]) if on else None for k, on in zip(("g_opacity", "g_scales", "g_rotations"), g)]
        ds = [gd.out(shape) if on else None for shape, on in zip(((P,), (P, 2), (P, 4)), d)]
        call("lara_activate_gaussians_backward", DEV, P, res["opacity"], res["scales"], r, *gs, *ds)
        res.update(dict(zip(("d_opacity", "d_scales", "d_rotations"), ds)))
    gd.check()
    return {k: v.cpu().numpy() for k, v in res.items() if v is not None}


@pytest.mark.parametrize("P,shift", [(1, s) for s in range(8)] + [(255, 0), (257, 0)])
def test_activations(hip_lib, P, shift):
    """Domain: |q| < 1e18 per component.  sigmoid, exp (expf enters the bound at one ulp) and x / max(|x|, 1e-12) at opacity
    +-0, +-20, +-88, +-104, scales -104, -87, 0, 88, quaternions zero, of norm 1e-13 and 1e-12 (1 +- 2^-20), with one component,
    with components of 1e18; the gradients against the fp64 derivative formed from the DEVICE's own saved outputs"""
    t = fc.activation_inputs(P, shift)
    got = run_activations(t)
    ref = fg.activate_forward(t["opacity"], t["scales"], t["rotations"])
    rb = fg.activate_backward(got["opacity"], got["scales"], t["rotations"], t["g_opacity"], t["g_scales"], t["g_rotations"])
    fails = _record(f"activations-P{P}-s{shift}", fc.worst(got, {**ref, **rb}, ("opacity", "scales", "rotations", "d_opacity", "d_scales", "d_rotations")))
    for s_on, r_on in ((False, False), (True, False), (False, True)):      # scales / rotations NULL in the forward
        part = run_activations(t, scales=s_on, rotations=r_on)
        assert set(part) == {"opacity"} | ({"scales"} if s_on else set()) | ({"rotations"} if r_on else set())
        assert all(fc.same_bits(part[k], got[k]) for k in part)
    for j, name in enumerate(("opacity", "scales", "rotations")):
        on = tuple(i != j for i in range(3))
        no_g = run_activations(t, g=on)          # a NULL gradient is zero
        assert not no_g["d_" + name].any() and all(fc.same_bits(no_g[k], got[k]) for k in got if k != "d_" + name)
        no_d = run_activations(t, d=on)          # a NULL output is not wanted
        assert "d_" + name not in no_d and all(fc.same_bits(no_d[k], got[k]) for k in no_d)
    assert not fails, "; ".join(fails)


def test_activations_no_gaussians(hip_lib):
    gd = Guarded()
    x = [gd.out((16,)) for _ in range(9)]
    call("lara_activate_gaussians_forward", DEV, 0, *x[:6])
    call("lara_activate_gaussians_backward", DEV, 0, *x)
    gd.check()
    assert all(bool(torch.isnan(o).all()) for o in x)


# ---------------------------------------------------------------------------------------------- through the wrappers

def test_wrappers_sample_point_feats(hip_lib):
    """`fine.sample_point_feats` on the exact case (its map gradients are the same bits in any atomic order): gradients requested
    for each subset of {points, image, acc_map, depth}, a non-contiguous `points` and a non-contiguous `depth`: the direct ABI's
    bits"""
    from lara_amd.fine import sample_point_feats
    t = fc.exact_inputs("edges")
    direct = run_sampler(t)
    names = ("points", "image", "acc_map", "depth")
    keys = dict(zip(names, ("d_points", "d_image", "d_acc_map", "d_depth")))
    for mask in range(16):
        for strided in ((False, True) if mask in (0, 15) else (False,)):
            d = {k: _dev(t[k]) for k in names + ("w2c", "ixt", "img_ref")}
            if strided:
                d["points"] = torch.cat([d["points"], d["points"]], 1)[:, :3]
                d["depth"] = torch.cat([d["depth"], d["depth"]], -1)[..., :1]
                assert not d["points"].is_contiguous() and not d["depth"].is_contiguous()
            want = [k for i, k in enumerate(names) if mask >> i & 1]
            for k in want:
                d[k].requires_grad_(True)
            out = sample_point_feats(*(d[k] for k in ("points", "w2c", "ixt", "img_ref", "image", "acc_map", "depth")))
            assert fc.same_bits(out.detach().cpu().numpy(), direct["out"])
            if want:
                grads = torch.autograd.grad((out * _dev(t["g_out"])).sum(), [d[k] for k in want])
                for k, g in zip(want, grads):
                    assert fc.same_bits(g.cpu().numpy(), direct[keys[k]]), (mask, strided, k)


def test_wrappers_surface_maps_and_activations(hip_lib):
    from lara_amd.renderer import activate_gaussians, surface_maps, surface_maps_views
    t = fc.surface_inputs(17, 16, 3, special=True)
    g = fc.surface_grads(t, "all")
    direct = run_surface(t, 0.25, g)
    c, a = _dev(t["color"]).requires_grad_(True), _dev(t["allmap"]).requires_grad_(True)
    outs = surface_maps_views(c, a, _dev(t["rays"]), _dev(t["rots"]).view(3, 3, 3), 0.25)
    sum((o * _dev(g[k])).sum() for k, o in zip(fc.MAP_KEYS, outs)).backward()
    for k, o in zip(fc.MAP_KEYS, outs):
        assert fc.same_bits(o.detach().cpu().numpy(), direct[k]), k
    assert fc.same_bits(c.grad.cpu().numpy(), direct["d_color"]) and fc.same_bits(a.grad.cpu().numpy(), direct["d_allmap"])
    W = 16
    c1, a1 = _dev(t["color"][0]).requires_grad_(True), _dev(t["allmap"][0]).requires_grad_(True)
    outs = surface_maps(c1, a1, _dev(t["rays"][0]), _dev(t["rots"][0]).view(3, 3), 0.25)
    sum((o * _dev(g[k][:, :W])).sum() for k, o in zip(fc.MAP_KEYS, outs)).backward()
    for k, o in zip(fc.MAP_KEYS, outs):
        assert fc.same_bits(o.detach().cpu().numpy(), direct[k][:, :W]), k
    assert fc.same_bits(c1.grad.cpu().numpy(), direct["d_color"][0]) and fc.same_bits(a1.grad.cpu().numpy(), direct["d_allmap"][0])
    t = fc.activation_inputs(257)
    direct = run_activations(t)
    raw = [_dev(t["opacity"])[:, None].requires_grad_(True), _dev(t["scales"]).requires_grad_(True), _dev(t["rotations"]).requires_grad_(True)]
    outs = activate_gaussians(*raw)
    sum((o * _dev(t[k]).view(o.shape)).sum() for o, k in zip(outs, ("g_opacity", "g_scales", "g_rotations"))).backward()
    for o, x, k in zip(outs, raw, ("opacity", "scales", "rotations")):
        assert fc.same_bits(o.detach().cpu().numpy().reshape(direct[k].shape), direct[k]), k
        assert fc.same_bits(x.grad.cpu().numpy().reshape(direct["d_" + k].shape), direct["d_" + k]), k


def test_wrappers_rows(hip_lib):
    from lara_amd.fine import take_rows_multi, voxel_rows_scenes
    c = fc.voxel_rows_case(80)
    vol = _dev(np.stack([c["src"], c["src"][::-1]])).requires_grad_(True)
    vox = [_dev(c["vox"]), _dev(c["vox"][:5])]
    rows = voxel_rows_scenes(vol, vox)
    assert fc.same_bits(rows[0].detach().cpu().numpy(), c["src"][c["vox"]]) and fc.same_bits(rows[1].detach().cpu().numpy(), c["src"][::-1][c["vox"][:5]])
    (rows[0] * _dev(c["g"])).sum().backward()
    _, seq = fg.voxel_rows_backward(c["vox"], c["g"], c["n_vox"])
    assert fc.same_bits(vol.grad[0].cpu().numpy(), seq) and not bool(vol.grad[1].any())
    rng = np.random.default_rng(3)
    idx = _dev(np.sort(rng.permutation(500)[:300]).astype(np.int64))
    xs = [_dev(rng.standard_normal((500, w)).astype(np.float32)).requires_grad_(True) for w in (3, 12, 1, 2, 4)]
    outs = take_rows_multi(xs, idx)
    gs = [torch.randn_like(o) for o in outs]
    sum((o * g).sum() for o, g in zip(outs, gs)).backward()
    for x, o, g in zip(xs, outs, gs):
        assert torch.equal(o, x.detach()[idx]) and torch.equal(x.grad, torch.zeros_like(x).index_copy_(0, idx, g))
