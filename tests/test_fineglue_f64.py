"""The fp64 reference of the point sampler, the surface maps and the activations (oracle/fineglue_f64.py) and the cases built on it
(tests/fineglue_cases.py), without a GPU.  What tests/test_fineglue_f64_gpu.py then holds csrc/pointfeat.hip and csrc/surface.hip
to rests on these:

  - every case meets its stated condition, from the reference alone: the exact-arithmetic cases are exact (an fp32 and an fp64
    evaluation of the projection, and of everything after it, agree bit for bit) and contain every named edge position; the
    general-position cases keep every (view, point) pair 1/16 px from a pixel border and 0.25 from the kink of | s - z |, with
    a propagated position bound below 1/256 px; the ordinary surface pixels have |a x b| >= 1e-3 |a| |b|; the special pixels
    are where they are said to be, three pixels apart; no quaternion's length is within 2^-21 of the 1e-12 threshold;
  - a straightforward fp32 numpy evaluation of the same formulas (mode "f32" of the reference's one statement of them) passes
    every check the device gets.  numpy cannot contract a * b + c to an FMA; the bounds count one rounding per operation, a
    fused operation has one rounding fewer, so they cover both forms -- and in the exact cases no operation rounds at all;
  - the reference agrees with the existing torch restatements (tests/test_pointfeat.py::restated, tests/test_surface.py::restated)
    run in fp64, on the cases without edge samples;
  - the checks bite: each of the twelve defects of `oracle.fineglue_f64.DEFECTS`, built into the fp32 evaluation, fails the case
    named beside it in DEFECT_CASES.

The fp32 stand-in's largest |diff| / limit: sampler 0.16 (d_points, V = 1), surface maps 0.18 (d_allmap), activations 0.21 (scales).
"""
import numpy as np
import pytest
import torch

from oracle import fineglue_f64 as fg
from tests import fineglue_cases as fc

SAMPLER_KEYS = ("out", "d_points") + fc.GRAD_KEYS
SURFACE_KEYS = fc.MAP_KEYS + ("d_color", "d_allmap")


def _passes(res, what):
    bad = {k: v for k, v in res.items() if not v <= 1.0}
    assert not bad, f"{what}: |diff| / limit {bad}"


# ---------------------------------------------------------------------------------------------- the point sampler

@pytest.mark.parametrize("variant", ["edges", "kink"])
def test_exact_cases_are_exact_and_hold_every_edge(variant):
    t = fc.exact_inputs(variant)
    assert t["img_ref"].shape[2] <= 48 and t["img_ref"].shape[3] <= 48 and len(t["points"]) <= 4096
    fc.exact_self_check(t)
    ref = fc.exact_reference(t, fc.pattern_for(t))       # asserts: representable in fp32, and the fp32 evaluation has the same bits
    if variant == "kink":
        pat = fc.pattern_for(t)
        cluster = slice(t["n_edge"], t["n_lattice"])
        assert (ref["resid"][:, cluster] == 0).all(), "the cluster does not sit on the kink in every view"
        assert (ref["out"][:, 7, cluster] == 0).all() and (ref["d_points"][cluster] == 0).all()
        assert np.array_equal(ref["d_depth"][0, 3:5, 2:4], pat["d_depth"][0, 3:5, 2:4]), "the kink passed a gradient to the depth map"
        assert (ref["resid"] != 0).any() and (ref["d_depth"] != pat["d_depth"]).any()        # (border samples are off the kink)


@pytest.mark.parametrize("case", fc.GENERAL_CASES, ids=lambda c: "-".join(map(str, c)))
def test_general_cases_keep_their_margins_and_the_fp32_evaluation_passes(case):
    t = fc.general_case(*case)
    ref = fg.point_feats(t, "f64", pattern=fc.pattern_for(t))
    info = fc.general_self_check(t, ref)
    assert 0 < info["outside"] < info["pairs"], "no point outside every frustum, or none inside"
    _passes(fc.worst(fg.point_feats(t, "f32", pattern=fc.pattern_for(t)), ref, SAMPLER_KEYS), case)


@pytest.mark.parametrize("V,n", fc.LANE_CASES)
def test_lane_cases(V, n):
    t = fc.general_inputs(V, n)
    ref = fg.point_feats(t, "f64")
    fc.general_self_check(t, ref)
    assert ref["out"].shape == (V, 8, n) and ref["d_points"].shape == (n, 3)
    _passes(fc.worst(fg.point_feats(t, "f32"), ref, SAMPLER_KEYS), (V, n))


def test_non_finite_positions_in_the_reference():
    """every tap of a non-finite position is outside: channels 0..6 are 0, channel 7 is |0 - z|, the maps receive nothing from
    that (point, view), and every other point is untouched"""
    t, bad = fc.nonfinite_inputs()
    ref = fg.point_feats(t, "f64")
    x = ref["x"].v
    assert not np.isfinite(x[1, bad[0]]) and np.isfinite(x[[0, 2], bad[0]]).all() and np.isnan(x[:, bad[1]]).all()
    for v, i in ((1, bad[0]), (0, bad[1]), (1, bad[1]), (2, bad[1])):
        assert (ref["out"].v[v, :7, i] == 0).all() and (ref["out"].A[v, :7, i] == 0).all()
    assert ref["out"].v[1, 7, bad[0]] == 0 and np.isnan(ref["out"].v[:, 7, bad[1]]).all()
    keep = np.setdiff1d(np.arange(65), bad)
    clean = dict(t, points=t["points"][keep], g_out=t["g_out"][:, :, keep])
    rc = fg.point_feats(clean, "f64")
    assert np.array_equal(rc["out"].v, ref["out"].v[:, :, keep]) and np.array_equal(rc["d_points"].v, ref["d_points"].v[keep])
    only = dict(t, points=t["points"][[bad[0]]], g_out=t["g_out"][:, :, [bad[0]]])     # the maps: clean run + point 5's views 0 and 2
    ro = fg.point_feats(only, "f64")
    for k in fc.GRAD_KEYS:
        assert np.isfinite(ref[k].v).all()
        assert np.allclose(ref[k].v, rc[k].v + ro[k].v, rtol=0, atol=1e-12)
    assert not ro["d_depth"].v[1].any()
    got = fg.point_feats(t, "f32")
    res = fc.worst({k: got[k] for k in fc.GRAD_KEYS}, ref, fc.GRAD_KEYS)
    res["out"] = float(fg.ratio(got["out"], ref["out"]).max())
    _passes(res, "non-finite")


def test_reference_agrees_with_the_torch_restatement_of_the_sampler():
    from tests.test_pointfeat import restated
    t = fc.general_case("smooth", 4, 1500)
    ref = fg.point_feats(t, "f64")
    d = {k: torch.from_numpy(t[k]).double() for k in ("points", "w2c", "ixt", "img_ref", "image", "acc_map", "depth", "g_out")}
    leaves = {k: d[k].clone().requires_grad_(True) for k in ("points", "image", "acc_map", "depth")}
    feats = restated(leaves["points"], d["w2c"], d["ixt"], d["img_ref"], leaves["image"], leaves["acc_map"], leaves["depth"])
    (feats * d["g_out"]).sum().backward()
    pairs = (("out", feats.detach()), ("d_points", leaves["points"].grad), ("d_image", leaves["image"].grad),
             ("d_acc_map", leaves["acc_map"].grad), ("d_depth", leaves["depth"].grad))
    for k, want in pairs:
        want = want.numpy()
        err = np.abs(ref[k].v - want).max() / (1 + np.abs(want).max())
        assert err <= 1e-9, (k, err)        # (grid_sample's fp64 round trip moves a position by 1e-15 px)


def test_voxel_rows_reference():
    for width in (4, 80):
        c = fc.voxel_rows_case(width)
        vox = c["vox"]
        assert vox[0] == 0 and vox[1] == 0 and vox[-1] == c["n_vox"] - 1 and (np.diff(vox) >= 0).all()
        assert (vox == c["n_vox"] - 1).sum() == 1000 and 7 not in vox and 20 not in vox
        ref, seq = fg.voxel_rows_backward(vox, c["g"], c["n_vox"])
        assert not seq[7].any() and not ref.v[20].any()
        assert float(fg.ratio(seq, ref).max()) <= 1.0


# ---------------------------------------------------------------------------------------------- the surface maps

def _surface_runs(t, ratio, mode="f32", defect=None, whiches=("all",) + fc.MAP_KEYS):
    for which in whiches:
        g = fc.surface_grads(t, which)
        yield which, fg.surface_maps(t, ratio, "f64", grads=g), fg.surface_maps(t, ratio, mode, defect=defect, grads=g)


@pytest.mark.parametrize("H,W,n,ratio", fc.SURFACE_CASES)
def test_surface_cases_and_the_fp32_evaluation(H, W, n, ratio):
    t = fc.surface_inputs(H, W, n)
    for which, ref, got in _surface_runs(t, ratio):
        fc.surface_self_check(t, ref, special=False)
        _passes(fc.worst(got, ref, SURFACE_KEYS), (H, W, n, ratio, which))
        if which not in ("all", "image"):
            assert not got["d_color"].any()


@pytest.mark.parametrize("H,W", fc.SPECIAL_SIZES)
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("ratio", [0.0, 0.25, 1.0])
def test_special_pixels_and_the_fp32_evaluation(H, W, n, ratio):
    t = fc.surface_inputs(H, W, n, special=True)
    for which, ref, got in _surface_runs(t, ratio, whiches=("all", "depth_normal", "depth", "image")):
        fc.surface_self_check(t, ref, special=True)
        _passes(fc.worst(got, ref, SURFACE_KEYS), (H, W, n, ratio, which))
        if which == "depth_normal":        # the clamped branch reaches the gradient: g * 1e12 through cross3, at the patch's arms
            y, x = t["where"][(0, "collinear_patch")]
            arm = ref["d_allmap"].v[0, 5 if ratio else 0, y + 1, x]
            assert abs(arm) > 1e6 and ref["d_allmap"].A[0, 5 if ratio else 0, y + 1, x] < 1e-6 * abs(arm)
            y, x = t["where"][(0, "flat_patch")]
            assert ref["d_allmap"].v[0, :, y, x].tolist() == [0.0] * 7
        if which in ("all", "image"):      # colour exactly 0 and exactly 1 pass the gradient, -2^-149 and 1 + 2^-23 block it
            d = ref["d_color"]
            assert d[0, 0, 0, 0] != 0 and d[0, 1, 0, 1] != 0 and d[0, 2, 0, 2] == 0 and d[0, 0, 0, 3] == 0


def test_reference_agrees_with_the_torch_restatement_of_the_surface_maps():
    from tests.test_surface import restated
    H, W, n = 17, 16, 3
    t = fc.surface_inputs(H, W, n)
    for ratio in (0.0, 0.25, 1.0):
        g = fc.surface_grads(t, "all")
        ref = fg.surface_maps(t, ratio, "f64", grads=g)
        for v in range(n):
            c, a = (torch.from_numpy(t[k][v]).double().requires_grad_(True) for k in ("color", "allmap"))
            out = restated(c, a, torch.from_numpy(t["rays"][v]).double(), torch.from_numpy(t["rots"][v].reshape(3, 3)).double(), ratio)
            loss = 0
            for k in fc.MAP_KEYS:
                mine = fg.val(ref[k])[:, v * W:(v + 1) * W].reshape(out[k].shape)
                assert np.abs(mine - out[k].detach().numpy()).max() <= 1e-12 * (1 + np.abs(mine).max()), k
                loss = loss + (out[k] * torch.from_numpy(g[k][:, v * W:(v + 1) * W].astype(np.float64)).reshape(out[k].shape)).sum()
            loss.backward()
            assert np.array_equal(c.grad.numpy(), ref["d_color"][v])
            want = a.grad.numpy()
            assert np.abs(ref["d_allmap"].v[v] - want).max() <= 1e-10 * (1 + np.abs(want).max())


def test_a_view_border_gradient_stays_in_its_view():
    """a huge g_depth_normal on view 1's border columns leaves d_allmap of views 0 and 2 as they are without it"""
    t = fc.surface_inputs(17, 16, 3)
    g = fc.surface_grads(t, "all")
    huge = {k: (None if v is None else v.copy()) for k, v in g.items()}
    huge["depth_normal"][:, [16, 31]] = 1e30
    zero = {k: (None if v is None else v.copy()) for k, v in g.items()}
    zero["depth_normal"][:, [16, 31]] = 0
    a, b = (fg.surface_maps(t, 0.25, "f32", grads=x)["d_allmap"] for x in (huge, zero))
    assert fc.same_bits(a[[0, 2]], b[[0, 2]]) and fc.same_bits(a[1], b[1])      # (a border pixel has no normal: nowhere at all)
    a = fg.surface_maps(t, 0.25, "f32", defect="stencil_crosses_views", grads=huge)["d_allmap"]
    assert not fc.same_bits(a[[0, 2]], b[[0, 2]])


# ---------------------------------------------------------------------------------------------- the activations

@pytest.mark.parametrize("P,shift", [(1, s) for s in range(8)] + [(255, 0), (257, 0)])
def test_activation_cases_and_the_fp32_evaluation(P, shift):
    """Domain: |q| < 1e18 per component."""
    t = fc.activation_inputs(P, shift)
    ln = fc.activation_self_check(t)
    if P > 8:
        assert (ln == 0).any() and ((ln > 0) & (ln < 5e-13)).any() and (ln > 1e18).any()
        assert set(fc.OPACITIES) <= set(t["opacity"].tolist()) and set(fc.SCALES) <= set(t["scales"].ravel().tolist())
    ref = fg.activate_forward(t["opacity"], t["scales"], t["rotations"])
    got = fg.activate_forward(t["opacity"], t["scales"], t["rotations"], "f32")
    _passes(fc.worst(got, ref, ("opacity", "scales", "rotations")), (P, "forward"))
    args = (got["opacity"], got["scales"], t["rotations"], t["g_opacity"], t["g_scales"], t["g_rotations"])
    _passes(fc.worst(fg.activate_backward(*args, mode="f32"), fg.activate_backward(*args), ("d_opacity", "d_scales", "d_rotations")), (P, "backward"))


# ---------------------------------------------------------------------------------------------- the checks bite

def _exact_defect(variant, defect, keys):
    t = fc.exact_inputs(variant)
    pat = fc.pattern_for(t)
    ref = fc.exact_reference(t, pat)
    got = fg.point_feats(t, "f32", defect=defect, pattern=pat)
    return [k for k in keys if not fc.same_bits(got[k], ref[k])]


def _surface_defect(defect, special, ratio, which="all"):
    t = fc.surface_inputs(17, 16, 3, special=special)
    g = fc.surface_grads(t, which)
    ref = fg.surface_maps(t, ratio, "f64", grads=g)
    res = fc.worst(fg.surface_maps(t, ratio, "f32", defect=defect, grads=g), ref, SURFACE_KEYS)
    return [k for k, v in res.items() if not v <= 1.0]


def _lanes_defect(defect):
    t = fc.general_inputs(3, 65)
    res = fc.worst(fg.point_feats(t, "f32", defect=defect), fg.point_feats(t, "f64"), SAMPLER_KEYS)
    return [k for k, v in res.items() if not v <= 1.0]


def _quaternion_defect(defect):
    t = fc.activation_inputs(255)
    fwd = fg.activate_forward(t["opacity"], t["scales"], t["rotations"], "f32")
    args = (fwd["opacity"], fwd["scales"], t["rotations"], t["g_opacity"], t["g_scales"], t["g_rotations"])
    res = fc.worst(fg.activate_backward(*args, mode="f32", defect=defect), fg.activate_backward(*args), ("d_opacity", "d_scales", "d_rotations"))
    return [k for k, v in res.items() if not v <= 1.0]


DEFECT_CASES = {       # defect -> (the case that catches it, the tensors it must fail -- and no others)
    "tap_clamped_to_border": (lambda d: _exact_defect("edges", d, SAMPLER_KEYS), None),
    "weights_swapped_at_minus_one": (lambda d: _exact_defect("edges", d, SAMPLER_KEYS), None),
    "last_view_dropped": (lambda d: _exact_defect("edges", d, SAMPLER_KEYS) + _lanes_defect(d), ["d_points", "d_points"]),
    "sign_of_zero_is_one": (lambda d: _exact_defect("kink", d, SAMPLER_KEYS), ["d_points", "d_depth"]),
    "scatter_overwrites": (lambda d: _exact_defect("edges", d, SAMPLER_KEYS), list(fc.GRAD_KEYS)),
    "unpack_assigns": (lambda d: _exact_defect("edges", d, SAMPLER_KEYS), list(fc.GRAD_KEYS)),
    "stencil_crosses_views": (lambda d: _surface_defect(d, False, 0.25), ["depth_normal", "d_allmap"]),
    "vjp_sign_flipped": (lambda d: _surface_defect(d, False, 0.25), ["d_allmap"]),
    "neg_inf_to_zero": (lambda d: _surface_defect(d, True, 1.0), None),
    "clamp_excludes_bounds": (lambda d: _surface_defect(d, True, 0.0), ["d_color"]),
    "rot_transposed": (lambda d: _surface_defect(d, False, 0.0), ["d_allmap"]),
    "clamped_quaternion_zero": (_quaternion_defect, ["d_rotations"]),
}


def test_every_defect_has_a_case():
    assert set(DEFECT_CASES) == set(fg.DEFECTS)


@pytest.mark.parametrize("defect", fg.DEFECTS)
def test_a_built_in_defect_is_caught(defect):
    run, expected = DEFECT_CASES[defect]
    failed = run(defect)
    assert failed, f"{defect}: no check noticed"
    if expected is not None:
        assert failed == expected, (defect, failed)
    else:
        assert "out" in failed or "depth" in failed, (defect, failed)
