"""csrc/meshray.hip held to the restatement of its header (tests/meshray_restate.py): `raycast` equal to restated brute force over
all triangles AS INTEGERS on every case of tests/meshray_cases.py -- the bits of t, the face, the bits of the barycentrics, no ray
exempt: both are argmins of the same computed numbers under the same tie rule --, with both sibling orders; `occluded` equal to
face >= 0; 4 096 copies of one triangle; inputs without a candidate; a permuted mesh; `visibility` against the restatement on every
(point, eye) pair outside the ambiguous band; `render_depth` as integers; `depth_scores(self_occlusion=True)` on a double wall, and
the unchanged default routes of `observe` and `depth_scores`; the bench tool at its --quick size."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import depthsurface_cases as DC
from tests import depthsurface_restate as DR
from tests import meshdist_restate as R
from tests import meshray_cases as MC
from tests import meshray_restate as RR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 8 * DR.U                      # the bar of tests/test_depthsurface_gpu.py
AMBIGUOUS_CAP = 0.005


def _dev():
    return torch.device("cuda", 0)


def _t(a, dtype=None):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(_dev(), dtype)          # (a copy: the cases are read-only)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _ibits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


_runs = {}


def _case(key):
    """One device build and one run of every query of the case, shared by the tests."""
    if key not in _runs:
        from lara_amd import meshbvh, meshray
        c = MC.case(key)
        bvh = meshbvh.TriangleBVH(_t(c["V"]), _t(c["F"]))
        rays = (_t(c["o"]), _t(c["d"]), _t(c["t_min"]), _t(c["t_max"]))
        _runs[key] = {"bvh": bvh, "cast": meshray.raycast(bvh, *rays, return_bary=True),
                      "other": meshray.raycast(bvh, *rays, return_bary=True, other_order=True),
                      "plain": meshray.raycast(bvh, *rays), "occluded": meshray.occluded(bvh, *rays)}
    return _runs[key]


@pytest.mark.parametrize("key", sorted(MC.CASES))
def test_raycast_equals_brute_force_as_integers(hip_lib, key):
    c, r = MC.case(key), _case(key)
    for name in ("cast", "other"):
        t, face, bary = (x.cpu().numpy() for x in r[name])
        assert t.dtype == np.float32 and face.dtype == np.int32 and bary.shape == (len(t), 3)
        assert np.array_equal(face, c["face"]), (key, name, int((face != c["face"]).sum()))
        assert np.array_equal(_ibits(t), _ibits(c["t"])), (key, name)
        hit = face >= 0
        assert np.array_equal(_ibits(bary[hit]), _ibits(c["bary"][hit])) and np.isnan(bary[~hit]).all(), (key, name)
        assert np.all(np.isposinf(t[~hit])) and not set(face[hit].tolist()) - set(np.nonzero(R.valid_triangles(c["V"], c["F"]))[0].tolist())
    t, face = r["plain"]
    assert torch.equal(_bits(t), _bits(r["cast"][0])) and torch.equal(face, r["cast"][1])
    kinds = np.arange(len(c["o"])) % 10
    by_kind = [int((c["face"][kinds == k] >= 0).sum()) for k in range(10)]
    print(f"meshray {key}: {int((c['face'] >= 0).sum())} of {len(c['o'])} rays hit; by kind {by_kind}")
    if key == "copies_4096":          # every copy is hit at the same t: the smallest id
        assert (c["hits"] == 4096).sum() > 50 and np.all(c["face"][c["hits"] == 4096] == 0)


@pytest.mark.parametrize("key", sorted(MC.CASES))
def test_occluded_equals_a_first_hit(hip_lib, key):
    c, r = MC.case(key), _case(key)
    assert r["occluded"].dtype == torch.bool and np.array_equal(r["occluded"].cpu().numpy(), c["face"] >= 0)


def test_scalar_windows_and_defaults(hip_lib):
    """Scalars for t_min and t_max equal tensors filled with them; the defaults are [0, +inf)."""
    from lara_amd import meshray
    c, bvh = MC.case("icosphere"), _case("icosphere")["bvh"]
    o, d = _t(c["o"]), _t(c["d"])
    n = len(c["o"])
    for lo, hi in ((0.0, np.inf), (-3.0, 0.75), (0.5, 2.0)):
        ref = RR.brute(c["o"], c["d"], c["V"], c["F"], lo, hi)
        for got in (meshray.raycast(bvh, o, d, lo, hi), meshray.raycast(bvh, o, d, _t(np.full(n, lo, np.float32)), _t(np.full(n, hi, np.float32)))):
            assert np.array_equal(_ibits(got[0].cpu().numpy()), _ibits(ref[0])) and np.array_equal(got[1].cpu().numpy(), ref[1])
        assert np.array_equal(meshray.occluded(bvh, o, d, lo, hi).cpu().numpy(), ref[1] >= 0)
    t, face = meshray.raycast(bvh, o, d)
    assert np.array_equal(face.cpu().numpy(), RR.brute(c["o"], c["d"], c["V"], c["F"])[1])
    t, face = meshray.raycast(bvh, o[:0], d[:0])
    assert t.shape == (0,) and face.shape == (0,) and meshray.occluded(bvh, o[:0], d[:0]).shape == (0,)


def test_meshes_and_rays_without_a_candidate(hip_lib):
    """A mesh with no valid triangle, a mesh of triangles with a coordinate that is not finite, and rays that can never hit (a zero
    direction, a NaN or an infinity in d or o): t = +inf, face = -1, bary = NaN, not occluded, and such a point is seen by no eye /
    such an eye hides nothing."""
    from lara_amd import meshbvh, meshray
    V, F = R.icosphere(1)
    o = _t(np.zeros((4, 3), np.float32))
    d = _t(np.array([[1, 0, 0], [0, 1, 0], [0, 0, -1], [1, 1, 1]], np.float32))
    Vn = V.copy()
    Vn[:, 1] = np.nan
    for bvh in (meshbvh.TriangleBVH(_t(V), _t(np.full((5, 3), len(V) + 1, np.int64))), meshbvh.TriangleBVH(_t(Vn), _t(F))):
        t, face, bary = meshray.raycast(bvh, o, d, return_bary=True)
        assert bool(torch.isposinf(t).all()) and bool((face == -1).all()) and bool(torch.isnan(bary).all())
        assert not bool(meshray.occluded(bvh, o, d).any())
        assert meshray.visibility(bvh, d, o[:2]).cpu().tolist() == [3, 3, 3, 3]
    bvh = meshbvh.TriangleBVH(_t(V), _t(F))
    oo = np.zeros((6, 3), np.float32)
    dd = np.array([[0, 0, 0], [np.nan, 1, 0], [1, np.inf, 0], [1, 0, 0], [1, 0, 0], [1, 0, 0]], np.float32)
    oo[3, 2], oo[4, 0] = np.nan, -np.inf
    t, face, bary = meshray.raycast(bvh, _t(oo), _t(dd), return_bary=True)
    assert face.cpu().tolist()[:5] == [-1] * 5 and face[5].item() >= 0 and bool(torch.isposinf(t[:5]).all()) and bool(torch.isnan(bary[:5]).all())
    assert meshray.occluded(bvh, _t(oo), _t(dd)).cpu().tolist() == [False] * 5 + [True]
    P = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, 0], [3, 0, 0]], np.float32)
    eyes = np.array([[0, 0, 0], [np.nan, 0, 0], [-3, 0, 0]], np.float32)
    seen = meshray.visibility(bvh, _t(P), _t(eyes)).cpu().tolist()
    assert seen[:2] == [0, 0] and seen[2] == 0b011 and seen[3] == 0b010          # (3, 0, 0) is hidden from the centre and from (-3, 0, 0)
    with pytest.raises(ValueError):
        meshray.visibility(bvh, _t(P), _t(np.zeros((65, 3), np.float32)))
    with pytest.raises(ValueError):
        meshray.visibility(bvh, _t(P), _t(eyes), shrink=1.0)


def test_a_permuted_mesh_gives_the_same_t_bits(hip_lib):
    """The triangles in another order: another tree, the same t bit for bit; the face follows the permutation except where the
    minimum is not unique."""
    from lara_amd import meshbvh, meshray
    c, r = MC.case("sphere_square"), _case("sphere_square")
    perm = np.random.default_rng(43).permutation(len(c["F"]))
    bvh = meshbvh.TriangleBVH(_t(c["V"]), _t(c["F"][perm]))
    t, face = meshray.raycast(bvh, _t(c["o"]), _t(c["d"]), _t(c["t_min"]), _t(c["t_max"]))
    assert torch.equal(_bits(t), _bits(r["cast"][0]))
    face = face.cpu().numpy()
    hit = face >= 0
    assert np.array_equal(hit, c["face"] >= 0)
    back = perm[face[hit]]
    moved = np.nonzero(hit)[0][back != c["face"][hit]]
    if len(moved):
        t_all = RR.all_hits(c["o"][moved], c["d"][moved], c["V"], c["F"], c["t_min"][moved], c["t_max"][moved])[0]
        k = np.arange(len(moved))
        assert np.all(t_all[k, perm[face[moved]]] == t_all[k, c["face"][moved]])
    again = meshray.raycast(bvh, _t(c["o"]), _t(c["d"]), _t(c["t_min"]), _t(c["t_max"]))
    assert torch.equal(_bits(again[0]), _bits(t)) and np.array_equal(again[1].cpu().numpy(), face)


@pytest.mark.parametrize("name", sorted(MC.visibility_cases()))
def test_visibility_equals_the_restatement(hip_lib, name):
    """Every (point, eye) pair outside the ambiguous band -- a hit within a relative 2^-18 of the 1 - shrink cut --, and at most
    0.5 % of the pairs inside it."""
    from lara_amd import meshbvh, meshray
    V, F, P, skip, eyes, shrink = MC.visibility_cases()[name]
    bvh = meshbvh.TriangleBVH(_t(V), _t(F))
    seen = meshray.visibility(bvh, _t(P), _t(eyes), _t(skip), shrink)
    assert seen.dtype == torch.int64 and seen.shape == (len(P),)
    got = DR.bits(seen.cpu().numpy(), len(eyes))
    ref, amb = RR.visibility(P, eyes, V, F, skip, shrink)
    want = DR.bits(ref, len(eyes))
    differ = got != want
    print(f"meshray visibility {name}: {differ.size} pairs, {int(amb.sum())} ambiguous, {int(differ.sum())} differ, {int(want.sum())} visible")
    assert amb.mean() <= AMBIGUOUS_CAP and not np.any(differ & ~amb)
    assert torch.equal(seen, meshray.visibility(bvh, _t(P), _t(eyes), _t(skip), shrink))
    if skip is not None:          # the skipped face matters once nothing is shrunk away: a sample ON the mesh meets its own triangle at t ~ 1
        seen0 = meshray.visibility(bvh, _t(P), _t(eyes), _t(skip), 0.0)
        assert not torch.equal(seen0, meshray.visibility(bvh, _t(P), _t(eyes), None, 0.0))
        ref0 = RR.visibility(P, eyes, V, F, skip, 0.0)
        assert not np.any((DR.bits(seen0.cpu().numpy(), len(eyes)) != DR.bits(ref0[0], len(eyes))) & ~ref0[1])


def test_render_depth_equals_the_restatement_as_integers(hip_lib):
    """The four 24 x 32 cameras of `sphere4` on the icosphere: the rays torch makes equal the restated ones bit for bit, depth and
    face equal restated brute force; the depth is the analytic sphere's but for the icosphere's sagitta."""
    from lara_amd import depthsurface, meshbvh, meshray
    c = DC.sphere4()
    V, F = R.icosphere(3, DC.RADIUS)
    bvh = meshbvh.TriangleBVH(_t(V), _t(F))
    k, pose = depthsurface.cameras(c["ixt"], c["c2w"])
    o, d = RR.pixel_rays(k, pose, 24, 32)
    go, gd = meshray.pixel_rays(c["ixt"], c["c2w"], 24, 32, _dev())
    assert np.array_equal(_ibits(go.cpu().numpy()), _ibits(o)) and np.array_equal(_ibits(gd.cpu().numpy()), _ibits(d))
    depth, face = meshray.render_depth(bvh, c["ixt"], c["c2w"], 24, 32)
    assert depth.shape == face.shape == (4, 24, 32) and depth.dtype == torch.float32 and face.dtype == torch.int32
    t, f = RR.brute(o.reshape(-1, 3), d.reshape(-1, 3), V, F)[:2]
    want = np.where(f >= 0, t, np.float32(0)).reshape(4, 24, 32)
    assert np.array_equal(_ibits(depth.cpu().numpy()), _ibits(want)) and np.array_equal(face.cpu().numpy(), f.reshape(4, 24, 32))
    both = (c["mask"] != 0) & (want > 0)
    assert both.sum() > 1200 and np.quantile(np.abs(want - c["depth"])[both], 0.9) < 0.01 and ((c["mask"] != 0) ^ (want > 0)).mean() < 0.05


_wall = {}


def _double_wall():
    """The unit sphere seen by the four cameras of `sphere4`, and as the prediction that sphere plus a concentric one of radius
    0.97: (views, pred, numpy V, F)."""
    if not _wall:
        c = DC.sphere4()
        depth, mask, _ = DC.raycast_spheres(c["c2w"], c["ixt"], 24, 32, radii=(1.0,))
        Va, Fa = DC.uv_sphere(1.0, 12, 24)
        Vb, Fb = DC.uv_sphere(0.97, 12, 24)
        V, F = np.concatenate([Va, Vb]), np.concatenate([Fa, Fb + len(Va)])
        _wall.update(views=(depth, mask, c["ixt"], c["c2w"]), V=V, F=F, outer=len(Fa))
    return _wall


def test_self_occlusion_on_a_double_wall(hip_lib):
    """tau = 0.05: the inner wall lies 0.03 behind the seen one, so by the depth rule its near side counts as observed; with
    ``self_occlusion`` it is hidden by the outer wall.  n_pred_self_occluded equals the restated count, n_pred_observed drops by
    exactly that, the accuracy is the float64 mean over the samples that remain; everything else in the dict is unchanged."""
    from lara_amd import depthsurface, meshmetrics
    w = _double_wall()
    depth, mask, ixt, c2w = w["views"]
    views = (_t(depth), _t(mask), ixt, c2w)
    pred = (_t(w["V"]), _t(w["F"]))
    n, tau = 1024, 0.05
    kw = dict(n=n, tau=tau, thresholds=(0.01, 0.02, 0.05), return_samples=True)
    plain = depthsurface.depth_scores(pred, *views, **kw)
    again = depthsurface.depth_scores(pred, *views, self_occlusion=False, **kw)
    got = depthsurface.depth_scores(pred, *views, self_occlusion=True, **kw)
    assert "n_pred_self_occluded" not in plain and set(plain) == set(again) and set(got) == set(plain) | {"n_pred_self_occluded"}
    assert all(plain[k] == again[k] for k in plain if k != "samples")
    assert all(torch.equal(a, b) for a, b in zip(plain["samples"], again["samples"]))
    P, _, _, _, d_p, _, _, _, seen0 = plain["samples"]
    assert all(torch.equal(a, b) for a, b in zip(plain["samples"][:8], got["samples"][:8]))          # the same points and distances
    faces = meshmetrics.sample_surface(*pred, n, 0)[2].cpu().numpy()
    inner = faces >= w["outer"]
    seen0 = seen0.cpu().numpy()
    assert (inner & (seen0 != 0)).sum() > 0.1 * inner.sum() > 0.04 * n          # the inner wall's near side counts today (the images show a cap)
    eyes = np.asarray(c2w, np.float32)[:, :3, 3]
    vis, amb = RR.visibility(P.cpu().numpy(), eyes, w["V"], w["F"], faces)
    hidden = (seen0 != 0) & ((seen0 & vis) == 0)
    print(f"meshray double wall: {int((seen0 != 0).sum())} of {n} samples observed by the depth rule, {int(hidden.sum())} of them "
          f"hidden by the mesh ({int((hidden & inner).sum())} on the inner wall); {int(amb.sum())} ambiguous pairs; "
          f"accuracy {plain['accuracy']:.5f} -> {got['accuracy']:.5f}")
    assert got["n_pred_self_occluded"] == int(hidden.sum()) > 0
    assert got["n_pred_observed"] == plain["n_pred_observed"] - got["n_pred_self_occluded"]
    assert got["n_pred_unobserved"] == n - got["n_pred_observed"]
    assert np.array_equal(got["samples"][8].cpu().numpy(), seen0 & vis)
    assert not np.any(inner & ((seen0 & vis) != 0)) and (hidden & inner).sum() == (inner & (seen0 != 0)).sum()          # none of the inner stays
    acc = d_p.cpu().numpy().astype(np.float64)[(seen0 & vis) != 0].mean()
    assert abs(got["accuracy"] - acc) <= BAR * acc and got["accuracy"] < plain["accuracy"]
    for k in ("completeness", "recall", "n_gt", "n_gt_raw", "n_pred", "tau", "fallbacks"):
        assert got[k] == plain[k], k
    tri = depthsurface.depth_scores(pred, *views, self_occlusion=True, distance="triangle", **kw)
    assert tri["n_pred_self_occluded"] == got["n_pred_self_occluded"] and tri["accuracy"] == got["accuracy"]
    assert tri["distance"] == "triangle"
    with pytest.raises(ValueError, match="self_occlusion needs a prediction that is a mesh"):
        depthsurface.depth_scores(P, *views, self_occlusion=True, n=n, tau=tau)


def test_observe_with_and_without_an_occluder(hip_lib):
    """Without an occluder `observe` returns the library's bits as before (the float64 restatement outside its ambiguous pairs);
    with one, those bits AND `visibility`'s."""
    from lara_amd import depthsurface, meshbvh, meshmetrics, meshray
    w = _double_wall()
    depth, mask, ixt, c2w = w["views"]
    views = (_t(depth), _t(mask), ixt, c2w)
    P, _, faces = meshmetrics.sample_surface(_t(w["V"]), _t(w["F"]), 1024, 0)
    plain = depthsurface.observe(P, *views, 0.05)
    assert torch.equal(plain, depthsurface.observe(P, *views, 0.05, True, depth_max=None, occluder=None))
    k, w2c = DR.cameras(ixt, c2w, invert=True)
    ref, amb = DR.observe(P.cpu().numpy(), depth, mask, k, w2c, 0.05)
    assert not np.any((DR.bits(plain.cpu().numpy(), 4) != DR.bits(ref, 4)) & ~amb)
    bvh = meshbvh.TriangleBVH(_t(w["V"]), _t(w["F"]))
    eyes = torch.as_tensor(c2w).to(_dev(), torch.float32)[:, :3, 3]
    for shrink in (2.0 ** -10, 0.25):
        got = depthsurface.observe(P, *views, 0.05, occluder=bvh, occluder_faces=faces, shrink=shrink)
        assert torch.equal(got, plain & meshray.visibility(bvh, P, eyes, faces, shrink))
    assert not torch.equal(depthsurface.observe(P, *views, 0.05, occluder=bvh, occluder_faces=faces), plain)


def test_the_default_route_of_depth_scores_does_not_import_meshray(hip_lib):
    import lara_amd
    from lara_amd import depthsurface
    w = _double_wall()
    depth, mask, ixt, c2w = w["views"]
    saved = {m: sys.modules.pop("lara_amd." + m, None) for m in ("meshray", "meshbvh")}
    for m in saved:
        vars(lara_amd).pop(m, None)
    try:
        for kw in ({}, {"self_occlusion": False}):
            out = depthsurface.depth_scores((_t(w["V"]), _t(w["F"])), _t(depth), _t(mask), ixt, c2w, n=256, tau=0.05, **kw)
            assert "lara_amd.meshray" not in sys.modules and "lara_amd.meshbvh" not in sys.modules and "n_pred_self_occluded" not in out
        depthsurface.depth_scores((_t(w["V"]), _t(w["F"])), _t(depth), _t(mask), ixt, c2w, n=256, tau=0.05, self_occlusion=True)
        assert "lara_amd.meshray" in sys.modules
    finally:
        for m, mod in saved.items():
            if mod is not None:
                sys.modules["lara_amd." + m] = mod
                setattr(lara_amd, m, mod)


def test_bench_tool_runs_at_its_quick_size(hip_lib, tmp_path):
    out = tmp_path / "bench.json"
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "meshray_bench.py"), "--quick", "--out", str(out)],
                         capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    res = json.loads(out.read_text())
    assert json.loads(run.stdout.strip().splitlines()[-1]) == res
    assert res["T"] <= 20000 and res["rays"] == 8 * 128 * 128 and res["copy_rate_GBps"] > 0
    assert res["both_orders_same_bits"] and res["any_hit_equals_first_hit"] and 0.0 < res["hit_share"] <= 1.0
    assert set(res["first_hit_ms"]) == {"sign_mask", "stored"} and all(v > 0 for v in res["first_hit_ms"].values())
    assert res["any_hit_ms"] > 0 and res["visibility"]["ms"] > 0 and 0.0 < res["visibility"]["visible_share_of_pairs"] < 1.0
    assert res["context_meshrender_depth_ms"] > 0 and res["context_torch_64_rays"]["same_faces"]
