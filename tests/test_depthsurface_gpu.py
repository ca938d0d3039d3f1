"""csrc/depthsurface.hip held to the numpy restatements of its header (tests/depthsurface_restate.py) on the cases of
tests/depthsurface_cases.py.  Exact throughout: the compaction order, the validity rule, the thinning winners, and the observation
bits outside the ambiguous set.

Bars (u = 2^-24).  Points: bit-equal to the fp32 restatement (the header fixes every operation), and within 8 u S of the float64
values of the same formula on the same fp32 inputs, S the sum of the four magnitudes a coordinate adds: two roundings in a (b),
one in a d, one per product with R, one per addition give 4 u (|R0 px| + |R1 py|) + u |R2 d| + 3 u S <= 7 u S to first order.
Normals: within 8 u of the float64 normals.  The depth-derived normal is DEFINED on the fp32 points ("computed in double from the
fp32 points"), so its float64 reference is that formula in float64 on the restated fp32 points -- which the first test holds
bit-equal to the device's; what is left is the rounding of a double quotient to fp32, u / 2 per component.  Reduction: sums of
doubles of non-negative terms, 8 u relative (the bars of tests/test_meshmetrics_gpu.py); counts exact.  Observation: equal to the
float64 restatement on every pair that is not ambiguous (a comparison within 2^-18 of its magnitudes; an fp32 evaluation errs by
a few u of them), and the ambiguous share at most 0.5 %.

Measured on an MI355X (worst |difference| / bar; the tests print them and write test_out/depthsurface_parity.txt, kept as
profiles/depthsurface_parity.txt): points 0.26, normals 0.06 in both modes, reduction sums 0.00; at most 0.098 % of a case's pairs
ambiguous (0.20 of the cap) and no pair, ambiguous or not, differed from float64."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import depthsurface_cases as C
from tests import depthsurface_restate as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 8 * R.U
AMBIGUOUS_CAP = 0.005
_worst = {}


def _note(key, ratio):
    _worst[key] = max(_worst.get(key, 0.0), float(ratio))
    out = os.path.join(ROOT, "test_out")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "depthsurface_parity.txt"), "w") as f:
        f.write("worst observed |difference| / bar of tests/test_depthsurface_gpu.py (bar = 1 fails; a share: of its 0.5 % cap)\n")
        for k in sorted(_worst):
            f.write(f"{k}: {_worst[k]:.4f}\n")
    print(f"depthsurface parity {key}: {ratio:.4f} of the bar")


def _dev():
    return torch.device("cuda", 0)


def _t(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(_dev(), dtype)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _mask(c, kind):
    return None if c["mask"] is None else C.mask_as(c["mask"], kind)


# ---- back-projection ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stride", [1, 2, 3])
@pytest.mark.parametrize("kind", ["uint8", "bool", "float32"])
@pytest.mark.parametrize("key", sorted(C.BACKPROJECT_CASES))
def test_backprojection_order_points_and_reproducibility(hip_lib, key, kind, stride):
    from lara_amd import depthsurface
    c = C.BACKPROJECT_CASES[key]()
    mask = _mask(c, kind)
    dmax = c.get("depth_max")
    k, pose = R.cameras(c["ixt"], c["c2w"])
    ref = R.backproject(c["depth"], mask, k, pose, stride, np.inf if dmax is None else dmax)
    run = lambda: depthsurface.backproject(_t(c["depth"]), _t(mask), c["ixt"], c["c2w"], stride=stride, depth_max=dmax)
    pts, nrm, pix = run()
    assert nrm is None and pts.shape == (len(ref["pixel"]), 3) and pts.dtype == torch.float32 and pix.dtype == torch.int32
    assert np.array_equal(pix.cpu().numpy().astype(np.int64), ref["pixel"])
    got = pts.cpu().numpy()
    assert np.array_equal(got.view(np.int32), ref["points32"].view(np.int32))
    diff = np.abs(got.astype(np.float64) - ref["points64"])
    assert np.all(diff <= BAR * ref["mag"])
    _note("points", (diff / np.where(ref["mag"] > 0, BAR * ref["mag"], 1.0)).max() if len(diff) else 0.0)
    pts2, _, pix2 = run()
    assert torch.equal(_bits(pts), _bits(pts2)) and torch.equal(pix, pix2)


NORMAL_CASES = [("sphere4", 0.05), ("sphere4", None), ("stride", None), ("edges_256", None), ("edges_256", 0.3), ("single", None)]


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("key,jump", NORMAL_CASES)
def test_backprojection_normals(hip_lib, key, jump, stride):
    from lara_amd import depthsurface
    c = C.BACKPROJECT_CASES[key]()
    dmax = c.get("depth_max")
    k, pose = R.cameras(c["ixt"], c["c2w"])
    args = (_t(c["depth"]), _t(c["mask"]), c["ixt"], c["c2w"])
    # from the depth
    ref = R.backproject(c["depth"], c["mask"], k, pose, stride, np.inf if dmax is None else dmax, "depth", np.inf if jump is None else jump)
    pts, nrm, pix = depthsurface.backproject(*args, stride=stride, depth_max=dmax, normals="depth", jump=jump)
    got = nrm.cpu().numpy()
    assert np.array_equal(pix.cpu().numpy().astype(np.int64), ref["pixel"])
    assert np.array_equal(pts.cpu().numpy().view(np.int32), ref["points32"].view(np.int32))
    assert np.all(got[~ref["applies"]] == 0) and np.all(np.any(got[ref["applies"]] != 0, axis=1))
    ratio = np.abs(got.astype(np.float64) - ref["normals"]).max() / BAR if len(got) else 0.0
    _note("normals from depth", ratio)
    assert ratio <= 1.0
    if key == "sphere4":
        assert ref["applies"].sum() > (800 if stride == 1 else 180)
    nrm2 = depthsurface.backproject(*args, stride=stride, depth_max=dmax, normals="depth", jump=jump)[1]
    assert torch.equal(_bits(nrm), _bits(nrm2))
    # given: the analytic map (sphere4) or a seeded one, with zero, NaN and infinite vectors among the valid pixels
    g = np.random.default_rng(3)
    nmap = c["normal_map"].copy() if "normal_map" in c else g.normal(size=c["depth"].shape + (3,)).astype(np.float32)
    flat = nmap.reshape(-1, 3)
    sel = ref["pixel"]
    if len(sel) >= 4:
        flat[sel[0]] = 0.0
        flat[sel[1], 1] = np.nan
        flat[sel[2], 2] = np.inf
        flat[sel[3]] = [3e-30, -4e-30, 0.0]          # tiny: the squares survive in double
    refg = R.backproject(c["depth"], c["mask"], k, pose, stride, np.inf if dmax is None else dmax, nmap)
    gotg = depthsurface.backproject(*args, stride=stride, depth_max=dmax, normals=_t(nmap))[1].cpu().numpy()
    if len(sel) >= 4:
        assert np.all(gotg[:3] == 0) and abs(np.linalg.norm(gotg[3].astype(np.float64)) - 1.0) < 1e-6
    ratio = np.abs(gotg.astype(np.float64) - refg["normals"]).max() / BAR if len(gotg) else 0.0
    _note("normals given", ratio)
    assert ratio <= 1.0


# ---- thinning -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["sphere4", "copies", "single", "one_cell", "nan_rows"])
def test_thin_keeps_the_smallest_index_of_every_cell(hip_lib, name):
    from lara_amd import depthsurface
    P, voxel = C.thin_sets()[name]
    Nn = np.random.default_rng(9).normal(size=P.shape).astype(np.float32)
    kept_ref, dropped_ref = R.thin(P, voxel)
    cap = depthsurface.MAX_CELLS if name == "sphere4" else 1 << 13          # (17^3 = 4913 cells at most here)
    p, n = _t(P), _t(Nn)
    out_p, out_n, kept, dropped = depthsurface.thin(p, n, voxel, max_cells=cap, return_dropped=True)
    assert dropped == dropped_ref and kept.dtype == torch.int32
    assert np.array_equal(kept.cpu().numpy().astype(np.int64), kept_ref)
    assert np.array_equal(out_p.cpu().numpy().view(np.int32), P[kept_ref].view(np.int32))
    assert np.array_equal(out_n.cpu().numpy().view(np.int32), Nn[kept_ref].view(np.int32))
    again = depthsurface.thin(p, n, voxel, max_cells=cap)
    assert torch.equal(again[2], kept) and torch.equal(_bits(again[0]), _bits(out_p)) and torch.equal(_bits(again[1]), _bits(out_n))
    bare = depthsurface.thin(p, None, voxel, max_cells=cap)
    assert bare[1] is None and torch.equal(bare[2], kept)
    if name == "sphere4":          # a grid that does not fit the room given is refused, one that just fits is not
        cells = int(np.prod(np.floor(np.ptp(P, axis=0) / np.float32(voxel)) + 1))
        with pytest.raises(ValueError, match="cells"):
            depthsurface.thin(p, None, voxel, max_cells=cells - 1)
        assert torch.equal(depthsurface.thin(p, None, voxel, max_cells=cells)[2], kept)
        empty = depthsurface.thin(p[:0], None, voxel, max_cells=64)
        assert empty[0].shape == (0, 3) and empty[2].shape == (0,)


# ---- observation --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("free", [True, False])
@pytest.mark.parametrize("n", C.QUERY_SIZES + ("special",))
def test_observation_equals_float64_outside_the_ambiguous_set(hip_lib, n, free):
    from lara_amd import depthsurface
    c = C.sphere4()
    k, w2c = R.cameras(c["ixt"], c["c2w"], invert=True)
    Q = C.queries_special() if n == "special" else C.queries(n)
    want, amb = R.observe(Q, c["depth"], c["mask"], k, w2c, C.TAU, free)
    seen = depthsurface.observe(_t(Q), _t(c["depth"]), _t(c["mask"]), c["ixt"], c["c2w"], C.TAU, free)
    assert seen.dtype == torch.int64 and seen.shape == (len(Q),)
    got = seen.cpu().numpy()
    assert np.all((got >> 4) == 0)
    differ = R.bits(got, 4) != R.bits(want, 4)
    share = amb.mean()
    print(f"depthsurface observe n={n} free={free}: {int(amb.sum())} of {amb.size} pairs ambiguous ({100 * share:.3f} %), "
          f"{int(differ.sum())} differ, {100 * (got != 0).mean():.1f} % of the samples observed")
    _note("observe ambiguous share", share / AMBIGUOUS_CAP)
    assert share <= AMBIGUOUS_CAP
    assert not (differ & ~amb).any()
    if n == "special":
        assert np.all(got[~np.isfinite(Q).all(axis=1)] == 0)
    # a float32 mask and the mask's other spellings see the same
    for kind in ("bool", "float32"):
        other = depthsurface.observe(_t(Q), _t(c["depth"]), _t(C.mask_as(c["mask"], kind)), c["ixt"], c["c2w"], C.TAU, free)
        assert torch.equal(other, seen)


# ---- reduction ----------------------------------------------------------------------------------------------------------------

THR = (0.01, 0.02, 0.03, 0.05)


def _reduce(N, M, dist, index, keep, nq, nt, thr=THR):
    from lara_amd import _native, depthsurface
    row = torch.full((depthsurface.ROW,), -1.0, dtype=torch.float64, device=_dev())
    if N == 0:          # (an empty tensor has no address: the normals come as a pair or not at all)
        nq = nt = None
    ws = _native.alloc_bytes(max(_native.query("lara_depthsurface_reduce_workspace_bytes", N), 256), _dev())
    _native.call("lara_depthsurface_reduce", _dev(), N, M, _t(dist), _t(index), _t(keep), _t(nq), _t(nt), len(thr),
                 _native.host_array("f", list(thr)), row, ws)
    return row.cpu().numpy()


@pytest.mark.parametrize("N", [0, 1, 255, 256, 257, 4096])
def test_reduce_equals_float64_sums_and_exact_counts(hip_lib, N):
    from lara_amd import _native, meshmetrics
    g = np.random.default_rng(40 + N)
    M = 300
    dist = (g.random(N) * 0.06).astype(np.float32)
    dist[: N // 7] = np.float32(0.02)          # ties with a threshold
    index = g.integers(0, M, N).astype(np.int32)
    index[N // 2: N // 2 + 3] = [-1, M, M + 5][: max(0, min(3, N - N // 2))]
    keep = (g.random(N) < 0.6).astype(np.uint8)
    nq, nt = g.normal(size=(N, 3)).astype(np.float32), g.normal(size=(M, 3)).astype(np.float32)
    nq[::5] = 0.0
    nq[1::5, :2] = 0.0          # one non-zero component is a non-zero normal
    nt[::7] = 0.0
    for kp, a, b in ((keep, nq, nt), (None, nq, nt), (keep, None, None), (np.zeros(N, np.uint8), nq, nt)):
        got = _reduce(N, M, dist, index, kp, a, b)
        ref = R.reduce_row(dist, index, M, kp, a, b, THR)
        assert np.array_equal(got[[0, 4, 5, 6, 7, 8]], ref[[0, 4, 5, 6, 7, 8]]) and np.all(got[9:] == 0)
        for j in (1, 2, 3):
            ratio = abs(got[j] - ref[j]) / (BAR * ref[j]) if ref[j] != 0 else float(got[j] != 0)
            _note("reduce sums", ratio)
            assert ratio <= 1.0
    # keep all ones, every normal non-zero: lara_meshmetrics_reduce's numbers, bit for bit
    index = g.integers(0, M, N).astype(np.int32)
    nq, nt = np.abs(nq) + 1.0, np.abs(nt) + 1.0
    got = _reduce(N, M, dist, index, np.ones(N, np.uint8), nq, nt)
    row = torch.zeros(meshmetrics.ROW, dtype=torch.float64, device=_dev())
    ws = _native.alloc_bytes(max(_native.query("lara_meshmetrics_reduce_workspace_bytes", N), 256), _dev())
    _native.call("lara_meshmetrics_reduce", _dev(), N, M, _t(dist), _t(index), *((None, None) if N == 0 else (_t(nq), _t(nt))),
                 len(THR), _native.host_array("f", list(THR)), row, ws)
    mm = row.cpu().numpy()
    assert got[0] == mm[0] == N and got[4] == N
    assert np.array_equal(got[[1, 2, 3]].view(np.int64), mm[[1, 2, 3]].view(np.int64)) and np.array_equal(got[5:9], mm[4:8])


# ---- what the feature is for --------------------------------------------------------------------------------------------------

def test_unobserved_surface_is_not_charged(hip_lib):
    """A sphere of radius 0.5 with a sphere of radius 0.3 inside it that no view can see, against the four views of `sphere4`."""
    from lara_amd import depthsurface, meshmetrics
    c = C.sphere4()
    V, F, inner_share = C.nested_spheres()
    pred = (_t(V), _t(F))
    views = (_t(c["depth"]), _t(c["mask"]), c["ixt"], c["c2w"])
    n = 8192
    out = depthsurface.depth_scores(pred, *views, n=n, return_samples=True)
    G, Gn, _ = depthsurface.backproject(*views, normals="depth")
    plain = meshmetrics.surface_scores(pred, (G, Gn), n=n)
    P, Pn, Gs, Gsn, d_p, i_p, d_g, i_g, seen = out["samples"]
    assert torch.equal(_bits(Gs), _bits(G)) and out["n_gt"] == out["n_gt_raw"] == G.shape[0] == plain["n_gt"]
    assert out["n_pred"] == n and out["n_pred_observed"] + out["n_pred_unobserved"] == n
    assert out["n_pred_observed"] == int((seen != 0).sum()) and out["tau"] == max(meshmetrics.THRESHOLDS) and out["voxel"] is None
    share = out["n_pred_unobserved"] / out["n_pred"]
    print(f"depthsurface: {100 * share:.1f} % of the samples unobserved; accuracy {out['accuracy']:.5f} masked, {plain['accuracy']:.5f} unmasked; "
          f"completeness {out['completeness']:.6f}")
    assert share >= inner_share
    inner = torch.linalg.norm(P, dim=1) < 0.4
    assert not bool((seen[inner] != 0).any()) and 0.2 < float(inner.float().mean()) < 0.33
    assert out["accuracy"] < 0.5 * plain["accuracy"]
    ratio = abs(out["completeness"] - plain["completeness"]) / (BAR * plain["completeness"])
    _note("completeness against surface_scores", ratio)
    assert ratio <= 1.0 and out["recall"] == plain["recall"]
    # the masked accuracy is the mean over the observed samples, in float64
    keep = (seen != 0).cpu().numpy()
    acc = d_p.cpu().numpy().astype(np.float64)[keep].mean()
    assert abs(out["accuracy"] - acc) <= BAR * acc
    assert out["normal_consistency"] is not None and 0 < out["normal_pairs"] <= out["n_pred_observed"] + out["n_gt"]
    # thinning: fewer ground-truth points, the same keys
    thinned = depthsurface.depth_scores(pred, *views, n=n, voxel=1.0 / 16)
    assert thinned["n_gt"] == len(R.thin(G.cpu().numpy(), 1.0 / 16)[0]) < thinned["n_gt_raw"] == out["n_gt_raw"] and thinned["voxel"] == 1.0 / 16
    assert set(thinned) == set(out) - {"samples"}
    # a blob of samples between camera 0 and its background: seen free space, or nothing, by background_is_free
    k0, pose0 = R.cameras(c["ixt"], c["c2w"])
    free_depth = np.zeros_like(c["depth"])
    free_depth[0, 2:5, 3:7] = 1.0          # (a corner of view 0's image, far from the sphere's silhouette)
    assert not c["mask"][0, 1:6, 2:8].any()
    blob = R.backproject(free_depth, None, k0, pose0)["points32"]
    for free, want in ((True, 1), (False, 0)):
        s = depthsurface.observe(_t(blob), *views, 0.01, free)
        assert bool(((s & 1) == want).all()), (free, s)


def test_bench_tool_runs_at_its_quick_size(hip_lib, tmp_path):
    out = tmp_path / "bench.json"
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "depthsurface_bench.py"), "--quick", "--out", str(out)],
                         capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    res = json.loads(out.read_text())
    assert json.loads(run.stdout.strip().splitlines()[-1]) == res
    assert res["views"] == 8 and res["n_gt_raw"] > 0 and res["copy_rate_GBps"] > 0
    (size,) = res["sizes"]
    assert size["samples"] <= 20000 and size["hip_ms"]["whole"] > 0 and size["torch_ms"]["whole"] > 0
    assert 0.0 < size["unobserved_share"] < 1.0
    assert size["torch_agrees"] is True
