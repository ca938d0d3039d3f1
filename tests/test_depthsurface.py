"""include/lara_depthsurface.h: its constants held to the module's, the two numpy restatements
(tests/depthsurface_restate.py: fp32 in the written order, float64 true values) held to each other on every case of
tests/depthsurface_cases.py, the cap on the ambiguous share of the observation cases, the library's refusals, and the score dict on
its way through the Evaluator -- no GPU.  tests/test_depthsurface_gpu.py holds the kernels to the restatements.

Bars (u = 2^-24).  A back-projected coordinate takes two roundings for a (b), one for a d, one for each product with R and one
for each of the three additions: first order 4 u (|R0 px| + |R1 py|) + u |R2 d| + u (|s1| + |s2| + |s3|) <= 7 u S with S the sum of
the four magnitudes added; the bar is 8 u S.  The observation bits of the two restatements must agree outside the ambiguous set."""
import numpy as np
import pytest
import torch

from lara_amd import depthsurface, evaluate
from tests import depthsurface_cases as C
from tests import depthsurface_restate as R

AMBIGUOUS_CAP = 0.005


def test_header_constants_equal_the_modules():
    """The limits and the normal modes of include/lara_depthsurface.h, as the header defines them and as the module and the
    restatement repeat them."""
    from tests import test_abi_cpu as abi
    assert (depthsurface.MAX_VIEWS, depthsurface.MAX_CELLS, depthsurface.MAX_THRESHOLDS, depthsurface.ROW) == (64, 1 << 27, 8, 13)
    assert (depthsurface.NORMALS_NONE, depthsurface.NORMALS_GIVEN, depthsurface.NORMALS_DEPTH) == (0, 1, 2)
    text = abi.header_texts()["lara_depthsurface.h"]
    for macro, value in (("MAX_VIEWS", "64"), ("MAX_CELLS", "(1 << 27)"), ("MAX_THRESHOLDS", "8"), ("ROW", "13"), ("NORMALS_NONE", "0"),
                         ("NORMALS_GIVEN", "1"), ("NORMALS_DEPTH", "2")):
        assert f"#define LARA_DEPTHSURFACE_{macro} {value}\n" in text
    assert (R.MAX_CELLS, R.ROW) == (depthsurface.MAX_CELLS, depthsurface.ROW)


def test_refusals(hip_lib):
    """Sizes out of range, a bad mask element size, a stride of 0, a voxel that is not positive come back as LARA2DGS_E_INVALID
    (-1) from host code, before any pointer is used; N = 0 is a no-op; the python layer refuses CPU tensors and skewed cameras."""
    import ctypes
    L = hip_lib
    n, counts = (ctypes.c_int64 * 1)(), (ctypes.c_int64 * 2)(7, 7)
    inf = float("inf")
    assert L.lara_depthsurface_backproject_workspace_bytes(0, 4, 4) == -1 and L.lara_depthsurface_backproject_workspace_bytes(65, 4, 4) == -1
    assert L.lara_depthsurface_backproject_workspace_bytes(64, 8192, 4096) == -1          # 2^31 pixels
    assert L.lara_depthsurface_backproject_workspace_bytes(3, 5, 67) == 256 + 256
    assert L.lara_depthsurface_backproject_count(0, 4, 4, None, None, 1, 1, inf, n, None, None) == -1
    assert L.lara_depthsurface_backproject_count(1, 4, 4, None, None, 1, 0, inf, n, None, None) == -1         # stride 0
    assert L.lara_depthsurface_backproject_count(1, 4, 4, None, 1, 2, 1, inf, n, None, None) == -1            # 2-byte mask
    assert L.lara_depthsurface_backproject_count(1, 4, 4, None, None, 1, 1, inf, n, None, None) == -1         # null pointers
    assert L.lara_depthsurface_backproject_emit(1, 4, 4, None, None, 1, 1, inf, None, None, 3, None, inf, None, None, None, None, None) == -1
    assert L.lara_depthsurface_thin_workspace_bytes(-1, 8) == -1 and L.lara_depthsurface_thin_workspace_bytes(8, 0) == -1
    assert L.lara_depthsurface_thin_workspace_bytes(8, (1 << 27) + 1) == -1 and L.lara_depthsurface_thin_workspace_bytes(8, 64) == 4 * 256
    assert L.lara_depthsurface_thin(4, None, None, 0.0, 64, None, None, None, counts, None, None) == -1
    assert L.lara_depthsurface_thin(4, None, None, float("nan"), 64, None, None, None, counts, None, None) == -1
    assert L.lara_depthsurface_thin(4, None, None, 0.1, 64, None, None, None, counts, None, None) == -1          # null pointers
    assert L.lara_depthsurface_thin(0, None, None, 0.1, 64, None, None, None, counts, None, None) == 0 and list(counts) == [0, 0]
    assert L.lara_depthsurface_observe(4, None, 1, 4, 4, None, None, 1, inf, None, None, -1.0, 1, None, None) == -1   # tau < 0
    assert L.lara_depthsurface_observe(0, None, 1, 4, 4, None, None, 1, inf, None, None, 0.0, 1, None, None) == 0
    assert L.lara_depthsurface_observe(4, None, 1, 4, 4, None, None, 1, inf, None, None, 0.0, 1, None, None) == -1
    assert L.lara_depthsurface_reduce(5, 5, None, None, None, None, None, 9, None, None, None, None) == -1
    assert L.lara_depthsurface_reduce_workspace_bytes(1000) >= 4 * (3 * 8 + 10 * 4) and L.lara_depthsurface_reduce_workspace_bytes(-1) == -1
    c = C.sphere4()
    t = lambda a: torch.from_numpy(np.asarray(a))
    with pytest.raises(RuntimeError, match="no CPU path"):
        depthsurface.backproject(t(c["depth"]), t(c["mask"]), c["ixt"], c["c2w"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        depthsurface.thin(torch.zeros(4, 3), None, 0.1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        depthsurface.observe(torch.zeros(4, 3), t(c["depth"]), t(c["mask"]), c["ixt"], c["c2w"], 0.01)
    skew, row = c["ixt"].copy(), c["ixt"].copy()
    skew[1, 0, 1] = 1e-3
    row[2, 2] = [0.0, 0.0, 2.0]
    for bad in (skew, row):
        with pytest.raises(ValueError, match="no skew"):
            depthsurface.cameras(bad, c["c2w"])
    k, pose = depthsurface.cameras(t(c["ixt"]), t(c["c2w"]), invert=True)
    rk, rpose = R.cameras(c["ixt"], c["c2w"], invert=True)
    assert np.array_equal(k, rk) and np.array_equal(pose, rpose) and k.dtype == np.float32 and pose.shape == (4, 16)


def test_the_cases_are_what_the_tests_rely_on():
    c = C.sphere4()
    per_view = c["mask"].reshape(4, -1).sum(axis=1)
    assert c["depth"].shape == (4, 24, 32) and per_view.min() == 332 and per_view.max() == 368
    assert np.array_equal(R.valid(c["depth"], c["mask"]), c["mask"] != 0)
    for total in (255, 256, 257):
        e = C.edges(total)
        ok = R.valid(e["depth"], e["mask"], e["depth_max"])
        assert e["depth"].shape == (3, 5, 67) and ok.sum() == total and not ok[1].any() and ok[0, 0, 0] and ok[2, 4, 66]
        d, m = e["depth"], e["mask"]
        with np.errstate(invalid="ignore"):
            assert np.isnan(d).any() and np.isinf(d).any() and (d < 0).any() and (d == 0).any() and (d > e["depth_max"]).any()
            assert ((m == 0) & (d > 0) & (d < e["depth_max"])).any()
        for kind in ("uint8", "bool", "float32"):      # every spelling of the mask means the same pixels
            assert np.array_equal(R.valid(d, C.mask_as(m, kind), e["depth_max"]), ok)
        assert ok.sum() > R.valid(d, m, 1.5).sum() > 0
    s = C.stride_case()
    assert R.selected(s["depth"], s["mask"], 2).sum() == 2 * 4 * 5 - 3 and R.selected(s["depth"], s["mask"], 3).sum() == 2 * 3 * 3 - 2
    assert [len(C.queries(n)) for n in C.QUERY_SIZES] == [1, 255, 256, 257, 4096]
    sets = C.thin_sets()
    assert len(R.thin(*sets["sphere4"])[0]) > 500 and np.ptp(sets["sphere4"][0], axis=0).max() / sets["sphere4"][1] < 17
    assert R.thin(*sets["copies"])[0].tolist() == [0]
    assert R.thin(*sets["single"])[0].tolist() == [0] and R.thin(*sets["one_cell"])[0].tolist() == [0]
    kept, dropped = R.thin(*sets["nan_rows"])
    assert dropped == 4 and not np.isin(kept, [0, 100, 101, len(sets["nan_rows"][0]) - 1]).any()
    with pytest.raises(ValueError):
        R.thin(sets["sphere4"][0], 1e-4, max_cells=1 << 27)


@pytest.mark.parametrize("key", sorted(C.BACKPROJECT_CASES))
def test_backprojection_restatements_agree(key):
    """Order and pixel indices by hand (ascending g, only selected pixels), the fp32 points within 8 u S of the float64 ones, the
    depth normals zero exactly where the rule says so and unit elsewhere, the given normals unit or zero."""
    c = C.BACKPROJECT_CASES[key]()
    k, pose = R.cameras(c["ixt"], c["c2w"])
    dmax = c.get("depth_max", np.inf)
    for stride in (1, 2, 3):
        b = R.backproject(c["depth"], c["mask"], k, pose, stride, dmax, "depth")
        V, H, W = c["depth"].shape
        g = b["pixel"]
        assert np.all(np.diff(g) > 0) and np.all((g % W) % stride == 0) and np.all(((g // W) % H) % stride == 0)
        assert len(g) == R.selected(c["depth"], c["mask"], stride, dmax).sum()
        if "total" in c and stride == 1:
            assert len(g) == c["total"]
        assert b["points32"].dtype == np.float32 and np.isfinite(b["points64"]).all()
        assert np.all(np.abs(b["points32"].astype(np.float64) - b["points64"]) <= 8 * R.U * b["mag"])
        length = np.linalg.norm(b["normals"], axis=1)
        assert np.all(np.abs(length[b["applies"]] - 1.0) < 1e-12) and np.all(b["normals"][~b["applies"]] == 0)
    if key == "sphere4":
        # the depth normals point along the analytic ones (towards the camera or away: the sign is the cross product's)
        b = R.backproject(c["depth"], c["mask"], k, pose, 1, np.inf, "depth", 0.05)
        given = R.backproject(c["depth"], c["mask"], k, pose, 1, np.inf, c["normal_map"])["normals"]
        assert 800 < b["applies"].sum() < len(b["pixel"])
        cos = (b["normals"] * given).sum(axis=1)[b["applies"]]
        assert np.all(np.abs(cos) > 0.95) and (np.all(cos > 0) or np.all(cos < 0))
        assert np.all(np.abs(np.linalg.norm(given, axis=1) - 1.0) < 1e-12)
        true = R.backproject(c["depth"], c["mask"], k, pose)["points64"]
        assert np.all(np.abs(np.linalg.norm(true, axis=1) - C.RADIUS) < 1e-6)          # the points lie on the sphere


@pytest.mark.parametrize("n", C.QUERY_SIZES + ("special",))
@pytest.mark.parametrize("free", [True, False])
def test_observation_restatements_agree_outside_the_ambiguous_set(n, free):
    """fp32 and float64 give the same bits on every non-ambiguous (sample, view) pair, and the ambiguous share stays below 0.5 %:
    a larger share would let the GPU test hide a failure."""
    c = C.sphere4()
    k, w2c = R.cameras(c["ixt"], c["c2w"], invert=True)
    Q = C.queries_special() if n == "special" else C.queries(n)
    s64, amb = R.observe(Q, c["depth"], c["mask"], k, w2c, C.TAU, free)
    s32, _ = R.observe(Q, c["depth"], c["mask"], k, w2c, C.TAU, free, dtype=np.float32)
    differ = R.bits(s64, 4) != R.bits(s32, 4)
    assert not (differ & ~amb).any()
    assert amb.mean() <= AMBIGUOUS_CAP, amb.mean()
    if n == 4096:
        assert (0.55 if free else 0.45) < (s64 != 0).mean() < 0.8 and amb.sum() < 30
    if n == "special":
        fin = np.isfinite(Q).all(axis=1)
        assert np.all(s64[~fin] == 0) and (~fin).sum() == 3
        assert s64[-2] == 0 and s64[-1] != 0          # the centre is occluded everywhere; the point in front of the sphere is seen


def test_observation_by_hand():
    """One camera at the origin looking down +z, a 4 x 4 image, fx = fy = 2, centre (2, 2); a wall at depth 2 on the left half
    (valid), background on the right."""
    depth = np.zeros((1, 4, 4), np.float32)
    depth[0, :, :2] = 2.0
    mask = (depth > 0).astype(np.uint8)
    k, w2c = R.cameras(C.intrinsics(1, 2.0, 2.0, 2.0, 2.0), np.eye(4)[None], invert=True)
    Q = np.float32([[-0.5, 0.1, 1.0], [-1.0, 0.2, 2.005], [-1.0, 0.2, 2.02], [0.5, 0.1, 1.0], [0.1, 0.1, -1.0], [3.0, 0.1, 1.0]])
    for free, want in ((True, [1, 1, 0, 1, 0, 0]), (False, [1, 1, 0, 0, 0, 0])):
        for dtype in (np.float32, np.float64):
            seen, _ = R.observe(Q, depth, mask, k, w2c, 0.01, free, dtype=dtype)
            assert seen.tolist() == want


def test_reduce_restatement_by_hand():
    d = np.float32([0.5, 0.25, 1.0, 2.0])
    idx = np.array([0, 1, 5, 1])
    nq = np.float32([[1, 0, 0], [0, 0, 0], [0, 1, 0], [0, -1, 0]])
    nt = np.float32([[0.5, 0, 0], [0, 0.5, 0]])
    row = R.reduce_row(d, idx, 2, np.uint8([1, 1, 1, 0]), nq, nt, (0.3, 1.0))
    assert row.tolist() == [3, 1.75, 0.25 + 0.0625 + 1.0, 0.5, 1, 1, 3] + [0] * 6
    row = R.reduce_row(d, idx, 2, None, nq, nt, (0.3,))
    assert row.tolist() == [4, 3.75, 5.3125, 1.0, 2, 1] + [0] * 7


def _rows(kept, n_gt=8):
    row_p = np.zeros(depthsurface.ROW)
    row_g = np.zeros(depthsurface.ROW)
    if kept:
        row_p[:7] = [kept, 0.5 * kept, 0.5 * kept, 3.0, 4, kept / 2, kept]
    row_g[:7] = [n_gt, 2.0, 1.0, 1.0, 2, 2, n_gt]
    return row_p, row_g


def test_score_dict_and_its_way_through_the_evaluator(tmp_path):
    """`scores_from_rows` on stubbed rows: the keys of `surface_scores` with the same meanings plus the new ones; accuracy and
    precision None (fscore 0) without an observed sample; `Evaluator.add_geometry` and `summary()` take the dict unchanged."""
    from lara_amd import meshmetrics
    thr = [0.01, 0.02]
    s = depthsurface.scores_from_rows(*_rows(4), thr, True, n_pred=10)
    base = meshmetrics.scores_from_rows(np.zeros(12) + 1, np.zeros(12) + 1, thr, True)
    assert set(base) <= set(s) and set(s) - set(base) == {"n_pred_observed", "n_pred_unobserved", "normal_pairs"}
    assert s["accuracy"] == 0.5 and s["completeness"] == 0.25 and s["chamfer"] == 0.75 and s["chamfer_sq"] == 0.5 + 0.125
    assert s["precision"] == [0.5, 1.0] and s["recall"] == [0.25, 1.0] and s["fscore"] == [2 * 0.5 * 0.25 / 0.75, 1.0]
    assert s["normal_consistency"] == 4.0 / 6.0 and s["normal_pairs"] == 6
    assert (s["n_pred"], s["n_pred_observed"], s["n_pred_unobserved"], s["n_gt"]) == (10, 4, 6, 8)
    assert depthsurface.scores_from_rows(*_rows(4), thr, False)["normal_consistency"] is None
    none = depthsurface.scores_from_rows(*_rows(0), thr, True, n_pred=10)
    assert none["accuracy"] is None and none["precision"] is None and none["chamfer"] is None and none["fscore"] == [0.0, 0.0]
    assert none["completeness"] == 0.25 and none["recall"] == [0.25, 1.0] and none["n_pred_unobserved"] == 10
    full = dict(s, fallbacks=0, n_gt_raw=12, tau=0.02, voxel=None)          # what depth_scores adds on top
    ev = evaluate.Evaluator(4)
    ev.add_geometry("a", full)
    ev.add_geometry("b", dict(full, accuracy=0.25, chamfer=0.5))
    got = ev.write(str(tmp_path / "geo.json"))
    assert got == ev.summary() and got["geometry_name"] == ["a", "b"] and got["geometry_thresholds"] == thr
    assert got["accuracy"] == [0.5, 0.25] and got["accuracy_mean"] == 0.375 and got["fscore_mean"] == s["fscore"]
    ev.add_geometry("c", dict(full, accuracy=None, chamfer=None, chamfer_sq=None))
    assert ev.summary()["accuracy_mean"] is None and ev.summary()["completeness_mean"] == 0.25


def test_views_of_slices_a_batch_and_unrolls_the_normal_strip():
    """`tar_nrm` is a [H, V W, 3] strip per scene (the views side by side): view v is columns [v W, (v + 1) W)."""
    g = torch.Generator().manual_seed(0)
    B, V, H, W = 2, 3, 4, 5
    nrm = torch.randn(B, V, H, W, 3, generator=g)
    batch = {"tar_dep": torch.rand(B, V, H, W, generator=g), "tar_msk": torch.ones(B, V, H, W, dtype=torch.uint8),
             "tar_ixt": torch.rand(B, V, 3, 3, generator=g), "tar_c2w": torch.rand(B, V, 4, 4, generator=g)}
    dep, msk, ixt, c2w, none = depthsurface.views_of(batch, 1)
    assert none is None and torch.equal(dep, batch["tar_dep"][1]) and msk.shape == (V, H, W) and ixt.shape == (V, 3, 3) and c2w.shape == (V, 4, 4)
    batch["tar_nrm"] = nrm.permute(0, 2, 1, 3, 4).reshape(B, H, V * W, 3)
    got = depthsurface.views_of(batch, 1)[4]
    assert got.shape == (V, H, W, 3) and torch.equal(got, nrm[1])
    assert torch.equal(batch["tar_nrm"][1][:, 2 * W:3 * W], nrm[1, 2])
