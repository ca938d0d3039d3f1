"""The float64 / integer restatement of include/lara_meshmetrics.h (tests/meshmetrics_restate.py) held to closed forms,
the header's constants held to the module's, the library's refusals, and the Evaluator's geometry hook -- no GPU.
tests/test_meshmetrics_gpu.py holds the kernels to this restatement."""
import ctypes
import json

import numpy as np
import pytest
import torch

from lara_amd import evaluate, meshmetrics
from tests import meshmetrics_restate as R


def test_header_constants_equal_the_modules():
    """The limits of include/lara_meshmetrics.h, as the header defines them and as the module repeats them."""
    from tests import test_abi_cpu as abi
    assert (meshmetrics.MAX_SAMPLES, meshmetrics.RMAX, meshmetrics.MAX_GRID, meshmetrics.MAX_THRESHOLDS, meshmetrics.ROW) == \
        (1 << 22, 4, 256, 8, 12)
    text = abi.header_texts()["lara_meshmetrics.h"]
    for macro, value in (("MAX_SAMPLES", "(1 << 22)"), ("RMAX", "4"), ("MAX_GRID", "256"), ("MAX_THRESHOLDS", "8"), ("ROW", "12")):
        assert f"#define LARA_MESHMETRICS_{macro} {value}\n" in text


def test_refusals(hip_lib):
    """T = 0, M = 0 and n > 2^22 come back as LARA2DGS_E_INVALID (-1) from host code, before any pointer is used; N = 0 is a
    no-op; the python layer refuses what the library refuses, and CPU tensors."""
    q, s = (ctypes.c_int64 * 4)(), (ctypes.c_int32 * 1)()
    assert hip_lib.lara_meshmetrics_sample_workspace_bytes(0) == -1
    assert hip_lib.lara_meshmetrics_sample_workspace_bytes(1 << 28) == -1
    assert hip_lib.lara_meshmetrics_sample_workspace_bytes(12) > 12 * 16
    assert hip_lib.lara_meshmetrics_sample_surface(4, 0, None, None, 16, 0, q, s, None, None, None, None, None) == -1
    assert hip_lib.lara_meshmetrics_sample_surface(4, 2, None, None, (1 << 22) + 1, 0, q, s, None, None, None, None, None) == -1
    assert hip_lib.lara_meshmetrics_sample_surface(4, 2, None, None, -1, 0, q, s, None, None, None, None, None) == -1
    assert hip_lib.lara_meshmetrics_sample_surface(4, 2, None, None, 16, 0, q, s, None, None, None, None, None) == -1      # null pointers
    assert hip_lib.lara_meshmetrics_nearest_workspace_bytes(5, 0) == -1
    assert hip_lib.lara_meshmetrics_nearest_workspace_bytes(0, 5) > 0
    assert hip_lib.lara_meshmetrics_nearest(5, 0, None, None, None, None, None, None, None) == -1
    assert hip_lib.lara_meshmetrics_nearest(0, 5, None, None, None, None, None, None, None) == 0
    assert hip_lib.lara_meshmetrics_nearest(5, 5, None, None, None, None, None, None, None) == -1
    assert hip_lib.lara_meshmetrics_reduce(5, 5, None, None, None, None, 9, None, None, None, None) == -1
    assert hip_lib.lara_meshmetrics_reduce_workspace_bytes(1000) >= 4 * (3 * 8 + 8 * 4)
    # the stated rule for the grid: clamp(ceil(sqrt(M / 4)), 1, 256)
    assert [hip_lib.lara_meshmetrics_grid_resolution(m) for m in (1, 4, 5, 63, 1000, 4096, 262144, 262145, 10 ** 6)] == \
        [1, 1, 2, 4, 16, 32, 256, 256, 256]
    assert hip_lib.lara_meshmetrics_grid_resolution(0) == -1
    V, F = R.cube()
    with pytest.raises(RuntimeError, match="no CPU path"):
        meshmetrics.sample_surface(torch.from_numpy(V), torch.from_numpy(F), 16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        meshmetrics.nearest(torch.zeros(4, 3), torch.zeros(4, 3))
    for fn in (lambda: R.sample_surface(V, F[:0], 16), lambda: R.sample_surface(V, F, (1 << 22) + 1),
               lambda: R.nearest(np.zeros((3, 3)), np.zeros((0, 3))), lambda: R.sample_surface(V, np.zeros((2, 3), np.int64), 16)):
        with pytest.raises(ValueError):
            fn()


def test_surfaces_are_taken_as_the_mesh_path_returns_them():
    """`clean_mesh` returns (vertices, triangles, colors, info) and `read_obj` numpy (vertices, triangles, colors or None): both
    are recognised as meshes by their integer second entry and reach the sampler (which, here, refuses the CPU); a floating
    second entry is a point set's normals."""
    V, F = R.cube()
    cpu = torch.device("cpu")
    for mesh in ((torch.from_numpy(V), torch.from_numpy(F), torch.rand(8, 3), {"kept": 1}), (V, F, None), (V, F.astype(np.int32))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            meshmetrics._surface(mesh, 16, 0, cpu)
    pts, nrm = meshmetrics._surface((V, np.ones_like(V)), 16, 0, cpu)
    assert pts.shape == (8, 3) and nrm.shape == (8, 3) and nrm.dtype == torch.float32
    assert meshmetrics._surface(V, 16, 0, cpu)[1] is None and meshmetrics._surface((torch.from_numpy(V),), 16, 0, cpu)[1] is None
    with pytest.raises(RuntimeError, match="shape of its points"):
        meshmetrics._surface((V, np.ones((3, 3), np.float32)), 16, 0, cpu)


def test_parallel_squares_at_distance_delta():
    """Two parallel unit squares at distance delta: every distance is >= delta, chamfer -> 2 delta as the sampling gets dense,
    and the F-score is 0 below delta and 1 above."""
    delta = 0.05
    (Va, Fa), (Vb, Fb) = R.unit_square(0.0), R.unit_square(delta)
    worst = []
    for n in (256, 4096):
        P, Pn, *_ = R.sample_surface(Va, Fa, n, seed=1)
        G, Gn, *_ = R.sample_surface(Vb, Fb, n, seed=2)
        s = R.scores(P, Pn, G, Gn, (0.5 * delta, 0.999 * delta, 1.5 * delta))
        (d_p, _), (d_g, _) = R.nearest(P, G), R.nearest(G, P)
        assert d_p.min() >= delta * (1 - 1e-6) and d_g.min() >= delta * (1 - 1e-6)
        assert s["fscore"][0] == 0.0 and s["fscore"][1] == 0.0 and s["precision"][:2] == [0.0, 0.0]
        assert s["chamfer"] >= 2 * delta * (1 - 1e-6)
        assert abs(s["normal_consistency"] - 1.0) < 1e-12
        worst.append(s["chamfer"] - 2 * delta)
        if n == 4096:      # the sample spacing is 1 / 64: the in-plane offset to the nearest sample is far below delta
            assert s["fscore"][2] == 1.0 and s["chamfer"] < 2 * delta * 1.03
    assert worst[1] < worst[0]


def test_a_surface_against_itself():
    V, F = R.uv_sphere()
    P, Pn, *_ = R.sample_surface(V, F, 1000, seed=3)
    s = R.scores(P, Pn, P, Pn, (1e-9,))
    assert s["chamfer"] == 0.0 and s["chamfer_sq"] == 0.0 and s["fscore"] == [1.0] and s["accuracy"] == 0.0
    assert abs(s["normal_consistency"] - 1.0) < 1e-12
    assert R.scores(P, None, P, Pn, (1e-9,))["normal_consistency"] is None


@pytest.mark.parametrize("n", [1, 63, 64, 257, 4096])
def test_stratified_counts_and_barycentrics(n):
    """Counts per triangle within +-1 of n A_i / sum A (the quantisation moves a stratum's edge by far less than a stratum);
    barycentrics non-negative, summing to 1 within 2^-23; zero-area triangles never chosen; points inside their triangles."""
    V, F = R.uv_sphere()
    F = np.concatenate([F, [[0, 0, 1], [3, 3, 3]]])          # two degenerate triangles at the end
    pts, nrm, face, q, s = R.sample_surface(V, F, n, seed=7)
    A = R.areas(V, F)
    assert q[-1] == 0 and q[-2] == 0 and 2 ** 38 - len(F) <= q.sum() < 2 ** 39
    counts = np.bincount(face, minlength=len(F))
    assert np.all(np.abs(counts - n * A / A.sum()) <= 1.0 + 1e-9) and counts[-2:].sum() == 0 and counts.sum() == n
    b = R.barycentrics(7, n)
    assert np.all(b >= 0.0) and np.all(np.abs(b.sum(1) - 1.0) <= 2.0 ** -23)
    assert np.all(np.abs(np.linalg.norm(nrm, axis=1) - 1.0) < 1e-12)
    # on the sphere's inscribed mesh: inside the unit ball, outside the ball the flat faces stay clear of, normals outward
    rad = np.linalg.norm(pts, axis=1)
    assert np.all(rad <= 1.0 + 1e-6) and np.all(rad > 0.9) and np.all((pts * nrm).sum(1) > 0)
    # another seed moves the points, not the faces
    pts2, _, face2, _, _ = R.sample_surface(V, F, n, seed=8)
    assert np.array_equal(face, face2) and not np.array_equal(pts, pts2)


def test_area_ratio_one_to_three():
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [3, 0, 0], [0, 0, 1]], np.float32)      # areas 1/2 and 3/2
    F = np.array([[0, 1, 2], [0, 3, 4]], np.int64)
    _, _, face, q, s = R.sample_surface(V, F, 64, seed=0)
    assert q.tolist() == [2 ** 36, 3 * 2 ** 36] and s == 37          # total 2 = 0.5 x 2^2: s = 39 - 2
    assert np.bincount(face).tolist() == [16, 48] and np.all(np.diff(face) >= 0)
    assert R.mix(np.uint64(0)) == 0 and R.mix(np.uint64(1)) != R.mix(np.uint64(2))
    r1, r2 = R.hashed_r(0, 4096)
    assert 0.45 < r1.mean() < 0.55 and 0.45 < r2.mean() < 0.55 and r1.max() < 1.0 and abs(np.corrcoef(r1, r2)[0, 1]) < 0.1


def _scores(chamfer, nc=0.9):
    return {"accuracy": chamfer / 4, "completeness": 3 * chamfer / 4, "chamfer": chamfer, "chamfer_sq": chamfer ** 2,
            "normal_consistency": nc, "thresholds": [0.01, 0.02], "precision": [0.5, 1.0], "recall": [0.25, 0.5],
            "fscore": [1.0 / 3.0, 2.0 / 3.0], "n_pred": 10, "n_gt": 10, "fallbacks": 0}


def test_evaluator_json_is_unchanged_without_geometry_and_holds_it_with(tmp_path):
    def fill(ev):
        ev.add_scores("a", psnr=30.0, ssim=0.9, lpips_vgg=0.1, lpips_alex=0.2)
        ev.add_scores("b", psnr=20.0, ssim=0.8, lpips_vgg=0.3, lpips_alex=0.4)
    plain, geo = evaluate.Evaluator(4), evaluate.Evaluator(4)
    fill(plain)
    fill(geo)
    expected = {"name": ["a", "b"], "psnr": [30.0, 20.0], "ssim": [0.9, 0.8], "lpips_vgg": [0.1, 0.3], "lpips_alex": [0.2, 0.4],
                "depth_acc": 0.0, "psnr_mean": 25.0, "ssim_mean": (0.9 + 0.8) / 2, "lpips_vgg_mean": 0.2,
                "lpips_alex_mean": (0.2 + 0.4) / 2}
    plain.write(str(tmp_path / "plain.json"))
    with open(tmp_path / "expected.json", "w") as f:
        json.dump(expected, f, indent=4)
    assert (tmp_path / "plain.json").read_bytes() == (tmp_path / "expected.json").read_bytes()
    geo.add_geometry("a", _scores(0.04))
    geo.add_geometry("b", _scores(0.02, nc=0.7))
    geo.write(str(tmp_path / "geo.json"))
    got = json.loads((tmp_path / "geo.json").read_text())
    assert list(got)[:len(expected)] == list(expected) and {k: got[k] for k in expected} == json.loads(json.dumps(expected))
    assert got["geometry_name"] == ["a", "b"] and got["geometry_thresholds"] == [0.01, 0.02]
    assert got["chamfer"] == [0.04, 0.02] and abs(got["chamfer_mean"] - 0.03) < 1e-15
    for k in ("accuracy", "completeness"):
        assert got[k] == [_scores(0.04)[k], _scores(0.02)[k]] and got[k + "_mean"] == sum(got[k]) / 2
    assert abs(got["normal_consistency_mean"] - 0.8) < 1e-15 and got["chamfer_sq"] == [0.04 ** 2, 0.02 ** 2]
    assert got["fscore"] == [[1.0 / 3.0, 2.0 / 3.0]] * 2 and got["fscore_mean"] == [1.0 / 3.0, 2.0 / 3.0]
    assert got["precision_mean"] == [0.5, 1.0] and got["recall_mean"] == [0.25, 0.5]
    # a point set without normals: the mean is null, as the LPIPS means are without a network
    geo.add_geometry("c", _scores(0.02, nc=None))
    assert geo.summary()["normal_consistency_mean"] is None and geo.summary()["normal_consistency"][2] is None
    # geometry alone is written too; thresholds must agree across scenes
    only = evaluate.Evaluator(4)
    assert only.summary() is None
    only.add_geometry("a", _scores(0.04))
    assert only.summary()["chamfer_mean"] == 0.04 and "psnr" not in only.summary()
    with pytest.raises(ValueError):
        only.add_geometry("b", dict(_scores(0.04), thresholds=[0.5]))


def test_scores_from_rows_handles_empty_matches():
    row_p = np.array([4, 2.0, 1.5, 3.0, 0, 2, 0, 0, 0, 0, 0, 0], np.float64)
    row_g = np.array([2, 1.0, 0.75, 1.0, 0, 2, 0, 0, 0, 0, 0, 0], np.float64)
    s = meshmetrics.scores_from_rows(row_p, row_g, [0.1, 0.2], True)
    assert s["accuracy"] == 0.5 and s["completeness"] == 0.5 and s["chamfer"] == 1.0 and s["chamfer_sq"] == 0.75
    assert s["precision"] == [0.0, 0.5] and s["recall"] == [0.0, 1.0] and s["fscore"] == [0.0, 2 * 0.5 / 1.5]
    assert s["normal_consistency"] == 4.0 / 6.0
    assert meshmetrics.scores_from_rows(row_p, row_g, [0.1], False)["normal_consistency"] is None
