"""`lara_amd.evaluate` on the CPU: camera paths against the reference's own (tests/golden/eval_ref.npz, made by
tests/golden/make_eval_fixture.py), the float64 restatement (tests/eval_restate.py) against the reference's depth functions and
against known SSIM answers, the host side of the scores, the `Evaluator`'s JSON, and the error paths.  The kernels themselves are
tested in tests/test_evaluate_gpu.py."""
import json
import math
import os

import numpy as np
import pytest
import torch

from lara_amd import evaluate
from tests import eval_restate as R

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = dict(rtol=2e-6, atol=2e-6)          # tests/test_cameras.py: fp32 LAPACK inverse in the reference, fp64 then rounded here


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(HERE, "golden", "eval_ref.npz"))


def _sample(ref):
    return {"transform_mats": torch.from_numpy(ref["cam/transform_mats"])}


def _fov(ref):
    return [torch.tensor([float(ref["cam/fov"][0])]), torch.tensor([float(ref["cam/fov"][1])])]


def _check_cams(cams, ref, tag, rays):
    assert len(cams) == ref[f"{tag}/world_view_transform"].shape[0]
    for i, cam in enumerate(cams):
        for name in ("world_view_transform", "full_proj_transform", "camera_center"):
            got, want = getattr(cam, name).numpy(), ref[f"{tag}/{name}"][i]
            assert got.dtype == np.float32 and got.shape == want.shape, (tag, name)
            np.testing.assert_allclose(got, want, err_msg=f"{tag} view {i} {name}", **TOL)
        fovx, fovy, near, far, w, h = ref[f"{tag}/scalars"][i]
        assert (cam.image_width, cam.image_height) == (int(w), int(h))
        assert math.isclose(cam.FoVx, fovx, rel_tol=1e-7) and math.isclose(cam.FoVy, fovy, rel_tol=1e-7), (tag, cam.FoVx, fovx)
        assert (cam.znear, cam.zfar) == (near, far)
        if rays:
            got = R.rays(cam.view_world_transform.numpy(), cam.FoVx, cam.FoVy, cam.image_width, cam.image_height)
            np.testing.assert_allclose(got, ref[f"{tag}/rays"][i], err_msg=f"{tag} view {i} rays", **TOL)


@pytest.mark.parametrize("family,name", [("gobj", "gobjeverse"), ("gobj", "GSO"), ("i3d", "instant3d"), ("i3d", "mvgen")])
@pytest.mark.parametrize("with_sample", [0, 1])
@pytest.mark.parametrize("elevation", [0, -30])
def test_video_cameras_equal_the_reference_path(ref, family, name, with_sample, elevation):
    size = tuple(int(v) for v in ref["cam/img_size"])
    cams = evaluate.video_cameras(8, name, size, sample=_sample(ref) if with_sample else None, fov=_fov(ref) if with_sample else None,
                                  elevation=elevation)
    _check_cams(cams, ref, f"cam/{family}/s{with_sample}/e{elevation}", rays=True)
    if family == "gobj":            # (sic) the reference's gobjaverse path overwrites whatever fov it was given
        assert (cams[0].FoVx, cams[0].FoVy) == (0.75, 0.75)
    elif with_sample:
        assert math.isclose(cams[0].FoVx, 0.6, rel_tol=1e-6) and math.isclose(cams[0].FoVy, 0.65, rel_tol=1e-6)


@pytest.mark.parametrize("family,name", [("gobj", "gobjeverse"), ("i3d", "instant3d"), ("i3d", "co3d")])
def test_mesh_cameras_equal_the_reference_path(ref, family, name):
    size = tuple(int(v) for v in ref["cam/img_size"])
    cams = evaluate.mesh_cameras(8, name, size, sample=_sample(ref), fov=_fov(ref))
    assert len(cams) == 24
    _check_cams(cams, ref, f"mesh/{family}", rays=False)


def test_unposed_path_and_unknown_datasets_are_refused():
    with pytest.raises(NotImplementedError, match="camera_utils"):
        evaluate.video_cameras(8, "unposed", (16, 16))
    with pytest.raises(NotImplementedError, match="camera_utils"):
        evaluate.mesh_cameras(8, "unposed", (16, 16))
    with pytest.raises(ValueError, match="no camera path"):
        evaluate.video_cameras(8, "co3d", (16, 16))            # uni_video_path has no branch for it (only uni_mesh_path)


def test_depth_scores_equal_the_reference_functions(ref):
    thresholds = [float(t) for t in ref["depth/thresholds"]]
    got = R.depth_scores(ref["depth/depth_fine"], ref["depth/tar_dep"], ref["depth/tar_msk"], thresholds)
    on_threshold = 0
    for b, (count, abs_sum, below) in enumerate(got):
        want_counts, want_acc = ref[f"depth/{b}/counts"], ref[f"depth/{b}/depth_acc"]
        assert [count] + below == [int(c) for c in want_counts], b                      # exact
        rows = [[0, 0, 0, 0, 0, count, abs_sum] + below + [0] * (9 - len(below))]
        acc = evaluate.scores_from_rows(rows, len(thresholds), image=False, depth=True)[0]["depth_acc"]
        assert acc == R.depth_acc(count, abs_sum, below)
        # the reference's mean is numpy's float32 mean: within its rounding (pairwise sums: a few spacings)
        assert abs(acc[0] - want_acc[0]) <= 4 * np.spacing(np.float32(want_acc[0])), (b, acc[0], want_acc[0])
        np.testing.assert_allclose(acc[1:], want_acc[1:], rtol=1e-15, atol=0)
    # the fixture holds differences exactly ON a threshold (not below it): the strict compare leaves them out
    B, V, H, W = ref["depth/tar_dep"].shape
    pred = ref["depth/depth_fine"].reshape(B, H, V * W)
    gt = ref["depth/tar_dep"].transpose(0, 2, 1, 3).reshape(B, H, V * W)
    for t in thresholds:
        on_threshold += int((np.abs(pred - gt) == np.float32(t)).sum())
    assert on_threshold > 0
    assert evaluate.scores_from_rows([[0.0] * 16], 2, image=False, depth=True)[0]["depth_acc"][0] != \
        evaluate.scores_from_rows([[0.0] * 16], 2, image=False, depth=True)[0]["depth_acc"][0]      # empty mask: NaN


def test_psnr_equals_the_reference_expression(ref):
    x, y = ref["psnr/images"].astype(np.float64), ref["psnr/img_gt"].astype(np.float64)
    rows = [[float(((x - y) ** 2).sum()), float(x.size)] + [1.0] * 14]
    got = evaluate.scores_from_rows(rows)[0]["psnr"]
    assert abs(got - float(ref["psnr/psnr"])) <= 8 * np.spacing(np.float32(ref["psnr/psnr"])), (got, float(ref["psnr/psnr"]))
    assert evaluate.scores_from_rows(rows)[0]["ssim"] == 1.0


def test_restated_taps_are_the_packages_float32_taps():
    from lara_amd.loss import _gauss_window
    np.testing.assert_array_equal(R.gauss_taps(), _gauss_window("cpu").double().numpy())


def test_ssim_known_answers():
    g = np.random.default_rng(0)
    x = g.random((2, 3, 20, 31))
    np.testing.assert_allclose(R.ssim(x, x), 1.0, rtol=0, atol=1e-15)
    s = R.gauss_taps().sum() ** 2          # the float32 taps do not sum to exactly 1
    for a, b in ((0.2, 0.7), (0.0, 1.0), (0.5, 0.5)):
        X, Y = np.full((1, 1, 11, 13), a), np.full((1, 1, 11, 13), b)
        C1, C2 = 0.01 ** 2, 0.03 ** 2
        lum = (2 * a * b * s * s + C1) / ((a * a + b * b) * s * s + C1)
        cs = (2 * a * b * (s - s * s) + C2) / ((a * a + b * b) * (s - s * s) + C2)
        np.testing.assert_allclose(R.ssim(X, Y), lum * cs, rtol=1e-12)
        # ... which is (2ab + C1) / (a^2 + b^2 + C1) up to the taps' own rounding: the contrast factor is 1 - (s - s^2) (a - b)^2 /
        # (C2 + ...) instead of 1 (1.7e-5 for (0.2, 0.7): the float32 taps sum to 1 - 3e-8), the luminance factor moves by O(s^2 - 1)
        bound = abs(s - s * s) * (a - b) ** 2 / C2 + 4 * abs(s * s - 1) + 1e-12
        np.testing.assert_allclose(R.ssim(X, Y), (2 * a * b + C1) / (a * a + b * b + C1), rtol=bound)
    with pytest.raises(ValueError):
        R.ssim(np.zeros((1, 1, 10, 40)), np.zeros((1, 1, 10, 40)))


def test_restatement_agrees_with_the_float64_level_0_of_the_training_term():
    from lara_amd.loss import _gauss_window, _ssim_cs
    g = torch.Generator().manual_seed(3)
    X, Y = torch.rand(2, 3, 37, 53, generator=g, dtype=torch.float64), torch.rand(2, 3, 37, 53, generator=g, dtype=torch.float64)
    s, cs = _ssim_cs(X, Y, _gauss_window("cpu").double())
    np.testing.assert_allclose(R.ssim(X.numpy(), Y.numpy()), s.numpy(), rtol=1e-12)
    np.testing.assert_allclose(R.ssim_map(X.numpy(), Y.numpy())[1].mean(axis=(-2, -1)), cs.numpy(), rtol=1e-12)


def test_evaluator_writes_the_reference_keys_and_means(tmp_path):
    ev = evaluate.Evaluator(n_views=4, eval_depth=[0.01, 0.05])
    ev.add_scores("a", 20.0, 0.8, [0.1, 0.5, 0.75])
    ev.add_scores("b", 30.0, 0.9, [0.3, 0.25, 1.0])
    path = tmp_path / "sub" / "metrics.json"
    ev.write(str(path))
    got = json.loads(path.read_text())
    # evaluation.py:167-172: the dictionary and its update ('depth_acc' ends up as the mean)
    assert set(got) == {"name", "psnr", "ssim", "lpips_vgg", "lpips_alex", "depth_acc", "psnr_mean", "ssim_mean", "lpips_vgg_mean",
                        "lpips_alex_mean"}
    assert got["name"] == ["a", "b"] and got["psnr"] == [20.0, 30.0] and got["ssim"] == [0.8, 0.9]
    assert got["psnr_mean"] == float(np.mean([20.0, 30.0])) and got["ssim_mean"] == float(np.mean([0.8, 0.9]))
    assert got["depth_acc"] == np.mean(np.stack([[0.1, 0.5, 0.75], [0.3, 0.25, 1.0]]), axis=0).tolist()
    # LPIPS is not computed here: null unless the caller brings the networks
    assert got["lpips_vgg"] == [None, None] and got["lpips_vgg_mean"] is None and got["lpips_alex_mean"] is None
    ev2 = evaluate.Evaluator(n_views=4, lpips={"vgg": lambda a, b: 0.25, "alex": lambda a, b: 0.5})
    ev2.add_scores("a", 20.0, 0.8, None, 0.25, 0.5)
    s = ev2.summary()
    assert s["lpips_vgg_mean"] == 0.25 and s["lpips_alex_mean"] == 0.5 and s["depth_acc"] == 0.0      # no thresholds: 0.0 (:162)
    assert evaluate.Evaluator(n_views=4).write(str(tmp_path / "none.json")) is None and not (tmp_path / "none.json").exists()


def test_error_paths():
    B, V, H, W = 1, 2, 16, 16
    batch = {"tar_rgb": torch.rand(B, V, H, W, 3), "tar_dep": torch.rand(B, V, H, W), "tar_msk": torch.ones(B, V, H, W)}
    output = {"image_fine": torch.rand(B, H, V * W, 3), "depth_fine": torch.rand(B, H, V * W, 1)}
    with pytest.raises(RuntimeError, match="no CPU path"):
        evaluate.scene_scores(batch, output, n_views=1, eval_depth=[0.1])
    with pytest.raises(RuntimeError, match="no CPU path"):
        evaluate.scene_scores(batch, output, n_views=2)                   # nothing left to score: still no CPU path
    with pytest.raises(RuntimeError, match="no CPU path"):
        evaluate.quantize_frames(torch.rand(2, 8, 8, 3), torch.rand(2, 8, 8, 3), torch.rand(2, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        evaluate.render_turntable(None, tuple(torch.zeros(4, k) for k in (3, 3, 1, 2, 4)), evaluate.video_cameras(2, "GSO", (16, 16)))
    with pytest.raises(ValueError, match="at most 8"):
        evaluate.scene_scores(batch, output, n_views=1, eval_depth=[0.01 * k for k in range(1, 10)])
    small = {"tar_rgb": torch.rand(1, 2, 10, 16, 3)}
    with pytest.raises(ValueError, match="at least 11"):
        evaluate.scene_scores(small, {"image_fine": torch.rand(1, 10, 32, 3)}, n_views=1)
    narrow = {"tar_rgb": torch.rand(1, 2, 16, 10, 3)}
    with pytest.raises(ValueError, match="at least 11"):
        evaluate.scene_scores(narrow, {"image_fine": torch.rand(1, 16, 20, 3)}, n_views=1)      # the crop leaves 10 columns


def test_library_refuses_bad_sizes_before_any_launch(hip_lib):
    """include/lara_eval.h: a side below 11, more than 8 thresholds, a bad mask element size -> LARA2DGS_E_INVALID (the
    argument checks come before any pointer is used)."""
    import ctypes
    from lara_amd._native import load_library
    lib = load_library()
    v = evaluate._ImgView(4096, 1000, 1, 100, 30, 3, 10)
    d = ctypes.c_void_p(4096)
    thr = (ctypes.c_double * 9)(*[0.1] * 9)
    call = lambda H, W, n_thr, mb=1: lib.lara_eval_scores(1, H, W, ctypes.byref(v), ctypes.byref(v), d, 1, 16, 16, d, d, d, mb, n_thr,
                                                          thr, d, d, None)
    assert call(10, 40, 0) == -1 and call(40, 10, 0) == -1 and call(16, 16, 9) == -1 and call(16, 16, 1, 2) == -1
    assert lib.lara_eval_workspace_doubles(1, 10, 40, 0, 0, 0) == -1
    assert lib.lara_eval_workspace_doubles(2, 11, 11, 0, 0, 0) == 2 * 4 + 1
    assert lib.lara_eval_quantize_frames(1, 0, 8, 8, 8, d, d, d, d, d, None) == -1
