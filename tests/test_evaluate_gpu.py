"""`lara_amd.evaluate` on the GPU (csrc/evalscores.hip): the scores kernel against the float64 restatement
(tests/eval_restate.py), bit-reproducibility and scene independence, the frame quantiser against numpy / torch on the CPU, and
the chunked turntable against per-view `render_img` calls.  Reads nothing outside this repository.

The bar of a score is 8 * max(E32, spacing32(value)): E32 is the error, against the restatement, of the SAME formulation in
float32 torch on the CPU (`lara_amd.loss._ssim_cs` level 0; `((x - y) ** 2).mean()`), spacing32 the float32 spacing at the value;
the factor 8 covers a different order of the same float32 sums (the sigma^2 = E[x^2] - mu^2 cancellation dominates both routes).
Every case prints both errors (copied to profiles/eval_parity.txt)."""
import math

import numpy as np
import pytest
import torch

from lara_amd import evaluate
from tests import eval_restate as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _images(B, V, H, W, noise, seed):
    """Seeded smooth-plus-noise pair: targets [B, V, H, W, 3] and the render [B, H, V*W, 3] = targets + noise, clamped."""
    g = torch.Generator().manual_seed(seed)
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    f = torch.rand(B, V, 1, 1, 3, generator=g) * 0.25 + 0.05
    ph = torch.rand(B, V, 1, 1, 3, generator=g) * 6.28
    tar = 0.5 + 0.35 * torch.sin(f * x[None, None, ..., None] + 0.7 * f * y[None, None, ..., None] + ph)
    img = tar.permute(0, 2, 1, 3, 4).reshape(B, H, V * W, 3)
    img = (img + noise * torch.randn(img.shape, generator=g)).clamp(0, 1)
    return tar.contiguous(), img.contiguous()


def _bars(tar, img, skip):
    """Per scene: float64 psnr / ssim[3] of the restatement and the float32-torch errors E32 of the same formulation."""
    from lara_amd.loss import _gauss_window, _ssim_cs
    W = tar.shape[3]
    psnr64, ssim64, _ = R.image_scores(img.numpy(), tar.numpy(), skip)
    x32 = img.permute(0, 3, 1, 2)[..., skip * W:].contiguous()
    y32 = torch.from_numpy(R.strip(tar.numpy()))[..., skip * W:].contiguous()
    ssim32 = _ssim_cs(x32, y32, _gauss_window("cpu"))[0].double().numpy()
    mse32 = ((x32 - y32) ** 2).flatten(1).mean(1).double().numpy()
    return psnr64, ssim64, np.abs(-10.0 * np.log10(mse32) - psnr64), np.abs(ssim32 - ssim64)


def _bar(e32, value):
    return 8.0 * max(float(e32), float(np.spacing(np.float32(abs(value)))))


@pytest.mark.parametrize("noise", [0.02, 0.3])
@pytest.mark.parametrize("B,V,n_views,H,W,crop", [(2, 8, 4, 64, 96, True), (2, 8, 4, 64, 96, False), (1, 1, 0, 11, 11, False),
                                                  (2, 3, 1, 37, 53, True), (1, 2, 0, 37, 53, False)])
def test_scores_against_the_float64_restatement(hip_lib, B, V, n_views, H, W, crop, noise):
    tar, img = _images(B, V, H, W, noise, seed=100 + H + V)
    skip = n_views if crop else 0
    psnr64, ssim64, e_psnr, e_ssim = _bars(tar, img, skip)
    batch, output = {"tar_rgb": tar.to(DEV)}, {"image_fine": img.to(DEV)}
    rows = evaluate.scores_device(output["image_fine"], batch["tar_rgb"], skip).cpu().numpy()
    got = evaluate.scene_scores(batch, output, n_views=n_views, novel_view_only=crop)
    failures = []
    for b in range(B):
        assert rows[b, 1] == 3 * H * (V - skip) * W
        psnr = -10.0 * math.log10(rows[b, 0] / rows[b, 1])
        assert got[b]["psnr"] == psnr and got[b]["ssim"] == (rows[b, 2] + rows[b, 3] + rows[b, 4]) / 3.0 and got[b]["depth_acc"] is None
        err, bar = abs(psnr - psnr64[b]), _bar(e_psnr[b], psnr64[b])
        print(f"eval_parity B={B} V={V} skip={skip} {H}x{W} noise={noise} scene={b} psnr={psnr64[b]:.6f} err={err:.3e} "
              f"E32={e_psnr[b]:.3e} bar={bar:.3e}")
        if not err <= bar:
            failures.append(("psnr", b, err, bar))
        for c in range(3):
            err, bar = abs(rows[b, 2 + c] - ssim64[b, c]), _bar(e_ssim[b, c], ssim64[b, c])
            print(f"eval_parity B={B} V={V} skip={skip} {H}x{W} noise={noise} scene={b} ch={c} ssim={ssim64[b, c]:.8f} "
                  f"err={err:.3e} E32={e_ssim[b, c]:.3e} bar={bar:.3e}")
            if not err <= bar:
                failures.append(("ssim", b, c, err, bar))
    assert not failures, failures


def _depth_inputs(seed=5):
    """Four scenes: masks empty, full, ~30 % inside (twice); differences exactly ON a threshold in scenes 1 and 2."""
    g = torch.Generator().manual_seed(seed)
    B, V, H, W = 4, 3, 40, 52
    thresholds = [0.01, 0.05, 0.1, 0.5]
    tar_dep = torch.rand(B, V, H, W, generator=g) * 2 + 0.5
    pred = tar_dep.permute(0, 2, 1, 3).reshape(B, H, V * W) + 0.08 * torch.randn(B, H, V * W, generator=g)
    msk = (torch.rand(B, V, H, W, generator=g) < 0.3).float() * (torch.rand(B, V, H, W, generator=g) + 0.5)      # nonzero = inside
    msk[0], msk[1] = 0.0, 1.0
    for b in (1, 2):
        for i, t in enumerate(thresholds):                # (2t, t), (t, 2t), (t, 0): exact in float32
            t32 = float(np.float32(t))
            tar_dep[b, 1, i, :3] = torch.tensor([t32, 2 * t32, 0.0])
            pred[b, i, W:W + 3] = torch.tensor([2 * t32, t32, t32])
            msk[b, 1, i, :3] = 1.0
    return pred.contiguous(), tar_dep.contiguous(), msk.contiguous(), thresholds


@pytest.mark.parametrize("mask_dtype", [torch.float32, torch.uint8, torch.bool, torch.int64])
@pytest.mark.parametrize("trailing", [False, True])
def test_depth_scores_counts_are_exact(hip_lib, mask_dtype, trailing):
    pred, tar_dep, msk, thresholds = _depth_inputs()
    want = R.depth_scores(pred.numpy(), tar_dep.numpy(), msk.numpy(), thresholds)
    m = msk.to(DEV) if mask_dtype == torch.float32 else (msk != 0).to(DEV).to(mask_dtype)
    p = pred[..., None] if trailing else pred
    rows = evaluate.scores_device(None, None, 0, p.to(DEV), tar_dep.to(DEV), m, thresholds).cpu().numpy()
    B, V, H, W = tar_dep.shape
    gt_strip = tar_dep.permute(0, 2, 1, 3).reshape(B, H, V * W).numpy()
    inside = (msk != 0).permute(0, 2, 1, 3).reshape(B, H, V * W).numpy()
    on = sum(int(((np.abs(pred.numpy() - gt_strip) == np.float32(t)) & inside).sum()) for t in thresholds)
    assert on >= 12, on                                   # differences exactly on a threshold are among the masked pixels
    assert [w[0] for w in want][:2] == [0, V * H * W] and 0.2 < want[2][0] / (V * H * W) < 0.4
    for b, (count, abs_sum, below) in enumerate(want):
        assert rows[b, 5] == count and list(rows[b, 7:7 + len(thresholds)]) == below, (b, rows[b], count, below)      # exact, every case
        assert not rows[b, :5].any() and not rows[b, 7 + len(thresholds):].any()
        if count:
            d = np.abs(pred.numpy()[b][inside[b]] - gt_strip[b][inside[b]])
            mean64 = abs_sum / count
            e32 = abs(float(d.mean()) - mean64)           # numpy's float32 mean: what the reference computes
            err, bar = abs(rows[b, 6] / rows[b, 5] - mean64), _bar(e32, mean64)
            print(f"eval_parity depth scene={b} mask={mask_dtype} mean_abs={mean64:.8f} err={err:.3e} E32={e32:.3e} bar={bar:.3e}")
            assert err <= bar, (b, err, bar)
    batch = {"tar_rgb": torch.rand(B, V, H, W, 3, device=DEV), "tar_dep": tar_dep.to(DEV), "tar_msk": m}
    output = {"image_fine": torch.rand(B, H, V * W, 3, device=DEV), "depth_fine": p.to(DEV)}
    got = evaluate.scene_scores(batch, output, n_views=V, novel_view_only=True, eval_depth=thresholds)       # the crop leaves nothing
    assert all(s["psnr"] is None and s["ssim"] is None for s in got)
    assert all(math.isnan(v) for v in got[0]["depth_acc"]) and len(got[0]["depth_acc"]) == 1 + len(thresholds)       # empty mask
    for b in (1, 2, 3):
        assert got[b]["depth_acc"] == R.depth_acc(int(rows[b, 5]), float(rows[b, 6]), [int(v) for v in rows[b, 7:7 + len(thresholds)]])


def test_scores_are_bit_reproducible_and_scenes_are_independent(hip_lib):
    B, V, H, W, n_views = 2, 8, 64, 96, 4
    tar, img = _images(B, V, H, W, 0.1, seed=9)
    pred, tar_dep, msk, thr = _depth_inputs(seed=6)
    tar, img = tar.to(DEV), img.to(DEV)
    dep = (pred[:2].to(DEV), tar_dep[:2].to(DEV), msk[:2].to(DEV))
    a = evaluate.scores_device(img, tar, n_views, *dep, thr)
    b = evaluate.scores_device(img, tar, n_views, *dep, thr)
    assert torch.equal(a, b) and torch.isfinite(a).all()
    for s in range(B):      # B = 2 gives the rows of two B = 1 calls
        one = evaluate.scores_device(img[s:s + 1].contiguous(), tar[s:s + 1].contiguous(), n_views, *(t[s:s + 1].contiguous() for t in dep), thr)
        assert torch.equal(one[0], a[s]), s
    # scores through the crop (a pointer offset into both layouts) == scores of a contiguous cropped copy
    cropped = evaluate.scores_device(img[:, :, n_views * W:].contiguous(), tar[:, n_views:].contiguous(), 0)
    assert torch.equal(cropped[:, :5], a[:, :5])
    full = evaluate.scores_device(img, tar, 0)
    assert not torch.equal(full[:, :5], a[:, :5])


def _tie_values():
    k = np.arange(255, dtype=np.float64)
    x = ((k + 0.5) / 255.0).astype(np.float32)
    ties = x[(x * np.float32(255)) == (k + 0.5).astype(np.float32)]
    assert ties.size > 0                                   # float32 x * 255 lands exactly on k + 1/2: rint must go to the even side
    return ties


@pytest.mark.parametrize("n,H,W,side_by_side", [(3, 16, 20, True), (3, 16, 20, False), (2, 9, 7, True), (1, 5, 13, False), (5, 32, 64, True)])
def test_quantiser_equals_numpy_and_the_float32_torch_expression(hip_lib, n, H, W, side_by_side):
    g = torch.Generator().manual_seed(n * 100 + W)
    ties = torch.from_numpy(_tie_values())
    shape = (H, n * W) if side_by_side else (n, H, W)
    image = torch.rand(*shape, 3, generator=g)
    flat = image.view(-1)
    special = torch.cat([torch.tensor([0.0, 1.0]), ties])[: flat.numel() // 2]
    flat[: special.numel()] = special
    normal = torch.nn.functional.normalize(torch.randn(*shape, 3, generator=g), dim=-1)
    normal.view(-1)[:6] = torch.tensor([1.0, -1.0, 0.0, 1.0, -1.0, 0.0])
    acc = torch.rand(*shape, generator=g)
    acc.view(-1)[:4] = torch.tensor([0.0, 1.0, 1.0, 0.0])
    frames, nframes = evaluate.quantize_frames(image.to(DEV), normal.to(DEV), acc.to(DEV), n=n if side_by_side else None)
    assert frames.dtype == torch.uint8 and frames.shape == (n, H, W, 3) == nframes.shape
    # evaluation.py:131, :134-135 evaluated on the CPU from the same inputs
    want = np.round(image.numpy() * 255).astype("uint8")
    alpha = acc[..., None]
    want_n = np.round((((normal * alpha + 1 - alpha) + 1) / 2).numpy() * 255).astype("uint8")
    assert np.array_equal(want, R.frames(image.numpy())) and np.array_equal(want_n, R.normal_frames(normal.numpy(), acc.numpy()))
    if side_by_side:
        want = want.reshape(H, n, W, 3).transpose(1, 0, 2, 3)
        want_n = want_n.reshape(H, n, W, 3).transpose(1, 0, 2, 3)
    assert np.array_equal(frames.cpu().numpy(), want)
    assert np.array_equal(nframes.cpu().numpy(), want_n)
    # an acc_map with a trailing axis of 1 is the same memory
    f2, n2 = evaluate.quantize_frames(image.to(DEV), normal.to(DEV), acc[..., None].to(DEV), n=n if side_by_side else None)
    assert torch.equal(f2, frames) and torch.equal(n2, nframes)


def _turntable_scene():
    from lara_amd.renderer import Renderer
    from tests.helpers import small_scene
    act, _ = small_scene(grid=16, size=128, seed=0)
    p = (act["means3D"].to(DEV), act["shs"].to(DEV), torch.logit(act["opacities"].to(DEV).clamp(1e-4, 1 - 1e-4)),
         torch.log(act["scales"].to(DEV)), act["rotations"].to(DEV))
    return Renderer(sh_degree=1, white_background=True), p


def _per_view_frames(renderer, cams, centers, shs, opacity, scales, rotations):
    """evaluation.py:126-135 with the rounding in torch: one `render_img` per camera under no_grad."""
    from lara_amd.batch import build_rays, fov_to_ixt
    frames, nframes = [], []
    with torch.no_grad():
        for cam in cams:
            ixt = fov_to_ixt(torch.tensor((cam.FoVx, cam.FoVy)), (cam.image_width, cam.image_height))[None].to(DEV)
            rays = build_rays(cam.view_world_transform[None].to(DEV), ixt, cam.image_height, cam.image_width)[0]
            out = renderer.render_img(cam, rays, centers, shs, opacity, scales, rotations, DEV)
            alpha = out["acc_map"].reshape(cam.image_height, cam.image_width)[..., None]
            frames.append(torch.round(out["image"] * 255).clamp(0, 255).to(torch.uint8))
            nframes.append(torch.round((((out["rend_normal"] * alpha + 1 - alpha) + 1) / 2) * 255).clamp(0, 255).to(torch.uint8))
    return torch.stack(frames), torch.stack(nframes)


@pytest.mark.parametrize("fine", [False, True])
def test_turntable_equals_per_view_render_img_calls(hip_lib, fine):
    renderer, (centers, shs, opacity, scales, rotations) = _turntable_scene()
    cams = evaluate.video_cameras(12, "gobjeverse", (128, 128), device=DEV)
    if fine:        # the fine 6-tuple: opacity / scaling / rotation are indexed by the mask, centres / shs come filtered already
        mask = torch.rand(centers.shape[0], generator=torch.Generator().manual_seed(1)).to(DEV) < 0.7
        assert 0 < int(mask.sum()) < mask.numel()
        gs = (centers[mask], shs[mask], opacity, scales, rotations, mask)
        args = (centers[mask], shs[mask], opacity[mask], scales[mask], rotations[mask])
    else:
        gs = (centers, shs, opacity, scales, rotations)
        args = gs
    frames, nframes = evaluate.render_turntable(renderer, gs, cams, chunk=5)
    assert frames.shape == (12, 128, 128, 3) == nframes.shape and frames.dtype == torch.uint8 and frames.is_cuda
    want, want_n = _per_view_frames(renderer, cams, *args)
    assert torch.equal(frames, want)
    assert torch.equal(nframes, want_n)
    assert frames.float().std() > 5 and nframes.float().std() > 5          # pictures, not a constant


def test_turntable_chunks_leave_no_memory_behind(hip_lib):
    renderer, gs = _turntable_scene()
    cams = evaluate.video_cameras(5, "gobjeverse", (128, 128), device=DEV)
    evaluate.render_turntable(renderer, gs, cams, chunk=5)
    torch.cuda.synchronize()
    first = torch.cuda.memory_allocated()
    for _ in range(50):
        evaluate.render_turntable(renderer, gs, cams, chunk=5)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == first
