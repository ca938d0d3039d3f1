"""Times `lara_amd.evaluate` against the routes the package offered before it, on one MI355X, with HIP events after warm-up:
  (a) scene_scores (one kernel pass, one host read) against the float32 torch `_ssim_cs` + mean-square on the device plus
      tools/depth.py's arithmetic in numpy after the three host copies (evaluation.py:75-111), for a synthetic batch at 512^2,
      8 target views, n_views = 4 (the crop leaves 4);
  (b) render_turntable (chunks of 8 through `render_views`, frames quantised on the device) against the per-view `render_img`
      loop with per-frame host rounding (evaluation.py:126-138 as written), 120 frames at 512^2;
  (c) bytes the scores image pass addresses per pixel of the strip (42 x 42 inputs per 32 x 32 tile) against the algorithmic
      count, and the rate of algorithmic bytes the kernels reach.
Wall-clock (host) times are reported beside the event times for the legs that end in a host read.  Prints one JSON line.
    python tools/eval_bench.py [--steps 10] [--warmup 3] [--frames 120] [--out profiles/eval_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, steps, warmup):
    """(ms per call by HIP events, ms per call by the host clock with a synchronise at the end)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps, (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench: needs an MI355X")
    from lara_amd import evaluate, synthetic
    from lara_amd.batch import build_rays, fov_to_ixt, synthetic_batch
    from lara_amd.loss import _gauss_window, _ssim_cs
    from lara_amd.renderer import Renderer
    dev = torch.device("cuda:0")
    B, V, n_views, S = 1, 8, 4, 512
    thresholds = [0.01, 0.05, 0.1]
    g = torch.Generator().manual_seed(0)
    batch = synthetic_batch(batch_size=B, n_views=V, H=S, W=S, n_input=n_views, seed=0, device=dev)
    batch["tar_rgb"] = torch.rand(B, V, S, S, 3, generator=g).to(dev)
    batch["tar_dep"] = (torch.rand(B, V, S, S, generator=g) * 2 + 0.5).to(dev)
    batch["tar_msk"] = (torch.rand(B, V, S, S, generator=g) < 0.3).float().to(dev)
    image = (batch["tar_rgb"].permute(0, 2, 1, 3, 4).reshape(B, S, V * S, 3) + 0.05 * torch.randn(B, S, V * S, 3, generator=g).to(dev)).clamp(0, 1)
    depth = (batch["tar_dep"].permute(0, 2, 1, 3).reshape(B, S, V * S) + 0.05 * torch.randn(B, S, V * S, generator=g).to(dev))[..., None]
    output = {"image_fine": image.contiguous(), "depth_fine": depth.contiguous()}
    win = _gauss_window(dev)

    def scores_hip():
        return evaluate.scene_scores(batch, output, n_views, True, thresholds)

    def scores_torch():          # evaluation.py:64-65, :75-87 with the package's torch SSIM, then :98-110 as written (numpy on the host)
        images = output["image_fine"][0]
        img_gt = batch["tar_rgb"][0].permute(1, 0, 2, 3).reshape(images.shape)
        images = images.permute(2, 0, 1)[None][..., S * n_views:]
        img_gt = img_gt.permute(2, 0, 1)[None][..., S * n_views:]
        psnr = (-10.0 * torch.log(((images - img_gt) ** 2).mean()) / math_log10).item()
        ssim = _ssim_cs(images, img_gt, win)[0].mean().item()
        mask = batch["tar_msk"].permute(0, 2, 1, 3).reshape(B, S, V * S).cpu().bool().numpy()
        gt = batch["tar_dep"].permute(0, 2, 1, 3).reshape(B, S, V * S).cpu().numpy()
        pred = output["depth_fine"].cpu().squeeze(-1).numpy()
        err = np.abs(pred[mask] - gt[mask])
        acc = [err.mean().item()] + [(np.abs(pred[mask] - gt[mask]) < t).astype("float").mean() for t in thresholds]
        return psnr, ssim, acc

    math_log10 = torch.log(torch.tensor([10.0], device=dev))
    res = {"shape": {"scenes": B, "views": V, "n_views": n_views, "size": [S, S], "thresholds": len(thresholds), "frames": a.frames}, "unit": "ms"}
    hip, ref = scores_hip()[0], scores_torch()
    res["scores_check"] = {"psnr": [hip["psnr"], ref[0]], "ssim": [hip["ssim"], ref[1]], "depth_acc0": [hip["depth_acc"][0], ref[2][0]]}
    res["scores_hip_event"], res["scores_hip_wall"] = timed(scores_hip, a.steps, a.warmup)
    res["scores_torch_numpy_event"], res["scores_torch_numpy_wall"] = timed(scores_torch, a.steps, a.warmup)
    # the kernels alone (no host read), and (c): what they address against the algorithmic count
    dev_only = lambda: evaluate.scores_device(output["image_fine"], batch["tar_rgb"], n_views, output["depth_fine"], batch["tar_dep"],
                                              batch["tar_msk"], thresholds)
    res["scores_kernels_event"], _ = timed(dev_only, a.steps * 5, a.warmup)
    Wc = (V - n_views) * S
    tiles = ((S - 10 + 31) // 32) * ((Wc - 10 + 31) // 32)
    img_alg, img_addr = 24.0, tiles * 42 * 42 * 24.0 / (S * Wc)       # two images x three floats; 42 x 42 inputs per 32 x 32 tile
    res["scores_bytes_per_strip_pixel"] = {"algorithmic": img_alg, "addressed_incl_halo": round(img_addr, 2),
                                           "depth_per_pixel_all_views": 12.0}
    moved = S * Wc * img_alg + V * S * S * 12.0
    res["scores_kernels_GBps_algorithmic"] = moved / (res["scores_kernels_event"] * 1e-3) / 1e9

    # (b) turntable
    sc = synthetic.make_scene(grid=64, K=2, regime="trained", seed=0, device=dev)
    gs = (sc["centers"], sc["shs"], sc["opacity"], sc["scales"], sc["rotations"])
    renderer = Renderer(sh_degree=1, white_background=True)
    cams = evaluate.video_cameras(a.frames, "gobjeverse", (S, S), device=dev)

    def turntable_hip():
        return evaluate.render_turntable(renderer, gs, cams, chunk=8)

    def turntable_loop():        # evaluation.py:126-138 as written (the camera's rays built on the device: the reference builds them in numpy)
        imgs, normal_whites = [], []
        with torch.no_grad():
            for cam in cams:
                ixt = fov_to_ixt(torch.tensor((cam.FoVx, cam.FoVy)), (S, S))[None].to(dev)
                rays = build_rays(cam.view_world_transform[None], ixt, S, S)[0]
                o = renderer.render_img(cam, rays, *gs, dev)
                img = np.round(o["image"].cpu().detach().numpy() * 255).astype("uint8")
                alpha = o["acc_map"].reshape(S, S)[..., None]
                nw = np.round((((o["rend_normal"] * alpha + 1 - alpha) + 1) / 2).cpu().detach().numpy() * 255).astype("uint8")
                imgs.append(img)
                normal_whites.append(nw)
        return imgs, normal_whites

    f_hip, n_hip = turntable_hip()
    f_ref, n_ref = turntable_loop()
    res["turntable_frames_equal"] = bool(np.array_equal(f_hip.cpu().numpy(), np.stack(f_ref)) and np.array_equal(n_hip.cpu().numpy(), np.stack(n_ref)))
    steps = max(2, a.steps // 3)
    res["turntable_hip_event"], res["turntable_hip_wall"] = timed(turntable_hip, steps, 1)
    res["turntable_hip_with_host_copy_wall"] = timed(lambda: [t.cpu() for t in turntable_hip()], steps, 1)[1]
    res["turntable_loop_event"], res["turntable_loop_wall"] = timed(turntable_loop, steps, 1)
    line = json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
