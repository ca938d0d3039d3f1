"""Refines a 2DGS ``point_cloud.ply`` -- one `lara_amd.splatio.write_ply` wrote, or one trained by the 2DGS code base -- against
posed views on one MI355X without running any network: `lara_amd.splatrefine.refine` (render, loss, backward, the one-launch sparse
Adam step) for ``--steps`` steps, the refined cloud through `splatio.write_ply`, and a small JSON beside it with the loss and the
PSNR over all views before and after, the step count and the wall time of the loop (ONE run: no spread is measured, and the JSON
says so).

``views.npz`` holds ``images`` [V,H,W,3] (uint8, or float in 0..1), ``c2w`` [V,4,4], and the scalars ``fovx``, ``fovy`` (radians),
``znear``, ``zfar``.  Cameras come from `cameras.make_cameras`, rays from `batch.build_rays`; the background is white.
``--lr KEY=VALUE`` (repeatable; KEY one of centers, sh0, sh_rest, opacity, scales, rotations) replaces a default learning rate;
``--dense`` updates every surfel in every step; ``--regularise-after N`` switches the distortion and normal terms on after N steps.
``--quick``: at most 10 steps (what tests/test_splatrefine_gpu.py runs).
``--densify-from N`` switches densification on (`lara_amd.splatdensify`: clone, split, prune between steps, from step N every
``--densify-interval`` steps until ``--densify-until``); ``--densify-grad-threshold``, ``--densify-percent-dense``,
``--densify-extent`` (the scene's radius), ``--densify-min-opacity``, ``--densify-max-screen-radius``,
``--densify-opacity-reset-interval``, ``--densify-n-split``, ``--densify-max-surfels`` and ``--densify-seed`` are the fields of
`splatdensify.DensifySchedule`; the JSON then lists every round's counts.
    python tools/refine_surfels.py scene.ply views.npz --steps 30 --out refined.ply [--json refined.json] [--quick]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load_views(path, dev):
    """(targets [V,H,W,3] fp32 on the device, cameras, rays) of a views file."""
    from lara_amd import cameras
    from lara_amd.batch import build_rays, fov_to_ixt
    with np.load(path) as z:
        missing = [k for k in ("images", "c2w", "fovx", "fovy", "znear", "zfar") if k not in z.files]
        if missing:
            sys.exit(f"tools/refine_surfels.py: {path} lacks {missing}")
        images, c2w = z["images"], np.asarray(z["c2w"], np.float32)
        fovx, fovy, znear, zfar = (float(z[k]) for k in ("fovx", "fovy", "znear", "zfar"))
    if images.ndim != 4 or images.shape[-1] != 3 or c2w.shape != (images.shape[0], 4, 4):
        sys.exit(f"tools/refine_surfels.py: images is [V,H,W,3] and c2w [V,4,4], got {images.shape} and {c2w.shape}")
    V, H, W = images.shape[:3]
    targets = torch.from_numpy(images).to(dev)
    targets = targets.float() / 255.0 if images.dtype == np.uint8 else targets.float()
    c2w = torch.from_numpy(c2w)
    cams = cameras.make_cameras(c2w, W, H, fovx, fovy, znear, zfar, device=dev)
    ixt = fov_to_ixt(torch.tensor([[fovx, fovy]] * V), (W, H)).to(dev)
    rays = build_rays(c2w.to(dev), ixt, H, W)
    return targets.contiguous(), cams, rays


@torch.no_grad()
def evaluate(renderer, cloud, cams, rays, targets):
    """(loss, mse) of the cloud over all views, as device tensors."""
    from lara_amd import splatrefine
    dev = cloud.device
    out = renderer.render_views(cams, rays, *cloud.render_args(), dev, concat=True)
    loss, stats = splatrefine._default_loss({"tar_rgb": targets[None]}, {k: t[None] for k, t in out.items()}, 0)
    return loss, stats["mse"]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("ply")
    ap.add_argument("views")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", required=True, help="the refined .ply")
    ap.add_argument("--json", default=None, help="the report (default: the output's name with .json)")
    ap.add_argument("--lr", action="append", default=[], metavar="KEY=VALUE")
    ap.add_argument("--dense", action="store_true")
    ap.add_argument("--regularise-after", type=int, default=None)
    ap.add_argument("--quick", action="store_true", help="at most 10 steps")
    ap.add_argument("--densify-from", type=int, default=None, help="densify from this step on (default: never)")
    ap.add_argument("--densify-until", type=int, default=10 ** 9)
    ap.add_argument("--densify-interval", type=int, default=100)
    ap.add_argument("--densify-grad-threshold", type=float, default=2e-4)
    ap.add_argument("--densify-percent-dense", type=float, default=0.01)
    ap.add_argument("--densify-extent", type=float, default=1.0)
    ap.add_argument("--densify-min-opacity", type=float, default=0.005)
    ap.add_argument("--densify-max-screen-radius", type=float, default=0.0)
    ap.add_argument("--densify-opacity-reset-interval", type=int, default=0)
    ap.add_argument("--densify-n-split", type=int, default=2)
    ap.add_argument("--densify-max-surfels", type=int, default=None)
    ap.add_argument("--densify-seed", type=int, default=0)
    args = ap.parse_args()
    if args.quick:
        args.steps = min(args.steps, 10)
    if not torch.cuda.is_available():
        sys.exit("tools/refine_surfels.py needs an MI355X")

    from lara_amd import splatio, splatrefine
    from lara_amd.renderer import Renderer

    lrs = dict(splatrefine.DEFAULT_LRS)
    for item in args.lr:
        key, _, value = item.partition("=")
        if key not in lrs or not value:
            sys.exit(f"tools/refine_surfels.py: --lr takes KEY=VALUE with KEY in {splatrefine.LR_KEYS}, got {item!r}")
        lrs[key] = float(value)

    schedule = None
    if args.densify_from is not None:
        from lara_amd import splatdensify
        schedule = splatdensify.DensifySchedule(
            from_step=args.densify_from, until_step=args.densify_until, interval=args.densify_interval,
            grad_threshold=args.densify_grad_threshold, percent_dense=args.densify_percent_dense, extent=args.densify_extent,
            min_opacity=args.densify_min_opacity, max_screen_radius=args.densify_max_screen_radius,
            opacity_reset_interval=args.densify_opacity_reset_interval, n_split=args.densify_n_split, max_surfels=args.densify_max_surfels,
            seed=args.densify_seed)

    dev = torch.device("cuda", 0)
    cloud, info = splatio.read_ply(args.ply, device=dev)
    targets, cams, rays = load_views(args.views, dev)
    renderer = Renderer(sh_degree=cloud.sh_degree, white_background=True)
    before = evaluate(renderer, cloud, cams, rays, targets)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    refined, history = splatrefine.refine(cloud, cams, rays, targets, steps=args.steps, lrs=lrs, sparse=not args.dense, renderer=renderer,
                                          regularise_after=args.regularise_after, densify=schedule)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    after = evaluate(renderer, refined, cams, rays, targets)
    splatio.write_ply(args.out, refined)

    def psnr(mse):
        return float(-10.0 * torch.log10(mse))
    res = {"ply": os.path.abspath(args.ply), "views": os.path.abspath(args.views), "out": os.path.abspath(args.out),
           "n_surfels": cloud.n_surfels, "sh_degree": cloud.sh_degree, "n_views": len(cams), "height": int(targets.shape[1]),
           "width": int(targets.shape[2]), "steps": args.steps, "sparse": not args.dense, "lrs": lrs,
           "loss_before": float(before[0]), "loss_after": float(after[0]), "psnr_before": psnr(before[1]), "psnr_after": psnr(after[1]),
           "loss_per_step": history["loss"].cpu().tolist(), "non_finite_gradient_words_skipped": int(history["skipped"].item()),
           "dropped_third_scale": info["dropped_third_scale"], "wall_s": wall,
           "wall_note": "the loop's wall time from ONE run, first-launch costs included; no spread was measured"}
    if schedule is not None:
        from lara_amd.splatdensify import COUNT_KEYS
        res["n_surfels_after"] = refined.n_surfels
        res["densify_rounds"] = [dict(zip(COUNT_KEYS, r["counts"].tolist()), step=r["step"], capped=r["capped"]) for r in history["densify"]]
    with open(args.json or os.path.splitext(args.out)[0] + ".json", "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "loss_per_step"}))


if __name__ == "__main__":
    main()
