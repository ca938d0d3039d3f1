"""Times `lara_amd.splatrefine` on one MI355X: HIP events after warm-up, windows of at least 0.1 s, at 524 288 surfels (the headline
cloud), SH degrees 1 and 3.  In the same process, alternating over ``--rounds`` rounds (each round times every variant once, in
turn; min, median and max over the rounds are reported):

  * the one-launch step (``adam_step``), dense and sparse (a seeded mask, half of the rows seen), with and without ``zero_grads``;
  * ``torch.optim.Adam(fused=True)`` over the same five tensors in six parameter groups (the SH tensor split into coefficient 0 and
    the rest: two tensors, which torch needs for two rates), alone and followed by its ``zero_grad(set_to_none=False)``;
  * the device-to-device copy rate, as the neighbouring tools measure it (bytes read + written per second);
  * the share of that rate the dense step reaches over its algorithmic bytes: 7 fp32 words per parameter word (p, g, m, v read; p, m,
    v written), 8 with ``zero_grads``.  The sparse rows are given in ms only: their bytes depend on the mask.

Then one whole ``refine`` step (render, loss, backward, update) at 4 views of 512 x 512 on a synthetic trained cloud of 524 288
surfels, and the same step without the update, so that the update's share of a step is known.
    python tools/splatrefine_bench.py [--quick] [--rounds 5] [--out profiles/splatrefine_bench.json]"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.meshmetrics_bench import timed  # noqa: E402
from tools.meshsimplify_bench import copy_rate  # noqa: E402

WINDOW_S = 0.1


def windowed(fn):
    """ms per call over a window of at least WINDOW_S, after warm-up; (ms, calls in the window)."""
    once = timed(fn, 2, 2)
    steps = max(3, int(math.ceil(1.2 * WINDOW_S * 1e3 / max(once, 1e-3))))
    return timed(fn, steps, 1), steps


def spread(values):
    return {"min": min(values), "median": statistics.median(values), "max": max(values)}


def update_rows(P, degree, dev, rounds, rate):
    from lara_amd import splatrefine as R
    n = (degree + 1) ** 2
    g = torch.Generator(device="cpu").manual_seed(degree)
    shapes = ((3,), (n, 3), (1,), (2,), (4,))
    params = [torch.randn(P, *s, generator=g).to(dev) for s in shapes]
    grads = [(torch.randn(P, *s, generator=g) * 1e-3).to(dev) for s in shapes]
    m, v = [torch.zeros_like(p) for p in params], [torch.zeros_like(p) for p in params]
    visible = (torch.rand(P, generator=g) < 0.5).to(torch.uint8).to(dev)
    counters = torch.zeros(1, dtype=torch.int64, device=dev)
    plan = R.plan(100)
    words = sum(p.numel() for p in params)

    # torch's fused Adam over the same values: six tensors in six groups
    leaves = [params[0].clone(), params[1][:, :1].clone(), params[1][:, 1:].clone(), params[2].clone(), params[3].clone(), params[4].clone()]
    leaf_grads = [grads[0].clone(), grads[1][:, :1].clone(), grads[1][:, 1:].clone(), grads[2].clone(), grads[3].clone(), grads[4].clone()]
    groups = []
    for leaf, gr, key in zip(leaves, leaf_grads, R.LR_KEYS):
        if leaf.numel() == 0:
            continue
        leaf.requires_grad_(True)
        leaf.grad = gr
        groups.append({"params": [leaf], "lr": R.DEFAULT_LRS[key]})
    opt = torch.optim.Adam(groups, betas=(0.9, 0.999), eps=1e-15, fused=True)

    def torch_step_and_zero():
        opt.step()
        opt.zero_grad(set_to_none=False)

    variants = {
        "dense_ms": lambda: R.adam_step(params, grads, m, v, plan, counters=counters),
        "dense_zero_grads_ms": lambda: R.adam_step(params, grads, m, v, plan, zero_grads=True, counters=counters),
        "sparse_ms": lambda: R.adam_step(params, grads, m, v, plan, visible=visible, counters=counters),
        "sparse_zero_grads_ms": lambda: R.adam_step(params, grads, m, v, plan, visible=visible, zero_grads=True, counters=counters),
        "torch_fused_adam_ms": opt.step,
        "torch_fused_adam_plus_zero_grad_ms": torch_step_and_zero,
    }
    times = {k: [] for k in variants}
    calls = {}
    for _ in range(rounds):
        for k, fn in variants.items():                   # alternating: every variant once per round
            ms, calls[k] = windowed(fn)
            times[k].append(ms)
    row = {"P": P, "sh_degree": degree, "parameter_words": words, "rounds": rounds, "calls_in_window": calls,
           **{k: spread(ts) for k, ts in times.items()}}
    for key, per_word in (("dense_ms", 7), ("dense_zero_grads_ms", 8)):
        nbytes = 4 * per_word * words
        ms = row[key]["median"]
        row[key.replace("_ms", "_bytes")] = nbytes
        row[key.replace("_ms", "_GBps")] = nbytes / (ms * 1e-3) / 1e9
        row[key.replace("_ms", "_fraction_of_copy_rate")] = nbytes / (ms * 1e-3) / rate
    row["torch_over_kernel"] = row["torch_fused_adam_ms"]["median"] / row["dense_ms"]["median"]
    row["torch_plus_zero_grad_over_kernel_with_zero_grads"] = (row["torch_fused_adam_plus_zero_grad_ms"]["median"]
                                                                / row["dense_zero_grads_ms"]["median"])
    row["skipped_counter"] = int(counters.item())
    return row


def whole_step(dev, quick, rounds):
    """One refine step at 4 views of 512 x 512 (quick: 64 x 64 of 1 024 surfels), with and without the update."""
    from lara_amd import cameras, splatio, splatrefine as R, synthetic
    from lara_amd.batch import build_rays, fov_to_ixt
    from lara_amd.renderer import Renderer
    size, grid = (64, 8) if quick else (512, 64)
    sc = synthetic.make_scene(grid=grid, K=2, regime="trained", sh_coeffs=4, device=dev)
    cloud = splatio.SurfelCloud(*(sc[k].contiguous() for k in R.FIELDS))
    c2w = cameras.turntable_c2w(4)
    cams = cameras.make_cameras(c2w, size, size, 0.75, 0.75, 0.5, 2.5, device=dev)
    rays = build_rays(c2w.float().to(dev), fov_to_ixt(torch.tensor([[0.75, 0.75]] * 4), (size, size)).to(dev), size, size)
    renderer = Renderer(sh_degree=cloud.sh_degree, white_background=True)
    with torch.no_grad():
        targets = renderer.render_views(cams, rays, *cloud.render_args(), dev, concat=True)["image"]
        targets = targets.reshape(size, 4, size, 3).permute(1, 0, 2, 3).contiguous()
    opt = R.SurfelAdam(cloud, sparse=True)

    def step(update):
        raster_out = []
        out = renderer.render_views(cams, rays, *opt.params(), dev, concat=True, raster_out=raster_out)
        loss, _ = R._default_loss({"tar_rgb": targets[None]}, {k: t[None] for k, t in out.items()}, 0)
        loss.backward()
        if update:
            opt.step((raster_out[0][1] > 0).any(0), zero_grads=True)
        else:
            opt.zero_grad()
            R.bump_version(opt.params())     # (as a step does: the renderer must not replay activations whose graph backward has freed)

    with_update, without = [], []
    for _ in range(rounds):
        with_update.append(windowed(lambda: step(True))[0])
        without.append(windowed(lambda: step(False))[0])
    out = {"P": cloud.n_surfels, "sh_degree": cloud.sh_degree, "views": 4, "size": size, "ms_ssim": size > R.MS_SSIM_MIN,
           "step_ms": spread(with_update), "step_with_zero_grad_in_place_of_the_update_ms": spread(without), "rounds": rounds,
           "skipped_counter": int(opt.skipped.item())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="65 536 surfels, short windows, a 64 x 64 step")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("splatrefine_bench: needs an MI355X")
    global WINDOW_S
    dev = torch.device("cuda:0")
    if a.quick:
        WINDOW_S = 0.005
    P = (1 << 16) if a.quick else (1 << 19)
    rate = copy_rate(dev, (1 << 26) if a.quick else (1 << 30))
    run = {"copy_rate_GBps": rate / 1e9, "window_s": WINDOW_S, "rows": [update_rows(P, d, dev, a.rounds, rate) for d in (1, 3)]}
    run["refine_step"] = whole_step(dev, a.quick, a.rounds)
    by_degree = {r["sh_degree"]: r for r in run["rows"]}
    like = by_degree.get(run["refine_step"]["sh_degree"])
    if like is not None and like["P"] == run["refine_step"]["P"]:
        run["refine_step"]["update_share_of_step"] = like["sparse_zero_grads_ms"]["median"] / run["refine_step"]["step_ms"]["median"]

    def rounded(x):
        if isinstance(x, float):
            return float(f"{x:.6g}")
        if isinstance(x, dict):
            return {k: rounded(v) for k, v in x.items()}
        if isinstance(x, list):
            return [rounded(v) for v in x]
        return x
    run = rounded(run)
    print(json.dumps(run))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(run, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
