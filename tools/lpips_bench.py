"""Times `lara_amd.lpips` on one MI355X, with HIP events after warm-up, for one scene at the evaluation's own size (512^2, 4 novel
views: render and target strips of 512 x 2048), both networks, seeded random weights (tests/lpips_restate.py):
  (a) `lpips_device` per scene and net (the in-place route: 2 images through every launch);
  (b) the same networks as torch modules with the same weights (fp32 `F.conv2d`, channels-first, on the permuted cropped copies the
      callable route of `Evaluator` makes): what a user's own callable cost before;
  (c) every convolution alone through `conv2d_nhwc` at its shape in the network: achieved TFLOP/s and the fraction of the
      157.3 TFLOP/s fp32 matrix peak, beside `F.conv2d` on the same shape;
  (d) workspace bytes.
Prints one JSON line.
    python tools/lpips_bench.py [--steps 5] [--warmup 2] [--out profiles/lpips_bench.json]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TFLOPS = 157.3


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--views", type=int, default=4, help="novel views (as many input views are cropped away)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from lara_amd import lpips as L
    from tests import lpips_restate as R

    dev = torch.device("cuda:0")
    H = W = args.size
    V, skip = 2 * args.views, args.views
    g = torch.Generator().manual_seed(0)
    tar = torch.rand(1, V, H, W, 3, generator=g).to(dev)
    img = (tar.permute(0, 2, 1, 3, 4).reshape(1, H, V * W, 3) + 0.1 * torch.randn(1, H, V * W, 3, generator=g).to(dev)).clamp(0, 1).contiguous()
    Wc = (V - skip) * W
    result = {"size": [H, Wc], "steps": args.steps, "warmup": args.warmup, "peak_tflops": PEAK_TFLOPS, "nets": {}}
    for net in ("vgg", "alex"):
        sd = R.make_state_dict(net, 1)
        m = L.LPIPS.from_state_dict(net, sd).to(dev)
        sd_dev = {k: v.to(dev) for k, v in sd.items()}
        hip_ms = timed(lambda: L.lpips_device([m], img, tar, skip), args.steps, args.warmup)

        def torch_route():
            x = img[0].permute(2, 0, 1)[None][..., W * skip:] * 2 - 1
            y = tar[0].permute(1, 0, 2, 3).reshape(img[0].shape).permute(2, 0, 1)[None][..., W * skip:] * 2 - 1
            return R.lpips(net, sd_dev, y, x, dtype=torch.float32)[1]
        torch_ms = timed(torch_route, args.steps, args.warmup)
        got = float(L.lpips_device([m], img, tar, skip)[0, 0, 5])
        layers, h, w = [], H, Wc
        for (ci, co, k, s, p, pk, ps, tap, key) in L.LAYERS[net]:
            if pk:
                h, w = (h - pk) // ps + 1, (w - pk) // ps + 1
            x = torch.randn(2, h, w, ci, generator=g).to(dev)
            wt, b = sd[f"net.slice{key[0]}.{key[1]}.weight"].to(dev), sd[f"net.slice{key[0]}.{key[1]}.bias"].to(dev)
            packed = L.repack(wt)
            ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
            flop = 2.0 * 2 * ho * wo * co * ci * k * k
            ms = timed(lambda: L.conv2d_nhwc(x, packed, b, s, p, True), args.steps, args.warmup)
            xc = x.permute(0, 3, 1, 2).contiguous()
            ms_t = timed(lambda: F.relu(F.conv2d(xc, wt, b, stride=s, padding=p)), args.steps, args.warmup)
            layers.append({"conv": f"{ci}->{co} k{k} s{s} p{p} @ {h}x{w}", "gflop": flop / 1e9, "hip_ms": ms, "hip_tflops": flop / ms / 1e9,
                           "fraction_of_peak": flop / ms / 1e9 / PEAK_TFLOPS, "torch_ms": ms_t, "torch_tflops": flop / ms_t / 1e9})
            del x, xc
            h, w = ho, wo
        result["nets"][net] = {"hip_ms_per_scene": hip_ms, "torch_ms_per_scene": torch_ms, "score": got,
                               "workspace_bytes": m.workspace_bytes(1, H, Wc), "conv_gflop": sum(l["gflop"] for l in layers),
                               "worst_fraction_of_peak": min(l["fraction_of_peak"] for l in layers[1:]), "layers": layers}
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
