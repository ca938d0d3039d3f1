"""Times the DINO image encoder (lightning/network.py:14-55) at LaRa's size -- B = 4 scenes x 4 views of 512^2, ViT-B/16 (C = 768,
12 blocks, 1025 tokens per image) -- with HIP events, forward and forward + backward, for
  torch:  the restatement (tests/dino_restate.py) under bf16 autocast: SDPA and hipBLASLt products;
  hip:    lara_amd.dino.DinoViT (csrc/vit.hip);
with TFLOP/s (matrix FLOPs from the shapes; forward + backward counted as 3x the forward) and the fraction of the bf16 dense peak,
the split of one HIP forward + backward by kernel class (products, attention, LayerNorm, elementwise; HIP events around every
launch), and the whole step from the images (forward_from_images + lara_loss + backward) against torch DINO +
forward_from_image_features.  Prints one JSON line.  Needs an MI355X.
    python tools/dino_bench.py [--steps 10] [--warmup 2] [--no-step]"""
import argparse
import json
import os
import sys
from collections import defaultdict

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BF16_PEAK_TFLOPS = 2500.0      # MI355X dense bf16 (MI355X_MICROARCH: ~2.5 PF)


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


def vit_flops(N, T, C, F, depth):
    hw = T - 1
    per_block = 2 * T * C * (3 * C + C + 2 * F) + 4 * T * T * C
    return N * (2 * hw * 768 * C + depth * per_block)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-step", action="store_true", help="the encoder only, not the whole step")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dino_bench: needs an MI355X")
    from lara_amd import rasterizer
    from lara_amd.batch import synthetic_batch
    from lara_amd.dino import DinoViT
    from tests.dino_restate import RestatedViT
    dev = torch.device("cuda:0")
    B, V, C, depth, heads, S = 4, 4, 768, 12, 12, 512
    N, T = B * V, 1 + (S // 16) ** 2
    torch.manual_seed(0)
    enc = DinoViT(embed_dim=C, depth=depth, num_heads=heads).to(dev)
    ref = RestatedViT(C, depth, heads, 4 * C).to(dev)
    ref.load_state_dict(enc.state_dict())
    batch = synthetic_batch(batch_size=B, n_views=V, H=S, W=S, n_input=4, seed=0, device=dev)
    batch["tar_rgb"] = torch.rand(batch["tar_rgb"].shape, device=dev)
    images = batch["tar_rgb"][:, :V].reshape(N, S, S, 3).permute(0, 3, 1, 2)
    gout = torch.randn(N, T - 1, C, device=dev)

    def torch_fwd():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return ref(images)

    def torch_fb():
        torch_fwd().float().backward(gout)

    def hip_fb():
        enc(images).backward(gout)

    fl = vit_flops(N, T, C, 4 * C, depth)
    res = {"shape": {"images": N, "size": [S, S], "C": C, "blocks": depth, "tokens": T}, "unit": "ms",
           "tflop_fwd": round(fl / 1e12, 3), "tflop_fwd_bwd": round(3 * fl / 1e12, 3)}
    with torch.no_grad():
        res["torch_fwd"] = timed(torch_fwd, a.steps, a.warmup)
        res["hip_fwd"] = timed(lambda: enc(images), a.steps, a.warmup)
    res["torch_fwd_bwd"] = timed(torch_fb, a.steps, a.warmup)
    res["hip_fwd_bwd"] = timed(hip_fb, a.steps, a.warmup)
    for k in ("torch_fwd", "hip_fwd", "torch_fwd_bwd", "hip_fwd_bwd"):
        f = fl * (3 if k.endswith("bwd") else 1)
        tf = f / (res[k] * 1e-3) / 1e12
        res[k + "_tflops"] = round(tf, 1)
        res[k + "_peak_frac"] = round(tf / BF16_PEAK_TFLOPS, 3)

    # split of one HIP forward + backward (events around every launch: slower than the plain run, shares only)
    torch.cuda.synchronize()
    rasterizer.profile_collect()
    rasterizer.profile_enable(True)
    hip_fb()
    torch.cuda.synchronize()
    rec = rasterizer.profile_collect()
    rasterizer.profile_enable(False)
    split = defaultdict(float)
    for name, ms in rec:
        if name.startswith("vit_"):
            split[name[4:]] += ms
    res["hip_fwd_bwd_split_ms"] = {k: round(v, 2) for k, v in sorted(split.items())}

    if not a.no_step:
        from lara_amd.encoder_train import VolTransformer
        from lara_amd.featvol import FeatureVolume
        from lara_amd.pipeline import CoarseFineDecoder, LaRaPipeline, lara_loss
        vt = VolTransformer(embed_dim=256, image_feat_dim=C + 32, n_groups=[16], vol_low_res=32, vol_high_res=64, out_dim=80,
                            num_layers=12, num_heads=16).to(dev)
        fv = FeatureVolume(C=C, E=32, R=16).to(dev)
        pipe = LaRaPipeline(vt, CoarseFineDecoder(), grid_reso=32, n_streams=2, feat_volume=fv, image_encoder=enc).to(dev)
        pipe.fine_mask = "plain"
        h = S // 16

        def step_hip():
            out = pipe.forward_from_images(batch)
            lara_loss(batch, out, ms_ssim=False)[0].backward()
            pipe.join_streams()

        def step_torch():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                tok = ref(images)
            feats = tok.float().transpose(1, 2).reshape(N, C, h, h)
            out = pipe.forward_from_image_features(batch, feats)
            lara_loss(batch, out, ms_ssim=False)[0].backward()
            pipe.join_streams()

        res["step_from_images_hip"] = timed(step_hip, max(3, a.steps // 2), a.warmup)
        res["step_from_images_torch_dino"] = timed(step_torch, max(3, a.steps // 2), a.warmup)
    print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
