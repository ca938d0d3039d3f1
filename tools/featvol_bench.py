"""Times the image-feature volume stage (network.py:352-379 + :448-452) at full size -- B = 4 scenes, V = 4 views, 512^2 inputs,
a 32 x 32 x 768 DINO map, R = 16 -- with HIP events, forward and forward + backward, for
  torch:  the reference arithmetic as torch operators under bf16 autocast, then the encoder's cond transpose (layout b);
  hip:    FeatureVolume (layout a, fp32 [B, V, 800, 16, 16, 16]);
  fused:  the feature-volume kernels writing the encoder's bf16 operand directly (layout b) and their backward from dcond;
and the whole step from the image features (forward_from_image_features + lara_loss + backward) against torch build_feat_vol +
pipe(batch, feat_vol).  Prints one JSON line.  Needs an MI355X.
    python tools/featvol_bench.py [--steps 20] [--warmup 3] [--no-step]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-step", action="store_true", help="the stage only, not the whole step")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("featvol_bench: needs an MI355X")
    from lara_amd.batch import synthetic_batch
    from lara_amd._native import current_stream as _stream, load_library as enc_lib
    from lara_amd.featvol import TOKENS, FeatureVolume
    from tests.featvol_restate import restated
    dev = torch.device("cuda:0")
    B, V, C, E, R, h = 4, 4, 768, 32, 16, 32
    torch.manual_seed(0)
    batch = synthetic_batch(batch_size=B, n_views=V, H=512, W=512, n_input=4, seed=0, device=dev)
    fv = FeatureVolume(C=C, E=E, R=R).to(dev)
    x = torch.einsum("blc->bcl", torch.randn(B * V, h * h, C, device=dev)).reshape(B * V, C, h, h).requires_grad_(True)
    S, CE = R ** 3, C + E
    n, lin = fv.dir_norm.norm, fv.dir_norm.mlp[1]

    def torch_fwd():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            vol = restated(batch, x, n.weight, n.bias, lin.weight, lin.bias, fv.view_embed, R, (512, 512), V, bf16=True)
        cond = torch.empty(B * S, V, CE, dtype=torch.bfloat16, device=dev)
        v = vol.detach().contiguous()
        enc_lib().lara_batched_transpose(B, V * CE, S, v.data_ptr(), cond.data_ptr(), 1, _stream(dev))
        return vol, cond

    def torch_fb():
        vol, _ = torch_fwd()
        g = torch.empty(B * S, V, CE, device=dev).normal_()
        gv = torch.empty_like(vol)
        enc_lib().lara_batched_transpose(B, S, V * CE, g.data_ptr(), gv.data_ptr(), 0, _stream(dev))
        vol.backward(gv)

    def hip_fb():
        fv(batch, x, V).backward(torch.ones(B, V, CE, R, R, R, device=dev))

    dcond = torch.randn(B * S, V, CE, device=dev)

    def fused_fwd():
        prep = fv.prepare(batch, x, V)
        prep.params(*fv._args(V))
        return prep, prep.forward(TOKENS)

    def fused_fb():
        prep, _ = fused_fwd()
        prep.backward(dcond, TOKENS)

    res = {"shape": {"B": B, "V": V, "C": C, "E": E, "R": R, "map": [h, h], "image": [512, 512]}, "unit": "ms"}
    res["torch_fwd"] = timed(lambda: torch_fwd(), a.steps, a.warmup)
    res["torch_fwd_bwd"] = timed(torch_fb, a.steps, a.warmup)
    with torch.no_grad():
        res["hip_fwd"] = timed(lambda: fv(batch, x, V), a.steps, a.warmup)
    res["hip_fwd_bwd"] = timed(hip_fb, a.steps, a.warmup)
    res["fused_fwd"] = timed(lambda: fused_fwd(), a.steps, a.warmup)
    res["fused_fwd_bwd"] = timed(fused_fb, a.steps, a.warmup)
    if not a.no_step:
        from lara_amd.encoder_train import VolTransformer
        from lara_amd.pipeline import CoarseFineDecoder, LaRaPipeline, lara_loss
        enc = VolTransformer(embed_dim=256, image_feat_dim=CE, n_groups=[16], vol_low_res=32, vol_high_res=64, out_dim=80,
                             num_layers=12, num_heads=16).to(dev)
        pipe = LaRaPipeline(enc, CoarseFineDecoder(), grid_reso=32, n_streams=2, feat_volume=fv).to(dev)
        pipe.fine_mask = "plain"

        def step_fused():
            out = pipe.forward_from_image_features(batch, x)
            lara_loss(batch, out, ms_ssim=False)[0].backward()
            pipe.join_streams()

        def step_torch():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                vol = restated(batch, x, n.weight, n.bias, lin.weight, lin.bias, fv.view_embed, R, (512, 512), V, bf16=True)
            out = pipe(batch, vol.float())
            lara_loss(batch, out, ms_ssim=False)[0].backward()
            pipe.join_streams()

        res["step_fused"] = timed(step_fused, max(3, a.steps // 4), a.warmup)
        res["step_torch"] = timed(step_torch, max(3, a.steps // 4), a.warmup)
    print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
