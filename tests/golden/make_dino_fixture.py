"""Records tests/golden/dino_ref.npz, the fixture that pins tests/dino_restate.py (the DINO encoder's oracle) independently of it.

The reference's `DinoWrapper` needs timm and pretrained weights, neither of which is available, so the fixture comes from a small
`transformers.ViTModel` -- an independent implementation of the same architecture -- with seeded weights mapped to timm's names
(q / k / v -> `qkv`, `o_proj` -> `proj`, layernorm_before / _after -> norm1 / norm2).  Config: width 128, 2 heads, 2 blocks, MLP
width 256 (the file must stay under 1 MB), eps 1e-6, exact GELU, a 48 x 80 image at the model's own grid (no resampling).  The
images are normalised as torchvision's Normalize does before the model sees them.

Stored: the weights (bf16-exact, as 16-bit patterns), the images (uint8 / 255), the output tokens [N, hw, C], and the gradients
of sum(out * gout) (gout bf16-exact): whole for tensors of at most 8192 entries, 1024 seeded entries of each larger one.

    python tests/golden/make_dino_fixture.py      (needs transformers; CPU, fp32)"""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
C, DEPTH, HEADS, FF, H, W, N = 128, 2, 2, 256, 48, 80, 2
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def bf16(t):
    return t.to(torch.bfloat16).float()


def bits(t):
    return (bf16(t).contiguous().view(torch.int32) >> 16).numpy().astype(np.uint16)


def main():
    from transformers import ViTConfig, ViTModel
    cfg = ViTConfig(hidden_size=C, num_hidden_layers=DEPTH, num_attention_heads=HEADS, intermediate_size=FF, hidden_act="gelu",
                    layer_norm_eps=1e-6, image_size=(H, W), patch_size=16, num_channels=3, qkv_bias=True,
                    hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    cfg._attn_implementation = "eager"
    model = ViTModel(cfg, add_pooling_layer=False).eval()
    g = torch.Generator().manual_seed(0)
    rn = lambda *s: torch.randn(*s, generator=g)
    emb = model.embeddings
    with torch.no_grad():
        emb.cls_token.copy_(bf16(rn(1, 1, C)))
        emb.position_embeddings.copy_(bf16(rn(*emb.position_embeddings.shape) * 0.5))
        emb.patch_embeddings.projection.weight.copy_(bf16(rn(C, 3, 16, 16) * 768 ** -0.5))
        emb.patch_embeddings.projection.bias.copy_(bf16(rn(C) * 0.1))
        for layer in model.layers:
            a = layer.attention
            for lin in (a.q_proj, a.k_proj, a.v_proj):     # logits of std ~ 3: peaked attention
                lin.weight.copy_(bf16(rn(C, C) * (3.0 / C) ** 0.5)); lin.bias.copy_(bf16(rn(C) * 0.1))
            a.o_proj.weight.copy_(bf16(rn(C, C) * C ** -0.5)); a.o_proj.bias.copy_(bf16(rn(C) * 0.1))
            layer.mlp.fc1.weight.copy_(bf16(rn(FF, C) * C ** -0.5)); layer.mlp.fc1.bias.copy_(bf16(rn(FF) * 0.1))
            layer.mlp.fc2.weight.copy_(bf16(rn(C, FF) * FF ** -0.5)); layer.mlp.fc2.bias.copy_(bf16(rn(C) * 0.1))
            for ln in (layer.layernorm_before, layer.layernorm_after):
                ln.weight.copy_(bf16(1 + rn(C) * 0.1)); ln.bias.copy_(bf16(rn(C) * 0.1))
        model.layernorm.weight.copy_(bf16(1 + rn(C) * 0.1)); model.layernorm.bias.copy_(bf16(rn(C) * 0.1))
    images_u8 = torch.randint(0, 256, (N, 3, H, W), generator=g, dtype=torch.uint8)
    images = images_u8.float() / 255.0
    pixel = (images - torch.tensor(MEAN).view(1, 3, 1, 1)) / torch.tensor(STD).view(1, 3, 1, 1)
    out = model(pixel_values=pixel).last_hidden_state[:, 1:]
    gout = bf16(rn(*out.shape))
    (out * gout).sum().backward()

    # timm names -> (tensor, gradient)
    named = {"cls_token": emb.cls_token, "pos_embed": emb.position_embeddings,
             "patch_embed.proj.weight": emb.patch_embeddings.projection.weight,
             "patch_embed.proj.bias": emb.patch_embeddings.projection.bias}
    cat = lambda ts: (torch.cat([t.detach() for t in ts]), torch.cat([t.grad for t in ts]))
    rec = {}
    for i, layer in enumerate(model.layers):
        a, p = layer.attention, f"blocks.{i}."
        rec[p + "attn.qkv.weight"] = cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight])
        rec[p + "attn.qkv.bias"] = cat([a.q_proj.bias, a.k_proj.bias, a.v_proj.bias])
        for name, t in (("norm1.weight", layer.layernorm_before.weight), ("norm1.bias", layer.layernorm_before.bias),
                        ("attn.proj.weight", a.o_proj.weight), ("attn.proj.bias", a.o_proj.bias),
                        ("norm2.weight", layer.layernorm_after.weight), ("norm2.bias", layer.layernorm_after.bias),
                        ("mlp.fc1.weight", layer.mlp.fc1.weight), ("mlp.fc1.bias", layer.mlp.fc1.bias),
                        ("mlp.fc2.weight", layer.mlp.fc2.weight), ("mlp.fc2.bias", layer.mlp.fc2.bias)):
            named[p + name] = t
    named["norm.weight"], named["norm.bias"] = model.layernorm.weight, model.layernorm.bias
    for k, t in named.items():
        rec[k] = (t.detach(), t.grad)

    rng = np.random.default_rng(0)
    arrays = {"config": np.array([C, DEPTH, HEADS, FF, H, W], dtype=np.int32), "images_u8": images_u8.numpy(),
              "out": out.detach().numpy().astype(np.float32), "gout_bf16": bits(gout)}
    for k, (w, gr) in rec.items():
        arrays["w:" + k] = bits(w)
        gr = gr.reshape(-1).numpy().astype(np.float32)
        if gr.size <= 8192:
            arrays["g:" + k] = gr
        else:
            idx = np.sort(rng.choice(gr.size, 1024, replace=False)).astype(np.int32)
            arrays["gi:" + k], arrays["gs:" + k] = idx, gr[idx]
    path = os.path.join(HERE, "dino_ref.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
