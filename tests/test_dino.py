"""The DINO image encoder (lara_amd.dino, include/lara_vit.h) without a GPU: the plain-torch restatement in tests/dino_restate.py
reproduces tests/golden/dino_ref.npz (recorded from transformers' ViTModel), which pins the oracle the GPU tests hold the kernels
to; the position-table resample is timm's; DinoViT keeps timm's parameter names and module types; bad arguments are refused
before anything is launched."""
import ctypes

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from lara_amd._native import load_library
from tests.dino_restate import RestatedViT, fixture_grads, load_fixture


def test_restatement_reproduces_the_transformers_fixture():
    f, images, m, gout = load_fixture()
    out = m(images)
    ref = torch.from_numpy(f["out"])
    assert (out - ref).abs().max() <= 1e-4 * (1 + ref.abs().max())
    (out * gout).sum().backward()
    grads = {n: p.grad for n, p in m.named_parameters()}
    checked = fixture_grads(f, grads)
    assert len(checked) == len(grads) == 4 + 12 * 2 + 2
    for n, got, exp in checked:
        err = (got - exp).abs().max() / (exp.abs().max() + 1e-12)
        assert err <= 1e-4, f"{n}: rel err {err:.2e}"


def test_fixture_attention_is_peaked():
    """The fixture's softmax rows are far from uniform, so a softmax error cannot hide behind flat rows."""
    f, images, m, _ = load_fixture()
    with torch.no_grad():
        x = (images - torch.tensor((0.485, 0.456, 0.406)).view(1, 3, 1, 1)) / torch.tensor((0.229, 0.224, 0.225)).view(1, 3, 1, 1)
        x = m.patch_embed.proj(x).flatten(2).transpose(1, 2)
        x = torch.cat([m.cls_token.expand(x.shape[0], -1, -1), x], 1) + m.pos_embed
        b = m.blocks[0]
        q, k, _ = b.attn.qkv(b.norm1(x)).reshape(x.shape[0], x.shape[1], 3, m.heads, 64).permute(2, 0, 3, 1, 4)
        p = torch.softmax(q @ k.transpose(-1, -2) / 8, -1)
    assert p.max(-1).values.mean() > 0.5


def test_resample_is_antialiased_bicubic_and_identity_at_the_native_grid():
    from lara_amd.dino import resample_pos_embed
    g = torch.Generator().manual_seed(0)
    pos = torch.randn(1, 1 + 14 * 14, 32, generator=g)
    assert resample_pos_embed(pos, (14, 14)) is pos
    out = resample_pos_embed(pos, (32, 20))
    grid = pos[:, 1:].reshape(1, 14, 14, 32).permute(0, 3, 1, 2)
    aa = F.interpolate(grid, size=(32, 20), mode="bicubic", antialias=True, align_corners=False)
    plain = F.interpolate(grid, size=(32, 20), mode="bicubic", antialias=False, align_corners=False)
    assert torch.equal(out[:, :1], pos[:, :1])
    assert torch.equal(out[:, 1:], aa.permute(0, 2, 3, 1).reshape(1, -1, 32))
    assert (aa - plain).abs().max() > 1e-3        # the constant matters: the plain bicubic is a different table
    # the backward is the operator's own gradient, formed as a deterministic product
    gout = torch.randn(1, 1 + 32 * 20, 32, generator=g)
    pos.requires_grad_(True)
    (resample_pos_embed(pos, (32, 20)) * gout).sum().backward()
    ref = pos.detach().clone().requires_grad_(True)
    t = F.interpolate(ref[:, 1:].reshape(1, 14, 14, 32).permute(0, 3, 1, 2), size=(32, 20), mode="bicubic", antialias=True,
                      align_corners=False)
    (torch.cat([ref[:, :1], t.permute(0, 2, 3, 1).reshape(1, -1, 32)], 1) * gout).sum().backward()
    assert torch.allclose(pos.grad, ref.grad, rtol=1e-5, atol=1e-5)


def test_state_dict_keys_are_timm_names_and_round_trip():
    from lara_amd.dino import DinoViT
    torch.manual_seed(0)
    ours = DinoViT(embed_dim=128, depth=2, num_heads=2, mlp_ratio=2.0, img_size=(48, 80))
    ref = RestatedViT(128, 2, 2, 256, (3, 5))
    assert list(ours.state_dict().keys()) == list(ref.state_dict().keys())
    for k, v in ours.state_dict().items():
        assert tuple(v.shape) == tuple(ref.state_dict()[k].shape), k
    ref.load_state_dict(ours.state_dict())
    back = DinoViT(embed_dim=128, depth=2, num_heads=2, mlp_ratio=2.0, img_size=(48, 80))
    back.load_state_dict(ref.state_dict())
    for k, v in back.state_dict().items():
        assert torch.equal(v, ours.state_dict()[k]), k


def _split(module):
    """system.configure_optimizers' rule (lightning/system.py:78-94): LayerNorm parameters and every module's `.bias` get no decay."""
    no_decay = []
    for _, m in module.named_modules():
        if isinstance(m, nn.LayerNorm):
            no_decay.extend(m.parameters())
        elif hasattr(m, "bias") and m.bias is not None:
            no_decay.append(m.bias)
    ids = set(map(id, no_decay))
    names = {id(p): n for n, p in module.named_parameters()}
    return sorted(names[i] for i in ids), sorted(n for n, p in module.named_parameters() if id(p) not in ids)


def test_weight_decay_split_matches_the_restatement():
    from lara_amd.dino import DinoViT
    ours, ref = _split(DinoViT(embed_dim=128, depth=2, num_heads=2)), _split(RestatedViT(128, 2, 2, 512))
    assert ours == ref
    assert "cls_token" in ours[1] and "pos_embed" in ours[1] and "blocks.0.norm1.weight" in ours[0]


def test_from_timm_adopts_the_parameters():
    from lara_amd.dino import DinoViT
    src = DinoViT(embed_dim=128, depth=2, num_heads=2)
    src.blocks[0].attn.num_heads = 2          # what a timm Attention carries
    m = DinoViT.from_timm(src)
    assert all(a is b for a, b in zip(m.parameters(), src.parameters()))


def test_argument_errors_raise_before_any_launch():
    from lara_amd.dino import DinoViT
    with pytest.raises(ValueError):
        DinoViT(embed_dim=100, num_heads=1)                     # C % 64
    with pytest.raises(ValueError):
        DinoViT(embed_dim=768, num_heads=8)                     # head width 96
    m = DinoViT(embed_dim=128, depth=1, num_heads=2)
    with pytest.raises(ValueError):
        m(torch.zeros(1, 3, 40, 48))                            # H % 16
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 3, 32, 48))                            # no CPU path
    with pytest.raises(ValueError):
        m.image_features({"tar_rgb": torch.zeros(1, 4, 40, 48, 3)}, 4)


def test_library_refuses_bad_dims(hip_lib):
    from lara_amd import dino
    lib = load_library()
    ok = dict(N=2, views=1, H=64, W=48, C=128, heads=2, F_=256, depth=2, eps=1e-6, strides=(9216, 0, 3072, 48, 1))
    assert lib.lara_vit_workspace_bytes(ctypes.byref(dino._dims(**ok)), 1) > 0
    assert lib.lara_vit_save_bytes(ctypes.byref(dino._dims(**ok))) > 0
    dummy = ctypes.c_void_p(4096)        # never dereferenced: the argument check comes first
    for bad in (dict(H=40), dict(C=96, heads=1), dict(heads=1), dict(F_=100), dict(views=3), dict(depth=0), dict(eps=0.0),
                dict(H=16 * 200, W=16 * 100)):
        d = dino._dims(**{**ok, **bad})
        assert lib.lara_vit_workspace_bytes(ctypes.byref(d), 1) < 0, bad
        assert lib.lara_vit_forward(ctypes.byref(d), dummy, dummy, dummy, None, dummy, None) == -1, bad
        assert lib.lara_vit_backward(ctypes.byref(d), dummy, dummy, dummy, dummy, dummy, None) == -1, bad


def test_pipeline_without_an_encoder_refuses_forward_from_images():
    from lara_amd.pipeline import LaRaPipeline
    pipe = LaRaPipeline.__new__(LaRaPipeline)
    nn.Module.__init__(pipe)
    pipe.image_encoder, pipe.feat_volume = None, object()
    with pytest.raises(RuntimeError, match="image_encoder"):
        pipe.forward_from_images({})
    pipe.image_encoder, pipe.feat_volume = object(), None
    with pytest.raises(RuntimeError, match="feat_volume"):
        pipe.forward_from_images({})
