"""Plain-torch restatement of timm's ``VisionTransformer.forward_features`` (``dynamic_img_size=True``) behind torchvision's
ImageNet ``Normalize``: what ``DinoWrapper`` (lightning/network.py:14-55) runs.  Shared by tests/test_dino.py, tests/test_dino_gpu.py
and tools/dino_bench.py.  Run it under ``torch.autocast(dtype=torch.bfloat16)`` for the precision LaRa trains in
(train_lightning.py:76): the patch conv, every Linear, GELU and SDPA then run in bf16, LayerNorm in fp32, and the residual stream
stays fp32 (``cat(cls, x)`` and ``+ pos_embed`` promote).

The reference's own encoder cannot run here (no timm, no weights): this restatement is pinned by tests/golden/dino_ref.npz, recorded
from ``transformers.ViTModel`` (tests/golden/make_dino_fixture.py), and by timm's documented semantics."""
import os

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def resample(pos, new_grid, old_grid):
    """timm ``resample_abs_pos_embed`` with one prefix token: bicubic, antialiased, fp32; unchanged at the table's own grid."""
    if tuple(new_grid) == tuple(old_grid):
        return pos
    (h, w), (gh, gw) = new_grid, old_grid
    table = pos[:, 1:].float().reshape(1, gh, gw, -1).permute(0, 3, 1, 2)
    table = F.interpolate(table, size=(h, w), mode="bicubic", antialias=True, align_corners=False)
    return torch.cat([pos[:, :1], table.permute(0, 2, 3, 1).reshape(1, h * w, -1).to(pos.dtype)], dim=1)


class _NS(nn.Module):
    def __init__(self, **kw):
        super().__init__()
        for k, v in kw.items():
            setattr(self, k, v)


class RestatedViT(nn.Module):
    """timm parameter names: cls_token, pos_embed, patch_embed.proj, blocks.{i}.{norm1, attn.qkv, attn.proj, norm2, mlp.fc1,
    mlp.fc2}, norm."""

    def __init__(self, C=768, depth=12, heads=12, F_=3072, grid=(14, 14), eps=1e-6):
        super().__init__()
        self.heads, self.grid = heads, tuple(grid)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, C))
        self.pos_embed = nn.Parameter(torch.zeros(1, 1 + grid[0] * grid[1], C))
        self.patch_embed = _NS(proj=nn.Conv2d(3, C, 16, 16))
        self.blocks = nn.ModuleList([_NS(norm1=nn.LayerNorm(C, eps=eps), attn=_NS(qkv=nn.Linear(C, 3 * C), proj=nn.Linear(C, C)),
                                         norm2=nn.LayerNorm(C, eps=eps), mlp=_NS(fc1=nn.Linear(C, F_), fc2=nn.Linear(F_, C)))
                                     for _ in range(depth)])
        self.norm = nn.LayerNorm(C, eps=eps)

    def forward(self, images):
        """images [N, 3, H, W] in [0, 1] -> [N, hw, C] (DinoWrapper.forward)."""
        dev = images.device
        x = (images - torch.tensor(MEAN, device=dev).view(1, 3, 1, 1)) / torch.tensor(STD, device=dev).view(1, 3, 1, 1)
        x = self.patch_embed.proj(x)
        N, C, h, w = x.shape
        x = x.permute(0, 2, 3, 1).reshape(N, h * w, C)
        x = torch.cat([self.cls_token.expand(N, -1, -1), x], dim=1)
        x = x + resample(self.pos_embed, (h, w), self.grid)
        T = x.shape[1]
        for b in self.blocks:
            qkv = b.attn.qkv(b.norm1(x)).reshape(N, T, 3, self.heads, C // self.heads).permute(2, 0, 3, 1, 4)
            a = F.scaled_dot_product_attention(qkv[0], qkv[1], qkv[2])
            x = x + b.attn.proj(a.transpose(1, 2).reshape(N, T, C))
            x = x + b.mlp.fc2(F.gelu(b.mlp.fc1(b.norm2(x))))
        return self.norm(x)[:, 1:]


def bf16_bits_to_f32(a):
    return torch.from_numpy((a.astype(np.uint32) << 16).view(np.float32).copy())


def load_fixture(device="cpu"):
    """-> (npz, images [N, 3, H, W], RestatedViT with the fixture's weights, gout [N, hw, C])."""
    f = np.load(os.path.join(HERE, "golden", "dino_ref.npz"))
    C, depth, heads, F_, H, W = (int(v) for v in f["config"])
    m = RestatedViT(C, depth, heads, F_, (H // 16, W // 16)).to(device)
    with torch.no_grad():
        for n, p in m.named_parameters():
            p.copy_(bf16_bits_to_f32(f["w:" + n]).reshape(p.shape))
    images = torch.from_numpy(f["images_u8"].astype(np.float32) / 255.0).to(device)
    return f, images, m, bf16_bits_to_f32(f["gout_bf16"]).to(device)


def fixture_grads(f, grads):
    """[(name, got, expected)] over what the fixture records: the whole gradient of a small tensor, sampled entries of a large one."""
    out = []
    for n, g in grads.items():
        flat = g.reshape(-1).float().cpu()
        if "g:" + n in f.files:
            out.append((n, flat, torch.from_numpy(f["g:" + n])))
        else:
            out.append((n, flat[torch.from_numpy(f["gi:" + n].astype(np.int64))], torch.from_numpy(f["gs:" + n])))
    return out
