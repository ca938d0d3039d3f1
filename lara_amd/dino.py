"""LaRa's DINO image encoder on the HIP kernels of ``liblara2dgs.so`` (csrc/vit.hip, include/lara_vit.h).

``DinoViT`` is ``DinoWrapper`` (lightning/network.py:14-55): timm's ``vit_base_patch16_224.dino`` built with
``dynamic_img_size=True``, torchvision's ``Normalize`` with the ImageNet mean and std in front, ``forward_features(...)[:, 1:]``
behind.  It mirrors the model as it trains under bf16 autocast (train_lightning.py:76).  The parameters keep timm's names and
live in real ``nn.Conv2d`` / ``nn.Linear`` / ``nn.LayerNorm`` modules, so ``load_state_dict(net.img_encoder.model.state_dict())``
loads a LaRa checkpoint's encoder and ``system.configure_optimizers`` splits weight decay the same way.

The whole encoder is one autograd node.  Its backward writes every parameter gradient in fp32 and is bit-reproducible (no float
atomics).  Under ``no_grad`` / ``inference_mode`` (or with every parameter frozen) the inference form keeps nothing.  The position
table is resampled to the token grid in torch (``resample_pos_embed``, timm's ``resample_abs_pos_embed``), so its gradient flows
through the resample.

There is no CPU path and no torch fallback: tensors must live on the GPU and the library must load.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from ._native import VitDims as _Dims, alloc_bytes, call, host_array, query, require_device
from ._native import load_library as _lib  # noqa: F401  (the shared loader; this name was imported from here)

PATCH, HEAD_DIM, MAX_C, MAX_F, MAX_T = 16, 64, 1024, 4096, 16384
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def resample_pos_embed(pos_embed: torch.Tensor, new_size: tuple, old_size: tuple = None, num_prefix_tokens: int = 1) -> torch.Tensor:
    """timm's ``resample_abs_pos_embed``: [1, prefix + gh * gw, C] -> [1, prefix + h * w, C] (``old_size`` = (gh, gw), square by
    default).  The prefix rows are kept, the grid is resampled with ``F.interpolate(mode='bicubic', antialias=True,
    align_corners=False)`` in fp32, and the table is returned unchanged at its own grid.  (torch's antialiased bicubic uses the
    kernel constant a = -0.5, the plain one a = -0.75.)"""
    h, w = int(new_size[0]), int(new_size[1])
    n_old = pos_embed.shape[1] - num_prefix_tokens
    if old_size is None:
        g = int(round(n_old ** 0.5))
        old_size = (g, g)
    gh, gw = int(old_size[0]), int(old_size[1])
    if gh * gw != n_old:
        raise ValueError(f"pos_embed holds {n_old} grid positions, not {gh} x {gw}")
    if (h, w) == (gh, gw):
        return pos_embed
    prefix, table = pos_embed[:, :num_prefix_tokens], pos_embed[:, num_prefix_tokens:]
    dtype = table.dtype
    table = table.float().reshape(1, gh, gw, -1).permute(0, 3, 1, 2)
    table = _Resample.apply(table, (h, w))
    table = table.permute(0, 2, 3, 1).reshape(1, h * w, -1).to(dtype)
    return torch.cat([prefix, table], dim=1)


_axis_cache = {}


def _axis_matrix(n_in, n_out, device):
    """[n_out, n_in]: the antialiased bicubic resample along one axis, read off torch's own operator (it is separable, and the
    other axis at its own size is the identity).  (A 1-wide probe does not work: a 1-pixel axis takes another path.)"""
    key = (n_in, n_out, str(device))
    if key not in _axis_cache:
        eye = torch.eye(n_in, device=device)[None, None]
        _axis_cache[key] = F.interpolate(eye, size=(n_out, n_in), mode="bicubic", antialias=True, align_corners=False)[0, 0]
    return _axis_cache[key]


class _Resample(torch.autograd.Function):
    """``F.interpolate(bicubic, antialias=True)`` forward (timm's values bit for bit); backward as the transposed separable
    product, Ah^T g Aw -- two matrix products in a fixed order instead of the operator's atomic scatter, so that the position
    table's gradient is bit-reproducible like the rest of the encoder's."""

    @staticmethod
    def forward(ctx, table, size):
        ctx.grid = table.shape[2:]
        return F.interpolate(table, size=size, mode="bicubic", antialias=True, align_corners=False)

    @staticmethod
    def backward(ctx, g):
        (gh, gw), (h, w) = ctx.grid, g.shape[2:]
        ah, aw = _axis_matrix(gh, h, g.device), _axis_matrix(gw, w, g.device)
        return torch.matmul(torch.matmul(ah.t(), g.float()), aw), None


class _PatchEmbed(nn.Module):
    def __init__(self, C):
        super().__init__()
        self.proj = nn.Conv2d(3, C, kernel_size=PATCH, stride=PATCH)


class _Attention(nn.Module):
    def __init__(self, C):
        super().__init__()
        self.qkv = nn.Linear(C, 3 * C)
        self.proj = nn.Linear(C, C)


class _Mlp(nn.Module):
    def __init__(self, C, F_):
        super().__init__()
        self.fc1 = nn.Linear(C, F_)
        self.fc2 = nn.Linear(F_, C)


class _Block(nn.Module):
    def __init__(self, C, F_, eps):
        super().__init__()
        self.norm1 = nn.LayerNorm(C, eps=eps)
        self.attn = _Attention(C)
        self.norm2 = nn.LayerNorm(C, eps=eps)
        self.mlp = _Mlp(C, F_)


def _dims(N, views, H, W, C, heads, F_, depth, eps, strides):
    d = _Dims()
    d.N, d.views, d.H, d.W, d.C, d.heads, d.F, d.depth = N, views, H, W, C, heads, F_, depth
    d.eps = float(eps)
    for i, s in enumerate(strides):
        d.img_stride[i] = int(s)
    return d


class _Run:
    """One call of the kernels: the dims, the flattened fp32 parameters (lara_vit.h order) and the saved state."""

    def __init__(self, d, images, params, dev):
        self.d, self.images, self.params, self.dev = d, images, params, dev
        self.ptrs = host_array("p", params)
        self.save = None

    def forward(self, training):
        d = self.d
        hw = (d.H // PATCH) * (d.W // PATCH)
        out = torch.empty(d.N, hw, d.C, dtype=torch.float32, device=self.dev)
        ws = alloc_bytes(query("lara_vit_workspace_bytes", d, 1 if training else 0), self.dev)
        self.save = alloc_bytes(query("lara_vit_save_bytes", d), self.dev) if training else None
        call("lara_vit_forward", self.dev, d, self.images, self.ptrs, out, self.save, ws)
        return out

    def backward(self, grad):
        d = self.d
        grad = grad.float().contiguous()
        grads = [torch.empty_like(p) for p in self.params]
        ws = alloc_bytes(query("lara_vit_workspace_bytes", d, 1), self.dev)
        gptrs = host_array("p", grads)
        call("lara_vit_backward", self.dev, d, self.ptrs, self.save, grad, gptrs, ws)
        return grads


class _VitFn(torch.autograd.Function):
    """(run, images (no gradient), *parameters in lara_vit.h order) -> tokens [N, hw, C]."""

    @staticmethod
    def forward(ctx, run, images, *params):
        ctx.run = run
        return run.forward(training=True)

    @staticmethod
    def backward(ctx, g):
        grads = ctx.run.backward(g)
        ctx.run = None
        return (None, None) + tuple(grads)


class DinoViT(nn.Module):
    """timm ``VisionTransformer`` (class token, absolute position table at ``img_size`` / 16, pre-norm blocks, final norm, no
    head) with ``dynamic_img_size``, behind torchvision's ImageNet ``Normalize``.  Defaults: ViT-B/16 (DINO's).  ``img_size``:
    an int or (H, W), the grid of the position table."""

    def __init__(self, embed_dim: int = 768, depth: int = 12, num_heads: int = 12, mlp_ratio: float = 4.0, img_size=224,
                 eps: float = 1e-6):
        super().__init__()
        C, F_ = int(embed_dim), int(round(embed_dim * mlp_ratio))
        if C % 64 or not 64 <= C <= MAX_C:
            raise ValueError(f"lara_amd.dino: embed_dim {C} must be a multiple of 64 in [64, {MAX_C}]")
        if C != HEAD_DIM * num_heads:
            raise ValueError(f"lara_amd.dino: the head width must be {HEAD_DIM}; embed_dim {C} / num_heads {num_heads} is not")
        if F_ % 64 or not 64 <= F_ <= MAX_F:
            raise ValueError(f"lara_amd.dino: the MLP width {F_} must be a multiple of 64 in [64, {MAX_F}]")
        self.C, self.F, self.depth, self.num_heads, self.eps = C, F_, int(depth), int(num_heads), float(eps)
        ih, iw = (img_size, img_size) if isinstance(img_size, int) else img_size
        self.grid = (ih // PATCH, iw // PATCH)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, C))
        self.pos_embed = nn.Parameter(torch.randn(1, 1 + self.grid[0] * self.grid[1], C) * 0.02)
        self.patch_embed = _PatchEmbed(C)
        self.blocks = nn.ModuleList([_Block(C, F_, eps) for _ in range(self.depth)])
        self.norm = nn.LayerNorm(C, eps=eps)

    @classmethod
    def from_timm(cls, model: nn.Module) -> "DinoViT":
        """Adopt the parameters (the same ``nn.Parameter`` objects) of a timm ``VisionTransformer`` such as
        ``DinoWrapper.model``."""
        C = model.cls_token.shape[-1]
        heads = model.blocks[0].attn.num_heads
        F_ = model.blocks[0].mlp.fc1.out_features
        grid = getattr(model.patch_embed, "grid_size", None)
        if grid is None:
            g = int(round((model.pos_embed.shape[1] - 1) ** 0.5))
            grid = (g, g)
        m = cls(C, len(model.blocks), heads, F_ / C, (grid[0] * PATCH, grid[1] * PATCH), model.norm.eps)
        theirs = dict(model.named_parameters())
        for name, _ in list(m.named_parameters()):
            if name not in theirs:
                raise ValueError(f"lara_amd.dino.from_timm: the model has no parameter {name}")
            *path, leaf = name.split(".")
            owner = m
            for p in path:
                owner = getattr(owner, p)
            setattr(owner, leaf, theirs[name])
        return m

    # -- the kernels' argument list --------------------------------------------------------------------------------------------
    def _params(self, h, w):
        ps = [self.cls_token, resample_pos_embed(self.pos_embed, (h, w), self.grid), self.patch_embed.proj.weight,
              self.patch_embed.proj.bias]
        for b in self.blocks:
            ps += [b.norm1.weight, b.norm1.bias, b.attn.qkv.weight, b.attn.qkv.bias, b.attn.proj.weight, b.attn.proj.bias,
                   b.norm2.weight, b.norm2.bias, b.mlp.fc1.weight, b.mlp.fc1.bias, b.mlp.fc2.weight, b.mlp.fc2.bias]
        return ps + [self.norm.weight, self.norm.bias]

    @staticmethod
    def check_size(H, W):
        if H <= 0 or W <= 0 or H % PATCH or W % PATCH:
            raise ValueError(f"lara_amd.dino: image size {H} x {W} must be a positive multiple of {PATCH} in both dimensions")
        if 1 + (H // PATCH) * (W // PATCH) > MAX_T:
            raise ValueError(f"lara_amd.dino: {H} x {W} gives more than {MAX_T} tokens")

    def _run(self, images, N, views, H, W, strides):
        self.check_size(H, W)
        require_device(images)
        if images.dtype != torch.float32:
            raise ValueError(f"lara_amd.dino: images must be fp32; got {images.dtype}")
        params = self._params(H // PATCH, W // PATCH)
        flat = [p.detach().float().contiguous() for p in params]
        run = _Run(_dims(N, views, H, W, self.C, self.num_heads, self.F, self.depth, self.eps, strides), images.detach(), flat,
                   images.device)
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            return _VitFn.apply(run, images.detach(), *params)
        return run.forward(training=False)

    def forward(self, images: torch.Tensor) -> torch.Tensor:
        """``DinoWrapper.forward``: images [N, 3, H, W] in [0, 1] (any strides) -> tokens [N, hw, C] fp32."""
        if images.dim() != 4 or images.shape[1] != 3:
            raise ValueError(f"lara_amd.dino: images must be [N, 3, H, W]; got {tuple(images.shape)}")
        N, _, H, W = images.shape
        s = images.stride()
        return self._run(images, N, 1, H, W, (s[0], 0, s[1], s[2], s[3]))

    def image_features(self, batch: dict, n_views: int) -> torch.Tensor:
        """network.py:439-445: reads ``batch['tar_rgb'][:, :n_views]`` ([B, V, H, W, 3]) in place and returns the image features
        [B * n_views, C, h, w], a channels-last view of the tokens (what ``FeatureVolume`` reads in place)."""
        rgb = batch["tar_rgb"]
        if rgb.dim() != 5 or rgb.shape[-1] != 3:
            raise ValueError(f"lara_amd.dino: tar_rgb must be [B, V, H, W, 3]; got {tuple(rgb.shape)}")
        B, V_all, H, W, _ = rgb.shape
        V = int(n_views)
        if not 1 <= V <= V_all:
            raise ValueError(f"lara_amd.dino: n_views {V} out of range for {V_all} views")
        s = rgb.stride()
        tok = self._run(rgb, B * V, V, H, W, (s[0], s[1], s[4], s[2], s[3]))
        return tok.view(B * V, H // PATCH, W // PATCH, self.C).permute(0, 3, 1, 2)
