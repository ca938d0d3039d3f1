"""LaRa's image-feature volume on the HIP kernels of ``liblara2dgs.so`` (csrc/featvol.hip, include/lara_featvol.h).

``FeatureVolume`` is ``Network.build_feat_vol`` plus the view-embedding concatenation (lightning/network.py:352-379 and
:448-452): Plucker ray features of ``tar_rays_down`` -> ``dir_norm`` (ModLN, under bf16 autocast as the reference trains)
-> bilinear samples of the modulated feature map at the projections of the R^3 ``volume_grid`` -> ``[B, V, C + E, R, R, R]``.
It owns the reference's parameters under the reference's names (``dir_norm.norm.*``, ``dir_norm.mlp.1.*``, ``view_embed``,
``volume_grid``), so a reference checkpoint loads into it, or it adopts the reference's own ``dir_norm`` / ``view_embed``.

The backward is bit-reproducible (no float atomics): the sampling backward is a gather over per-view texel lists.
``encoder_train.VolTransformer.forward_from_image_features`` runs the same kernels straight into the encoder's bf16 operand.

There is no CPU path and no torch fallback: tensors must live on the GPU and the library must load.
"""
from __future__ import annotations

import torch
from torch import nn

from ._native import FeatvolDims as _Dims, alloc_bytes, call, query, require_device
from ._native import load_library as _lib  # noqa: F401  (the shared loader; this name was imported from here)

VOLUME, TOKENS = 0, 1          # LARA_FEATVOL_VOLUME / LARA_FEATVOL_TOKENS
MAX_C, MAX_HW = 1024, 8192


class _ModLN(nn.Module):
    """Parameter container shaped like the reference's ``ModLN`` (network.py:190-213)."""

    def __init__(self, inner_dim: int, mod_dim: int, eps: float):
        super().__init__()
        self.norm = nn.LayerNorm(inner_dim, eps=eps)
        self.mlp = nn.Sequential(nn.SiLU(), nn.Linear(mod_dim, inner_dim * 2))


def build_dense_grid(reso: int, scene_size: float = 0.5) -> torch.Tensor:
    """network.py:345-349."""
    a = torch.arange(reso)
    grid = torch.stack(torch.meshgrid(a, a, a, indexing="ij"), dim=-1)
    return ((grid + 0.5) / reso * 2 - 1).reshape(reso, reso, reso, 3) * scene_size


class _Prep:
    """Everything one call of the kernels reads, checked and laid out."""

    def __init__(self, fv, batch, img_feats, n_views_sel):
        require_device(img_feats)
        if img_feats.dim() != 4 or img_feats.dtype != torch.float32:
            raise ValueError(f"img_feats must be fp32 [B*V, C, h, w]; got {img_feats.dtype} {tuple(img_feats.shape)}")
        V = int(n_views_sel)
        rays = batch["tar_rays_down"]
        B = rays.shape[0]
        BV, C, h, w = img_feats.shape
        if not 1 <= V <= min(8, rays.shape[1]) or BV != B * V:
            raise ValueError(f"img_feats holds {BV} maps; expected B * n_views_sel = {B} * {V} (at most 8 and the batch's views)")
        if tuple(rays.shape[2:]) != (h, w, 6):
            raise ValueError(f"tar_rays_down {tuple(rays.shape)} does not match the feature map {h} x {w}")
        if C != fv.C or C % 64 or C > MAX_C or h * w > MAX_HW:
            raise ValueError(f"feature channels {C} (module: {fv.C}; a multiple of 64 up to {MAX_C}), map {h} x {w} (at most {MAX_HW} texels)")
        if V > fv.view_embed.shape[1] and fv.E > 0:
            raise ValueError(f"view_embed has {fv.view_embed.shape[1]} rows, n_views_sel = {V}")
        dev = img_feats.device
        f32 = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
        self.x = img_feats.detach()
        self.rays = f32(rays[:, :V])
        self.w2c = f32(batch["tar_w2c"][:, :V])
        self.ixt = f32(batch["tar_ixt"][:, :V])
        self.grid = f32(fv.volume_grid.reshape(-1, 3))
        H, W = batch["tar_rgb"].shape[2:4]
        d = _Dims()
        d.B, d.V, d.C, d.E, d.h, d.w, d.R, d.img_w, d.img_h = B, V, C, fv.E, h, w, fv.R, int(W), int(H)
        d.eps = float(fv.dir_norm.norm.eps)
        for i, s in enumerate(img_feats.stride()):
            d.x_stride[i] = s
        self.d, self.dev, self.B, self.V, self.C, self.E, self.S = d, dev, B, V, C, fv.E, fv.R ** 3

    def params(self, ln_w, ln_b, mlp_w, mlp_b, embed):
        f = lambda t: None if t is None else t.detach().float().contiguous()
        self.p = (f(ln_w), f(ln_b), f(mlp_w), f(mlp_b), f(embed))

    def _ws(self):
        return alloc_bytes(query("lara_featvol_workspace_bytes", self.d), self.dev)

    def _inputs(self):
        return (self.x, self.rays, self.w2c, self.ixt, self.grid) + self.p[:4]

    def forward(self, layout):
        CE, R = self.C + self.E, self.d.R
        out = (torch.empty(self.B, self.V, CE, R, R, R, dtype=torch.float32, device=self.dev) if layout == VOLUME else
               torch.empty(self.B * self.S, self.V, CE, dtype=torch.bfloat16, device=self.dev))
        call("lara_featvol_forward", self.dev, self.d, *self._inputs(), self.p[4], layout, out, self._ws())
        return out

    def backward(self, grad, layout, want_embed=True):
        """grad fp32 in `layout` -> (dx at img_feats' strides, d ln_w, d ln_b, d mlp_w, d mlp_b, d embed [V, E] or None)"""
        f32 = dict(dtype=torch.float32, device=self.dev)
        grad = grad.float().contiguous()
        dx = torch.empty_strided(self.x.shape, self.x.stride(), **f32)
        C = self.C
        d_lnw, d_lnb = torch.empty(C, **f32), torch.empty(C, **f32)
        d_w, d_b = torch.empty(2 * C, 32, **f32), torch.empty(2 * C, **f32)
        d_e = torch.empty(self.V, self.E, **f32) if (want_embed and self.E > 0) else None
        call("lara_featvol_backward", self.dev, self.d, *self._inputs(), grad, layout, dx, d_lnw, d_lnb, d_w, d_b, d_e, self._ws())
        return dx, d_lnw, d_lnb, d_w, d_b, d_e


class _FeatVolFn(torch.autograd.Function):
    """(img_feats, gamma, beta, W, b, view_embed rows [V, E] or None) -> feat_vol [B, V, C + E, R, R, R]."""

    @staticmethod
    def forward(ctx, img_feats, ln_w, ln_b, mlp_w, mlp_b, embed, prep):
        prep.params(ln_w, ln_b, mlp_w, mlp_b, embed)
        ctx.prep = prep
        return prep.forward(VOLUME)

    @staticmethod
    def backward(ctx, g):
        dx, d_lnw, d_lnb, d_w, d_b, d_e = ctx.prep.backward(g, VOLUME, ctx.needs_input_grad[5])
        return dx, d_lnw, d_lnb, d_w, d_b, d_e, None


class FeatureVolume(nn.Module):
    """network.py:352-379 + :448-452 on the HIP kernels.  ``C``: image-feature channels (DINO's 768); ``E``:
    ``view_embed_dim`` (0: no view embedding); ``R``: ``vol_feat_reso``.  ``dir_norm`` / ``view_embed``: adopt the reference
    ``Network``'s own objects instead of creating new ones."""

    def __init__(self, C: int = 768, E: int = 32, R: int = 16, eps: float = 1e-6, scene_size: float = 0.5,
                 dir_norm: nn.Module = None, view_embed: nn.Parameter = None):
        super().__init__()
        self.C, self.E, self.R = C, E, R
        self.dir_norm = dir_norm if dir_norm is not None else _ModLN(C, 16 * 2, eps)
        if E > 0:
            self.view_embed = view_embed if view_embed is not None else nn.Parameter(torch.randn(1, 4, E, 1, 1, 1) * (1. / E) ** 0.5)
            if tuple(self.view_embed.shape[2:]) != (E, 1, 1, 1):
                raise ValueError(f"view_embed must be [1, n, {E}, 1, 1, 1]; got {tuple(self.view_embed.shape)}")
        else:
            self.view_embed = None
        lin = self.dir_norm.mlp[1]
        if tuple(lin.weight.shape) != (2 * C, 32) or lin.bias is None or self.dir_norm.norm.weight.shape[0] != C:
            raise ValueError("dir_norm must be ModLN(C, 32): norm = LayerNorm(C), mlp = Sequential(SiLU, Linear(32, 2C))")
        self.register_buffer("volume_grid", build_dense_grid(R, scene_size))

    def _args(self, V):
        n, lin = self.dir_norm.norm, self.dir_norm.mlp[1]
        embed = self.view_embed[0, :V, :, 0, 0, 0] if self.E > 0 else None
        return n.weight, n.bias, lin.weight, lin.bias, embed

    def prepare(self, batch, img_feats, n_views_sel=None):
        V = n_views_sel if n_views_sel is not None else img_feats.shape[0] // batch["tar_rays_down"].shape[0]
        return _Prep(self, batch, img_feats, V)

    def forward(self, batch, img_feats, n_views_sel=None):
        prep = self.prepare(batch, img_feats, n_views_sel)
        return _FeatVolFn.apply(img_feats, *self._args(prep.V), prep)
