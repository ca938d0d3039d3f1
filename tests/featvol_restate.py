"""Plain-torch restatement of network.py:352-379 + :448-452 (the image-feature volume), shared by tests/test_featvol.py and
tests/test_featvol_gpu.py.  `bf16=True` spells out what bf16 autocast does to it (train_lightning.py:76): the Linear of ModLN on
bf16 operands with a bf16 result; `1 + scale` of that bf16 tensor stays bf16; the two matmuls of `projection` on bf16 operands,
so the sample positions are bf16 tensors until grid_sample; LayerNorm and grid_sample in fp32."""
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))


def rsh3(v):
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    x2, y2, z2, xy, xz, yz = x * x, y * y, z * z, x * y, x * z, y * z
    return torch.stack([torch.full_like(x, 0.282094791773878), -0.48860251190292 * y, 0.48860251190292 * z,
                        -0.48860251190292 * x, 1.09254843059208 * xy, -1.09254843059208 * yz, 0.94617469575756 * z2 - 0.31539156525252,
                        -1.09254843059208 * xz, 0.54627421529604 * x2 - 0.54627421529604 * y2, -0.590043589926644 * y * (3.0 * x2 - y2),
                        2.89061144264055 * xy * z, 0.304697199642977 * y * (1.5 - 7.5 * z2),
                        1.24392110863372 * z * (1.5 * z2 - 0.5) - 0.497568443453487 * z, 0.304697199642977 * x * (1.5 - 7.5 * z2),
                        1.44530572132028 * z * (x2 - y2), -0.590043589926644 * x * (x2 - 3.0 * y2)], -1)


def dense_grid(R, scene_size=0.5, device="cpu"):
    a = torch.arange(R, device=device)
    g = torch.stack(torch.meshgrid(a, a, a, indexing="ij"), dim=-1)
    return ((g + 0.5) / R * 2 - 1) * scene_size


def restated(batch, x, ln_w, ln_b, mlp_w, mlp_b, view_embed, R, img_hw, V, bf16=False, eps=1e-6):
    """-> [B, V, C + E, R, R, R] fp32; x [B V, C, h, w] fp32; view_embed [1, n, E, 1, 1, 1] or None."""
    BV, C, h, w = x.shape
    B = BV // V
    rays = batch["tar_rays_down"][:, :V].reshape(BV, h, w, 6).float()
    d = F.normalize(rays[..., 3:6], p=2.0, dim=-1)
    f = torch.cat([rsh3(d), rsh3(torch.cross(rays[..., :3], d, dim=-1))], -1)
    a = F.silu(f)
    mod = F.linear(a.bfloat16(), mlp_w.bfloat16(), mlp_b.bfloat16()) if bf16 else F.linear(a, mlp_w, mlp_b)
    shift, scale = mod.chunk(2, dim=-1)
    n = F.layer_norm(x.permute(0, 2, 3, 1), (C,), ln_w, ln_b, eps)
    y = n * (1 + scale) + shift
    H, W = img_hw
    w2c = batch["tar_w2c"][:, :V].reshape(-1, 4, 4).float()
    ixt = batch["tar_ixt"][:, :V].reshape(-1, 3, 3).float()
    grid, rot, t = dense_grid(R, device=x.device).reshape(1, -1, 3), w2c[:, :3, :3], w2c[:, :3, 3][:, None]
    if bf16:      # the matmuls of `projection` and everything after them up to grid_sample run on bf16 tensors
        grid, rot, ixt = grid.bfloat16(), rot.bfloat16(), ixt.bfloat16()
    pc = grid @ rot.permute(0, 2, 1) + t
    q = (pc.bfloat16() if bf16 else pc) @ ixt.permute(0, 2, 1)
    g = (q[..., :2] / q[..., -1:] + 0.5) / torch.tensor([W, H], device=x.device) * 2 - 1.0
    s = F.grid_sample(y.permute(0, 3, 1, 2).float(), g.float().unsqueeze(1), align_corners=False).view(B, V, C, R, R, R)
    if view_embed is None:
        return s
    return torch.cat([s, view_embed[:, :V].expand(B, -1, -1, R, R, R)], dim=2)


def load_fixture(device="cpu"):
    f = np.load(os.path.join(HERE, "golden", "featvol_ref.npz"))
    t = {k: torch.from_numpy(f[k]).to(device) for k in f.files if not k.endswith("_dtypes") and k != "img_hw"}
    B, V, h, w = t["tar_rays_down"].shape[:4]
    C = t["ln_w"].shape[0]
    # the reference's image features: a channels-last view of DINO's [B V, h w, C] tokens (network.py:443-445)
    t["img_feats"] = torch.einsum("blc->bcl", t["tokens"]).reshape(B * V, C, h, w)
    batch = {k: t[k] for k in ("tar_rays_down", "tar_w2c", "tar_ixt")}
    H, W = (int(v) for v in f["img_hw"])
    batch["tar_rgb"] = torch.zeros(B, V, H, W, 3, device=device)
    return f, t, batch
