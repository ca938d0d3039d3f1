"""Generates tests/golden/eval_ref.npz by importing the REFERENCE's own modules (read from /root/reference; run in the build
container only:  python tests/golden/make_eval_fixture.py).  Arrays only.

  cameras  `tools.gen_video_path.generate_gobjverse_frames` / `generate_instant3d_frames` (what `uni_video_path` and
           `uni_mesh_path` dispatch to, :107-129), n = 8, elevations 0 and -30, with and without `sample['transform_mats']`:
           the `world_view_transform`, `full_proj_transform`, `camera_center` and `get_rays()` of the reference's own `MiniCam`s;
           and the matrices of one `uni_mesh_path` call per family.  `tools.gen_video_path` imports here only with `h5py` / `cv2`
           stand-ins (as tests/golden/make_loader_fixture.py does), a bare `dataLoader` package and a stand-in for
           `tools.camera_utils` (used by the 'unposed' path only).
  depth    the outputs of the reference's own `tools.depth.abs_error` / `acc_threshold`, called as evaluation.py:98-110 calls them,
           on seeded float32 maps, masks and thresholds (some differences sit exactly on a threshold).
  psnr     the reference has no callable for it (it is inline in `main`): the expression of evaluation.py:84-85 is evaluated HERE,
           verbatim, on seeded images.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for name in ("h5py", "cv2"):
    sys.modules.setdefault(name, types.ModuleType(name))
pkg = types.ModuleType("dataLoader")
pkg.__path__ = ["/root/reference/dataLoader"]
sys.modules["dataLoader"] = pkg
sys.path.insert(0, "/root/reference")
# tools/camera_utils.py (the nerfstudio pose interpolation: only the 'unposed' path calls it) needs `jaxtyping`, absent here
cu = types.ModuleType("tools.camera_utils")
cu.get_interpolated_poses_many = None
sys.modules["tools.camera_utils"] = cu
from tools import gen_video_path as gvp  # noqa: E402
from tools.depth import abs_error, acc_threshold  # noqa: E402

out = {}
N, SIZE = 8, (12, 8)                      # (width, height)
g = torch.Generator().manual_seed(11)

# a rigid transform as the loader's `transform_mats` [B, 1, 4, 4]
q = torch.linalg.qr(torch.randn(3, 3, generator=g))[0]
if torch.det(q) < 0:
    q[:, 0] = -q[:, 0]
tm = torch.eye(4)
tm[:3, :3], tm[:3, 3] = q, torch.randn(3, generator=g) * 0.1
sample = {"transform_mats": tm[None, None].clone()}
fov = [torch.tensor([0.6]), torch.tensor([0.65])]
out["cam/transform_mats"] = sample["transform_mats"].numpy()
out["cam/fov"] = np.array([0.6, 0.65], np.float32)
out["cam/img_size"] = np.array(SIZE)


def store(tag, cams, rays=True):
    out[f"{tag}/world_view_transform"] = np.stack([c.world_view_transform.numpy() for c in cams])
    out[f"{tag}/full_proj_transform"] = np.stack([c.full_proj_transform.numpy() for c in cams])
    out[f"{tag}/camera_center"] = np.stack([c.camera_center.numpy() for c in cams])
    out[f"{tag}/scalars"] = np.array([[c.FoVx, c.FoVy, c.znear, c.zfar, c.image_width, c.image_height] for c in cams], np.float64)
    if rays:
        out[f"{tag}/rays"] = np.stack([c.get_rays().numpy()[0] for c in cams])


for family, name, fn in (("gobj", "gobjeverse", gvp.generate_gobjverse_frames), ("i3d", "instant3d", gvp.generate_instant3d_frames)):
    cfg = types.SimpleNamespace(dataset_name=name, img_size=SIZE)
    for with_sample in (0, 1):
        for elev in (0, -30):
            cams = fn(N, cfg, sample if with_sample else None, elev, fov=fov if with_sample else None)
            store(f"cam/{family}/s{with_sample}/e{elev}", cams)
    store(f"mesh/{family}", gvp.uni_mesh_path(N, cfg, sample, fov=fov), rays=False)
    # uni_video_path is the elevation-0 case above; checked here so that the fixture says so
    a = gvp.uni_video_path(N, cfg, sample, fov=fov)
    assert all(torch.equal(x.world_view_transform, torch.from_numpy(y)) for x, y in zip(a, out[f"cam/{family}/s1/e0/world_view_transform"]))

# ---- depth: evaluation.py:98-110 on a `sample` / `output` pair of seeded maps
B, V, H, W = 3, 3, 10, 14
thresholds = [0.01, 0.05, 0.1]
tar_dep = (torch.rand(B, V, H, W, generator=g) * 2 + 0.5).float()
depth_gt_strip = tar_dep.permute(0, 2, 1, 3).reshape(B, H, V * W)
depth_fine = (depth_gt_strip + torch.randn(B, H, V * W, generator=g) * 0.05).float()
# differences placed exactly on a threshold: (pred, gt) = (2 t, t), (t, 2 t), (t, 0), (0, t) with t = float32(threshold) --
# doubling and subtracting a number from its double are exact in float32
for i, t in enumerate(thresholds):
    t32 = float(np.float32(t))
    pairs = torch.tensor([[2 * t32, t32], [t32, 2 * t32], [t32, 0.0], [0.0, t32]], dtype=torch.float32)
    tar_dep[0, 0, i, :4] = pairs[:, 1]                    # view 0, row i, columns 0..3 = the strip's row i, columns 0..3
    depth_gt_strip = tar_dep.permute(0, 2, 1, 3).reshape(B, H, V * W)
    depth_fine[0, i, :4] = pairs[:, 0]
tar_msk = (torch.rand(B, V, H, W, generator=g) < 0.3).float()
tar_msk[0, :, :3] = 1.0                                   # the rows holding the on-threshold differences are inside
tar_msk[1] = 1.0                                          # a full mask
out["depth/tar_dep"], out["depth/tar_msk"] = tar_dep.numpy(), tar_msk.numpy()
out["depth/depth_fine"] = depth_fine[..., None].numpy()
out["depth/thresholds"] = np.array(thresholds, np.float64)
strip = lambda t: t.permute(0, 2, 1, 3).reshape(t.shape[0], H, V * W)      # [B, V, H, W] -> the side-by-side layout of :99, :101
for b in range(B):          # one scene per call, as the reference's batch of one
    mask = strip(tar_msk[b:b + 1]).bool().numpy()
    gt = strip(tar_dep[b:b + 1]).numpy()
    pred = depth_fine[b:b + 1, ..., None].squeeze(-1).numpy()
    accs = [acc_threshold(pred, gt, mask, threshold=t) for t in thresholds]
    out[f"depth/{b}/depth_acc"] = np.array([abs_error(pred, gt, mask).mean().item()] + [a.mean() for a in accs], np.float64)
    out[f"depth/{b}/counts"] = np.array([int(mask.sum())] + [int(a.sum()) for a in accs], np.int64)   # masked, below each threshold

# ---- psnr: evaluation.py:84-85, verbatim (no callable in the reference)
device = "cpu"
images = torch.rand(1, 3, 16, 40, generator=g)
img_gt = (images + torch.randn(1, 3, 16, 40, generator=g) * 0.05).clamp(0, 1)
color_loss_all = (images - img_gt) ** 2
psnr = -10. * torch.log(color_loss_all.mean()) / torch.log(torch.tensor([10.]).to(device))
out["psnr/images"], out["psnr/img_gt"], out["psnr/psnr"] = images.numpy(), img_gt.numpy(), np.array(psnr.item())

np.savez_compressed(os.path.join(ROOT, "tests", "golden", "eval_ref.npz"), **out)
print("wrote", len(out), "arrays")
