"""Generates tests/golden/shim_settings_ref.npz: the rasteriser settings record that the REFERENCE's own, unmodified
`lightning.renderer_2dgs.Renderer.set_rasterizer` (renderer_2dgs.py:119-139) builds from its own `MiniCam`
(lightning/utils.py:5-48) when `diff_surfel_rasterization` resolves to this repository's shim: the field names in order,
each field's Python type and value, and the names the reference module takes from the shim.  Run where a LaRa checkout
is available:
    python tests/golden/make_shim_settings_fixture.py <path of the LaRa checkout>
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.path.abspath(sys.argv[1])
sys.path.insert(0, ROOT)     # the shim `diff_surfel_rasterization`
sys.path.insert(0, REF)
import diff_surfel_rasterization as shim  # noqa: E402
import lightning.renderer_2dgs as ref_r  # noqa: E402  (unmodified; `from diff_surfel_rasterization import ...` at :7-10)
from lightning.utils import MiniCam  # noqa: E402

# the camera of tests/test_cameras.py: pose 3 of cameras_ref.npz, a non-square image, distinct fields of view
c2w = torch.from_numpy(np.load(os.path.join(ROOT, "tests", "golden", "cameras_ref.npz"))["c2w"][3])
W, H, fovx, fovy, zn, zf = 512, 384, 0.75, 0.6, 1.106, 2.706
bg = torch.tensor([0.5, 0.5, 0.5])
cam = MiniCam(c2w.clone(), W, H, torch.tensor(fovy), torch.tensor(fovx), torch.tensor(zn), torch.tensor(zf), "cpu")
r = ref_r.Renderer(sh_degree=1, white_background=True)
r.set_bg_color(bg)                                      # network.py:489-490
settings = r.set_rasterizer(cam, device="cpu").raster_settings

store = {"pose_index": np.array(3), "camera": np.array([W, H, fovx, fovy, zn, zf], np.float64), "bg": bg.numpy(),
         "shim_names": np.array(sorted(n for n in vars(ref_r) if not n.startswith("__") and getattr(shim, n, None) is getattr(ref_r, n))),
         "field_names": np.array(settings._fields), "field_types": np.array([type(v).__name__ for v in settings])}
for name, v in zip(settings._fields, settings):
    store[f"value/{name}"] = v.numpy() if isinstance(v, torch.Tensor) else np.array(v)
np.savez_compressed(os.path.join(ROOT, "tests", "golden", "shim_settings_ref.npz"), **store)
print("wrote", {k: (v.dtype, v.shape) for k, v in store.items()})
