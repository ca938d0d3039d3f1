"""Adapter between the reference's OWN gobjaverse dataset class and the device-side ray kernel (SURVEY.md
section 8f row 3, the loader half).

The dataset class stays reference code (``dataLoader/gobjverse.py:17-146``: HDF5 layout, view selection,
compositing, first-view alignment are its business and are not restated here).  What this module changes is only
where the two ray maps come from: the reference builds ``tar_rays`` / ``tar_rays_down`` (6 floats per pixel and
view, 50 MB per scene at 8 x 512^2) on the CPU workers (``gobjverse.py:90-93``, ``dataLoader/utils.py:21-34``) and
ships them through the DataLoader; here

* ``skip_cpu_rays(module)`` turns the two ``build_rays`` calls of the reference's loader module into no-ops, and
* ``collate_to_device(items, device)`` is the ``collate_fn`` that moves the collated cameras and images to the GPU
  and generates both ray maps there with the HIP kernel (``lara_amd.batch.build_rays``, csrc/rays.hip).

    import dataLoader.gobjverse as ref                       # the reference's module, unmodified
    lara_amd.dataset.skip_cpu_rays(ref)
    loader = DataLoader(ref.gobjverse(cfg), batch_size=4, num_workers=0, collate_fn=lambda b: collate_to_device(b, "cuda"))

Worker processes: a ``collate_fn`` runs INSIDE the DataLoader's workers, where HIP cannot be initialised after a fork (and a
lambda does not pickle under spawn) -- so the form above is for ``num_workers=0``.  With workers (the reference trains with 8,
train_lightning.py:35-39) keep the default CPU collate in the workers and finish the batch in the training process:

    lara_amd.dataset.skip_cpu_rays(ref)                      # before the workers start; patches this process AND, under fork,
                                                             # the workers (under spawn call it in `worker_init_fn` as well)
    loader = DataLoader(ref.gobjverse(cfg), batch_size=4, num_workers=8, collate_fn=lara_amd.dataset.collate_cpu)
    for batch in lara_amd.dataset.on_device(loader, "cuda"): ...

The image half.  The class also builds every item's images in float32 on the worker (``gobjverse.py:127-141``, ``:82-84``: the
division by 255, the composite over the view's background, the normal decode and its product with the first view's rotation), and
ships them 3.6 times as large as they are stored.  ``raw_views(ds)`` makes the class ship the arrays as stored -- ``tar_rgb`` uint8
[V,H,W,4], ``tar_nrm_u8`` uint8 [V,H,W,3], ``tar_msk`` an empty stub -- with the same random draws and every other field as before, and
``finish_on_device`` (so ``on_device`` and ``collate_to_device`` too) finishes such a batch with ONE kernel (``finish_images``,
csrc/batchfinish.hip, include/lara_batchfinish.h) into the tensors the class's own items collate to: ``tar_rgb`` fp32 [B,V,H,W,3] with
the class's bits, ``tar_msk`` uint8 [B,V,H,W], ``tar_nrm`` fp32 [B,H,V*W,3] (a 3-term fp32 sum in a fixed order, where numpy's matmul
picks its own).  Float items go through every function here exactly as before.

    lara_amd.dataset.skip_cpu_rays(ref)
    loader = DataLoader(lara_amd.dataset.raw_views(ref.gobjverse(cfg)), batch_size=4, num_workers=8, collate_fn=lara_amd.dataset.collate_cpu)
    for batch in lara_amd.dataset.on_device(loader, "cuda"): ...
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native

RAY_KEYS = ("tar_rays", "tar_rays_down")
_WHO = "lara_amd.dataset"


def skip_cpu_rays(loader_module):
    """Replace ``build_rays`` in the namespace of the reference's loader module (``dataLoader.gobjverse``) by a stub
    returning an empty array: its ``__getitem__`` then spends no CPU time on the rays and ships 0 bytes for them;
    ``collate_to_device`` fills both keys on the GPU.  Returns the original function (to restore it)."""
    original = loader_module.build_rays
    loader_module.build_rays = lambda c2ws, ixts, H, W, scale=1.0: np.zeros((0,), dtype=np.float32)
    return original


def collate_cpu(items):
    """The worker-side half: default collate WITHOUT the two ray maps (picklable: a module-level function).  The uint8 arrays of
    ``raw_views`` items are collated as they are."""
    return torch.utils.data.default_collate([{k: v for k, v in it.items() if k not in RAY_KEYS} for it in items])


def finish_on_device(batch, device="cuda"):
    """The training-process half: move a CPU-collated batch (``collate_cpu``) to `device` and build both ray maps there.  A batch
    of ``raw_views`` items (``tar_rgb`` uint8 with 4 channels) has its image half finished there too (``finish_images``): ``tar_rgb``
    and ``tar_msk`` are filled, ``tar_nrm`` replaces ``tar_nrm_u8``.  Any other batch is handled as it always was."""
    from .batch import build_rays
    dev = torch.device(device)
    batch = {k: (v.to(dev, non_blocking=True) if torch.is_tensor(v) else v) for k, v in batch.items()}
    stored = batch.get("tar_rgb")
    if torch.is_tensor(stored) and stored.dtype == torch.uint8 and stored.shape[-1] == 4:      # a batch of `raw_views` items
        normals = batch.pop("tar_nrm_u8", None)
        rot = batch["transform_mats"][:, 0, :3, :3].contiguous() if normals is not None else None
        batch["tar_rgb"], batch["tar_msk"], nrm = finish_images(batch["tar_rgb"], batch["bg_color"], normals, rot)
        if nrm is not None:
            batch["tar_nrm"] = nrm
    B, V = batch["tar_c2w"].shape[:2]
    H, W = int(batch["meta"]["tar_h"][0]), int(batch["meta"]["tar_w"][0])
    c2w, ixt = batch["tar_c2w"].reshape(B * V, 4, 4).float(), batch["tar_ixt"].reshape(B * V, 3, 3).float()
    batch["tar_rays"] = build_rays(c2w, ixt, H, W, 1.0).view(B, V, H, W, 6)
    down = build_rays(c2w, ixt, H, W, 1.0 / 16)
    batch["tar_rays_down"] = down.view(B, V, *down.shape[1:])
    return batch


def on_device(loader, device="cuda"):
    """Iterate a DataLoader built with ``collate_fn=collate_cpu`` (any ``num_workers``), yielding device batches."""
    for batch in loader:
        yield finish_on_device(batch, device)


def collate_to_device(items, device="cuda"):
    """Default-collate a list of the reference dataset's items onto `device`; ``tar_rays`` [B,V,H,W,6] and
    ``tar_rays_down`` [B,V,H/16,W/16,6] are (re)built there from the collated ``tar_c2w`` / ``tar_ixt``, whatever
    the items carried under those keys (CPU rays, or the empty stubs of `skip_cpu_rays`).  ``num_workers=0`` only (see the
    module docstring): it touches the GPU."""
    return finish_on_device(collate_cpu(items), device)


# ---------------------------------------------------------------------------------------------------------- the image half, worker side

class _CfgView:
    """The caller's cfg with ``load_normal`` read as False: every other attribute is forwarded, the cfg object itself is not touched.
    The reference's ``__getitem__`` then skips its float32 normal product (``gobjverse.py:82-84``)."""
    load_normal = False

    def __init__(self, cfg):
        self._cfg = cfg

    def __getattr__(self, name):                 # (only for what the instance and the class do not have)
        if name.startswith("__") or name == "_cfg":      # pickle and copy probe a bare instance: no forwarding before _cfg exists
            raise AttributeError(name)
        return getattr(self._cfg, name)


def _read_stored_image(scene, view_idx, bg_color, scene_name):
    """``read_image`` of a taken-over instance: the stored RGBA as it is, no normal, an empty mask (``finish_images`` fills it)."""
    return np.array(scene[f"image_{view_idx}"]), None, np.zeros((0,), dtype=np.uint8)


class RawViews(torch.utils.data.Dataset):
    """What ``raw_views`` returns: the taken-over instance, and the stored normals of each item's own views read by key."""

    def __init__(self, ds):
        cfg = ds.cfg._cfg if isinstance(ds.cfg, _CfgView) else ds.cfg
        self.load_normal = bool(cfg.load_normal)
        ds.cfg = _CfgView(cfg)
        ds.read_image = _read_stored_image       # (an instance attribute: the class and its other instances keep their method)
        self.ds = ds

    def __len__(self):
        return len(self.ds)

    def __getitem__(self, index):
        item = self.ds[index]
        if self.load_normal:
            scene = self.ds.metas[item["meta"]["scene"]]
            item["tar_nrm_u8"] = np.stack([np.array(scene[f"normal_{v}"]) for v in item["meta"]["tar_view"]])
        return item


def raw_views(ds):
    """Take over an instance of the reference's ``gobjverse`` class so that its items carry the images as stored: ``tar_rgb`` uint8
    [V,H,W,4], ``tar_msk`` an empty stub, and -- when ``ds.cfg.load_normal`` is set -- ``tar_nrm_u8`` uint8 [V,H,W,3] in place of
    ``tar_nrm``.  Views, ``bg_color``, cameras, ``transform_mats`` (it carries the normals' rotation), ``near_far`` and ``meta`` are
    the class's own, with its own random draws.  The instance gets a ``read_image`` of its own and a view of its cfg; the cfg object,
    the class and the scene store are not touched.  Returns a picklable ``Dataset``; ``skip_cpu_rays`` composes with it."""
    return RawViews(ds)


# ---------------------------------------------------------------------------------------------------------- the image half, device side

def _refuse(name, t, dtype, shape, device=None):
    """ValueError unless ``t`` is a contiguous tensor of ``dtype`` and ``shape`` (None: any extent) on ``device``."""
    want = f"a contiguous {str(dtype).replace('torch.', '')} [{', '.join('*' if n is None else str(n) for n in shape)}] tensor"
    if not torch.is_tensor(t):
        raise ValueError(f"{_WHO}: {name} must be {want}, got {type(t).__name__}")
    if t.dtype != dtype or t.dim() != len(shape) or any(n is not None and int(m) != n for m, n in zip(t.shape, shape)):
        raise ValueError(f"{_WHO}: {name} must be {want}, got {t.dtype} {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{_WHO}: {name} must be contiguous (strides {tuple(t.stride())} of shape {tuple(t.shape)})")
    if device is not None and t.device != device:
        raise ValueError(f"{_WHO}: {name} lies on {t.device}, rgba on {device}: all arguments share one device")


def _finish_into(rgba, bg_color, normals_u8, rot, out_rgb, out_msk, out_nrm):
    """One launch (one host loop for host tensors) into outputs the caller has allocated and checked."""
    B, V, H, W = (int(n) for n in rgba.shape[:4])
    if B * V * H * W == 0:                       # (an empty tensor has no address to hand over; the entry points launch nothing either)
        return
    if B * V * H * W >= 2 ** 31:
        raise ValueError(f"{_WHO}: rgba holds {B * V * H * W} pixels; one call takes fewer than 2^31")
    _native.call_on("lara_batch_finish", rgba.device, rgba, bg_color, normals_u8, rot, B, V, H, W, out_rgb, out_msk, out_nrm)


@torch.no_grad()
def finish_images(rgba, bg_color, normals_u8=None, rot=None):
    """The image half of a batch from the stored arrays (include/lara_batchfinish.h has the arithmetic, operation by operation):
    ``rgba`` uint8 [B,V,H,W,4] and ``bg_color`` fp32 [B,V,3] -> ``tar_rgb`` fp32 [B,V,H,W,3], the colour over each view's own
    background, and ``tar_msk`` uint8 [B,V,H,W], alpha > 0; with ``normals_u8`` uint8 [B,V,H,W,3] and ``rot`` fp32 [B,3,3]
    (``transform_mats[:, 0, :3, :3]``) also ``tar_nrm`` fp32 [B,H,V*W,3], the decoded normals times R^T with the views side by side;
    else None in its place.  Device tensors: one kernel on the current stream, no host read.  Host tensors: the same per-pixel
    function compiled for the CPU (``lara_batch_finish_host``), the reference the kernel is held to, not a fast path.  ValueError,
    naming the argument: a wrong dtype or shape, a non-contiguous input (a contiguous view at a storage offset is fine), normals
    without ``rot`` or ``rot`` without normals, arguments on different devices.  An empty batch launches nothing."""
    _refuse("rgba", rgba, torch.uint8, (None, None, None, None, 4))
    B, V, H, W = (int(n) for n in rgba.shape[:4])
    dev = rgba.device
    _refuse("bg_color", bg_color, torch.float32, (B, V, 3), dev)
    if (normals_u8 is None) != (rot is None):
        missing = "rot" if rot is None else "normals_u8"
        raise ValueError(f"{_WHO}: {missing} is missing: normals_u8 and rot (transform_mats[:, 0, :3, :3]) go together")
    if normals_u8 is not None:
        _refuse("normals_u8", normals_u8, torch.uint8, (B, V, H, W, 3), dev)
        _refuse("rot", rot, torch.float32, (B, 3, 3), dev)
    out_rgb = torch.empty(B, V, H, W, 3, dtype=torch.float32, device=dev)
    out_msk = torch.empty(B, V, H, W, dtype=torch.uint8, device=dev)
    out_nrm = torch.empty(B, H, V * W, 3, dtype=torch.float32, device=dev) if normals_u8 is not None else None
    _finish_into(rgba, bg_color, normals_u8, rot, out_rgb, out_msk, out_nrm)
    return out_rgb, out_msk, out_nrm
