"""LaRa's evaluation loop (evaluation.py:54-176) behind ``Network.forward``, on the device (include/lara_eval.h,
csrc/evalscores.hip); opt-in like every module here.

Per scene the reference (a) permutes render and targets, computes PSNR and ``pytorch_msssim.ssim`` on the side-by-side strip,
optionally cropped to the novel views (:75-95); (b) copies three full [B, H, N*W] maps to the host and reduces them with numpy
(:97-111, tools/depth.py); (c) renders ``video_frames`` turntable views one ``render_img`` at a time, each followed by host
copies of two float maps and ``np.round(... * 255)`` (:118-141).  Here:

  * ``scene_scores``     one scores pass over the tensors where they lie (the crop is a pointer offset) and ONE device-to-host copy
                         of a [B, 16] array;
  * ``video_cameras`` / ``mesh_cameras``  ``uni_video_path`` / ``uni_mesh_path`` (tools/gen_video_path.py) as one batched pass;
  * ``render_turntable`` device-side rays, ``Renderer.render_views(..., concat=True)`` in chunks, one frame-quantising kernel
                         per chunk: two device uint8 tensors [N, H, W, 3] -- what a video writer takes;
  * ``Evaluator``        accumulates scenes and writes the JSON of evaluation.py:164-176.

Limits.  SSIM: `pytorch_msssim` is absent from the reference tree and from the build image (version not pinned): the kernel
follows the published algorithm (11-tap sigma-1.5 Gaussian, 'valid', K = (0.01, 0.03)) and is held to a float64 restatement
(tests/eval_restate.py) -- PARITY with the package itself is UNPINNED, as for the MS-SSIM term (lara_amd/loss.py).  LPIPS
(evaluation.py:48-49, :89-90) runs on the device through `lara_amd.lpips` when ``Evaluator`` is given ``lara_amd.lpips.LPIPS``
instances (the pretrained weights are the caller's to load; parity with the `lpips` package is unpinned too); it also takes any
other callables, and writes null without either.  Writing the jpg strip and the mp4 (cv2 / imageio) is left to the caller.  No
CPU path: tensors must live on the GPU.
"""
from __future__ import annotations

import json
import math
import os

import torch

from . import cameras as _cameras
from ._native import ImageView as _ImgView, call, host_array, query, require_device
from ._native import load_library as _lib  # noqa: F401  (the shared loader; this name was imported from here)
from .loss import _window_host

ROW = 16                   # include/lara_eval.h: LARA_EVAL_ROW
MAX_THRESHOLDS = 8         # LARA_EVAL_MAX_THRESHOLDS


# ---------------------------------------------------------------------------------------------------------- scores

def scores_device(image, tar_rgb, skip_views=0, depth_pred=None, tar_dep=None, tar_msk=None, thresholds=()):
    """The device array [B, 16] (float64) of ``lara_eval_scores`` (layout: include/lara_eval.h) for the render ``image``
    [B, H, V*W, 3] against ``tar_rgb`` [B, V, H, W, 3] without their first ``skip_views`` views (evaluation.py:75-78: a pointer
    offset, nothing is copied), and the depth scores over all views of ``depth_pred`` [B, H, V*W(, 1)], ``tar_dep`` and
    ``tar_msk`` [B, V, H, W] (all three or none).  ``image`` None: no image scores.  No host synchronisation."""
    thresholds = [float(t) for t in thresholds]
    if len(thresholds) > MAX_THRESHOLDS:
        raise ValueError(f"lara_amd.evaluate: at most {MAX_THRESHOLDS} depth thresholds per call, got {len(thresholds)}")
    have_depth = depth_pred is not None
    if have_depth and (tar_dep is None or tar_msk is None):
        raise ValueError("lara_amd.evaluate: depth_pred, tar_dep and tar_msk come together")
    B = H = Wc = 0
    if image is not None:
        B, V, H, W = tar_rgb.shape[:4]
        if tuple(tar_rgb.shape) != (B, V, H, W, 3) or tuple(image.shape) != (B, H, V * W, 3):
            raise ValueError("lara_amd.evaluate: expected tar_rgb [B,V,H,W,3] and image [B,H,V*W,3]")
        if not 0 <= skip_views < V:
            raise ValueError("lara_amd.evaluate: the crop leaves no view to score")
        Wc = (V - skip_views) * W
        if min(H, Wc) < 11:
            raise ValueError(f"lara_amd.evaluate: SSIM needs sides of at least 11 (one window), got {H} x {Wc}")
    Vd = Hd = Wd = 0
    if have_depth:
        Bd, Vd, Hd, Wd = tar_dep.shape
        if tuple(tar_msk.shape) != (Bd, Vd, Hd, Wd) or depth_pred.numel() != Bd * Vd * Hd * Wd or depth_pred.shape[:2] != (Bd, Hd):
            raise ValueError("lara_amd.evaluate: expected depth_pred [B,H,V*W(,1)], tar_dep and tar_msk [B,V,H,W]")
        if image is not None and Bd != B:
            raise ValueError("lara_amd.evaluate: image and depth maps disagree in the number of scenes")
        B = Bd
    if image is None and not have_depth:
        raise ValueError("lara_amd.evaluate: nothing to score")
    first = image if image is not None else depth_pred
    for t in (image, tar_rgb if image is not None else None, depth_pred, tar_dep, tar_msk):
        if t is not None:
            require_device(t)
    dev = first.device
    xv = yv = None
    if image is not None:
        image, tar_rgb = image.detach().float().contiguous(), tar_rgb.detach().float().contiguous()
        xv = _ImgView(image.data_ptr() + 4 * skip_views * W * 3, H * V * W * 3, 1, V * W * 3, W * 3, 3, W)
        yv = _ImgView(tar_rgb.data_ptr() + 4 * skip_views * H * W * 3, V * H * W * 3, 1, W * 3, H * W * 3, 3, W)
    msk_bytes = 1
    if have_depth:
        depth_pred, tar_dep = depth_pred.detach().float().contiguous(), tar_dep.detach().float().contiguous()
        tar_msk = tar_msk.detach()
        if tar_msk.dtype == torch.float32:
            msk_bytes = 4
        elif tar_msk.dtype not in (torch.uint8, torch.bool):
            tar_msk = (tar_msk != 0).to(torch.uint8)          # `.bool()` of any other type
        tar_msk = tar_msk.contiguous()
    nws = query("lara_eval_workspace_doubles", B, H, Wc, Vd, Hd, Wd,
                error=ValueError("lara_amd.evaluate: sizes out of range for lara_eval_scores"))
    ws = torch.empty(nws, dtype=torch.float64, device=dev)
    scores = torch.empty(B, ROW, dtype=torch.float64, device=dev)
    thr = host_array("d", thresholds or [0.0])
    call("lara_eval_scores", dev, B, H, Wc, xv, yv, _window_host(), Vd, Hd, Wd, depth_pred, tar_dep, tar_msk, msk_bytes,
         len(thresholds), thr, scores, ws)
    return scores


def scores_from_rows(rows, n_thresholds=0, image=True, depth=False):
    """Host side of ``scene_scores``: rows [B][16] (Python floats) -> per scene {'psnr', 'ssim', 'depth_acc'} as
    evaluation.py:85, :87 (mean of the three channels), :107-110 compute them; None where that score was not asked for."""
    out = []
    for r in rows:
        s = {"psnr": None, "ssim": None, "depth_acc": None}
        if image:
            mse = r[0] / r[1]
            s["psnr"] = -10.0 * math.log10(mse) if mse > 0 else math.inf
            s["ssim"] = (r[2] + r[3] + r[4]) / 3.0
        if depth:
            n = r[5]          # an empty mask: numpy's mean of nothing, NaN
            s["depth_acc"] = [r[6] / n if n else math.nan] + [r[7 + k] / n if n else math.nan for k in range(n_thresholds)]
        out.append(s)
    return out


@torch.no_grad()
def scene_scores(batch, output, n_views, novel_view_only=True, eval_depth=(), prex="_fine"):
    """Per scene of the batch: {'psnr', 'ssim', 'depth_acc' = [mean abs error, acc@t1, ...]} as evaluation.py:92-111 appends
    them (the reference scores scene 0 of a batch of one; here every scene gets its row).  ``n_views``: the input views
    the "novel views only" crop drops (``cfg.n_views``); if it leaves no columns there are no image scores (:83: psnr and
    ssim are None).  ``eval_depth``: the thresholds (``cfg.infer.eval_depth``; empty = no depth scores, :97).  One kernel
    pass, one device-to-host copy.  SSIM parity with `pytorch_msssim` is unpinned; LPIPS is `lara_amd.lpips.scene_lpips`'s."""
    eval_depth = list(eval_depth)
    image, tar = output[f"image{prex}"], batch["tar_rgb"]
    V = tar.shape[1]
    skip = int(n_views) if novel_view_only else 0
    with_image = skip < V
    depth = len(eval_depth) > 0
    if not with_image and not depth:
        for t in (image, tar):
            require_device(t)
        return [{"psnr": None, "ssim": None, "depth_acc": None} for _ in range(tar.shape[0])]
    dev_rows = scores_device(image if with_image else None, tar, skip,
                             output[f"depth{prex}"] if depth else None, batch["tar_dep"] if depth else None,
                             batch["tar_msk"] if depth else None, eval_depth)
    rows = dev_rows.cpu().tolist()                     # the one host read of the call
    return scores_from_rows(rows, len(eval_depth), with_image, depth)


# ---------------------------------------------------------------------------------------------------------- camera paths

_GOBJ = ("gobjeverse", "GSO")
_I3D_VIDEO = ("instant3d", "mvgen")
_I3D_MESH = ("instant3d", "co3d", "mvgen")
# generate_instant3d_frames' constants (tools/gen_video_path.py:56-66) as the float32 numbers the reference holds
_I3D_ROT = [[-7.0710677e-01, 2.4184476e-01, -6.6446304e-01], [7.0710677e-01, 2.4184476e-01, -6.6446304e-01],
            [-5.2163419e-17, -9.3969262e-01, -3.4202015e-01]]
_I3D_POS = [1.328926, 1.328926, 6.8404031e-01]
_I3D_TRANSFORM = [[-7.0710677e-01, 7.0710677e-01, 7.8504622e-17, 0.0], [2.4184476e-01, 2.4184476e-01, -9.3969262e-01, 0.0],
                  [-6.6446304e-01, -6.6446304e-01, -3.4202015e-01, 0.0], [0.0, 0.0, 0.0, 1.0]]


def _instant3d_c2w(n, elevation_deg=0.0):
    """tools/gen_video_path.py:52-60, :72-78: the canonical instant3d pose tilted about +x, rotated about +z in steps of
    2*pi/n.  [n,4,4] float64 (the reference multiplies the step matrix up in fp32, one product per frame)."""
    base = torch.eye(4, dtype=torch.float64)
    base[:3, :3] = torch.tensor(_I3D_ROT, dtype=torch.float32).double()
    base[:3, 3] = torch.tensor(_I3D_POS, dtype=torch.float32).double()
    a = elevation_deg / 180.0 * math.pi
    rx = torch.eye(4, dtype=torch.float64)
    rx[1, 1], rx[1, 2], rx[2, 1], rx[2, 2] = math.cos(a), -math.sin(a), math.sin(a), math.cos(a)
    base = rx @ base
    out = []
    for i in range(n):
        a = 2.0 * math.pi * i / n
        rz = torch.eye(4, dtype=torch.float64)
        rz[0, 0], rz[0, 1], rz[1, 0], rz[1, 1] = math.cos(a), -math.sin(a), math.sin(a), math.cos(a)
        out.append(rz @ base)
    return torch.stack(out)


def _fov_pair(fov, default):
    if fov is None:
        return default, default
    return tuple(float(torch.as_tensor(f).reshape(-1)[0]) for f in fov[:2])      # `fov[0].item(), fov[1].item()`


def _path_c2w(n, dataset_name, sample, fov, elevation, families):
    """(c2w [n,4,4] float32 with the sample's transform applied on the left, fovx, fovy, znear, zfar) of one orbit."""
    if dataset_name == "unposed":
        raise NotImplementedError("lara_amd.evaluate: the 'unposed' camera path needs the nerfstudio pose interpolation of the "
                                  "reference's tools/camera_utils.py (get_interpolated_poses_many), which is not restated here")
    tm = None if sample is None else torch.as_tensor(sample["transform_mats"][0]).detach().cpu().reshape(4, 4).double()
    if dataset_name in _GOBJ:
        fovx, fovy = 0.75, 0.75                        # (sic) gen_video_path.py:16 overwrites whatever `fov` said
        near, far = 0.5, 2.5
        c2w = _cameras.turntable_c2w(n, float(elevation)).double()
        if tm is None:
            tm = torch.eye(4, dtype=torch.float64)
    elif dataset_name in families:
        fovx, fovy = _fov_pair(fov, 0.7)
        near, far = 1.0, 3.0
        c2w = _instant3d_c2w(n, float(elevation))
        if tm is None:
            tm = torch.tensor(_I3D_TRANSFORM, dtype=torch.float32).double()
    else:
        raise ValueError(f"lara_amd.evaluate: no camera path for dataset {dataset_name!r}")
    return (tm @ c2w).float(), fovx, fovy, near, far


def _build(c2w, img_size, fovx, fovy, near, far, device):
    width, height = img_size
    cams = _cameras.make_cameras(c2w, width, height, fovx, fovy, near, far, device=device)
    c2w_dev = c2w.contiguous().to(cams[0].world_view_transform.device)
    for i, cam in enumerate(cams):
        cam.view_world_transform = c2w_dev[i]          # as the reference's MiniCam keeps it (tools/camera.py:39): the rays' pose
    return cams


def video_cameras(n, dataset_name, img_size, sample=None, fov=None, elevation=0, device=None):
    """``uni_video_path(n, cfg.infer.dataset, sample, fov)`` (tools/gen_video_path.py:107-115) for the 'gobjeverse' / 'GSO' and
    'instant3d' / 'mvgen' families: n `lara_amd.cameras.Camera`s on one orbit, built in one batched pass.  ``img_size`` =
    (width, height).  The reference's quirks are kept: the gobjaverse path ignores ``fov`` (0.75), ``sample['transform_mats'][0]``
    multiplies from the left.  Each camera also carries ``view_world_transform`` (its c2w).  'unposed' raises
    NotImplementedError."""
    c2w, fovx, fovy, near, far = _path_c2w(int(n), dataset_name, sample, fov, elevation, _I3D_VIDEO)
    return _build(c2w, img_size, fovx, fovy, near, far, device)


def mesh_cameras(n, dataset_name, img_size, sample=None, fov=None, device=None):
    """``uni_mesh_path(n, cfg.infer.dataset, sample, fov)`` (tools/gen_video_path.py:117-129): the orbit at elevations 0, -30
    and 30 degrees, 3 n cameras; pass them to ``MeshExtractor.extract(cams=...)``."""
    parts = [_path_c2w(int(n), dataset_name, sample, fov, e, _I3D_MESH) for e in (0, -30, 30)]
    _, fovx, fovy, near, far = parts[0]
    return _build(torch.cat([p[0] for p in parts]), img_size, fovx, fovy, near, far, device)


# ---------------------------------------------------------------------------------------------------------- frames

def quantize_frames(image, rend_normal, acc_map, n=None):
    """uint8 frames of evaluation.py:131-135 from float maps on the device: ``image`` / ``rend_normal`` [H, n*W, 3] and ``acc_map``
    [H, n*W(, 1)] side by side (pass ``n``), or per view [n, H, W, 3] / [n, H, W(, 1)].  Returns (frames, normal_frames), both
    [n, H, W, 3] uint8: rint(image * 255) and rint((((normal * alpha + 1 - alpha) + 1) / 2) * 255), ties to even, clamped."""
    for t in (image, rend_normal, acc_map):
        require_device(t)
    image, rend_normal, acc_map = (t.detach().float().contiguous() for t in (image, rend_normal, acc_map))
    if image.dim() == 3:
        if n is None:
            raise ValueError("lara_amd.evaluate: side-by-side maps need the number of views n")
        H, nW = image.shape[:2]
        if nW % n:
            raise ValueError("lara_amd.evaluate: the strip's width is not a multiple of n")
        W = nW // n
        sV, sY = W, nW
    else:
        n, H, W = image.shape[:3]
        sV, sY = H * W, W
    if image.numel() != n * H * W * 3 or rend_normal.shape != image.shape or acc_map.numel() != n * H * W:
        raise ValueError("lara_amd.evaluate: image, rend_normal and acc_map disagree in size")
    frames = torch.empty(n, H, W, 3, dtype=torch.uint8, device=image.device)
    normals = torch.empty_like(frames)
    call("lara_eval_quantize_frames", image.device, n, H, W, sV, sY, image, rend_normal, acc_map, frames, normals)
    return frames, normals


def _cam_c2w(cam):
    c2w = getattr(cam, "view_world_transform", None)
    if c2w is None:
        c2w = torch.linalg.inv(cam.world_view_transform.detach().double().T)
    return torch.as_tensor(c2w).detach().float()


@torch.no_grad()
def render_turntable(renderer, gs_params, cams, chunk=8, bg=None):
    """evaluation.py:122-138 without the per-frame host work: rays on the device (`lara_amd.batch.build_rays`),
    ``renderer.render_views(..., concat=True)`` ``chunk`` cameras at a time (the last chunk may be shorter), each chunk quantised
    by one kernel.  ``gs_params``: the reference's ``output['render_pkg'][1]`` -- a 5-tuple (centers, shs, opacity, scaling,
    rotation) is used as is; of the fine 6-tuple (..., mask) opacity / scaling / rotation are indexed by ``mask`` and centres /
    shs taken as they are (:123, :129).  ``bg``: one background colour [3] for every view (default: the renderer's).
    Returns (frames, normal_frames): two device uint8 tensors [N, H, W, 3]."""
    from .batch import build_rays, fov_to_ixt
    cams = list(cams)
    if len(gs_params) == 6:
        centers, shs, opacity, scaling, rotation, mask = gs_params
        opacity, scaling, rotation = opacity[mask], scaling[mask], rotation[mask]
    else:
        centers, shs, opacity, scaling, rotation = gs_params
    require_device(centers)
    dev = centers.device
    N = len(cams)
    H, W = int(cams[0].image_height), int(cams[0].image_width)
    if any((int(c.image_height), int(c.image_width)) != (H, W) for c in cams):
        raise ValueError("lara_amd.evaluate: the cameras of a turntable must share one image size")
    frames = torch.empty(N, H, W, 3, dtype=torch.uint8, device=dev)
    normals = torch.empty_like(frames)
    if N == 0:
        return frames, normals
    for cam in cams:
        if hasattr(cam, "to_device"):
            cam.to_device(dev)
    c2w = torch.stack([_cam_c2w(cam) for cam in cams]).to(dev)
    ixt = torch.stack([fov_to_ixt(torch.tensor((cam.FoVx, cam.FoVy)), (W, H)) for cam in cams]).to(dev)
    for o in range(0, N, max(int(chunk), 1)):
        part = cams[o:o + max(int(chunk), 1)]
        n = len(part)
        rays = build_rays(c2w[o:o + n], ixt[o:o + n], H, W)            # as tools/camera.py:54-57, one call for the chunk
        bgs = None if bg is None else torch.as_tensor(bg, dtype=torch.float32, device=dev).reshape(1, 3).expand(n, 3)
        out = renderer.render_views(part, rays, centers, shs, opacity, scaling, rotation, dev, bg_colors=bgs, concat=True)
        img, nrm, acc = (out[k].contiguous() for k in ("image", "rend_normal", "acc_map"))
        call("lara_eval_quantize_frames", dev, n, H, W, W, n * W, img, nrm, acc, frames[o:o + n], normals[o:o + n])
    return frames, normals


def render_mesh_turntable(mesh, cams, chunk=8):
    """evaluation.py:150-155 (``infer.mesh_video_frames > 0``) without Mitsuba: the extracted mesh -- a (vertices, triangles[,
    colors]) tuple on the device, as ``MeshExtractor.extract`` returns it -- seen from ``cams`` through the z-buffer rasteriser
    of `lara_amd.meshrender`, ``chunk`` cameras at a time.  Returns the device uint8 tensor [N, H, W, 3]; the frames register
    pixel for pixel with ``render_turntable``'s for the same cameras."""
    from .meshrender import render_mesh_views
    return render_mesh_views(cams, mesh[0], mesh[1], mesh[2] if len(mesh) > 2 else None, chunk=chunk)["frames"]


def save_surfels(path, render_pkg_item, min_opacity=None, thickness=None, format="ply"):
    """One entry of ``output['render_pkg']`` (the coarse 5-tuple or the fine 6-tuple) as a 2DGS ``point_cloud.ply`` beside the
    mesh (`lara_amd.splatio`: the pre-activation values, bit for bit); ``min_opacity`` drops the surfels at or below it first,
    ``thickness`` adds a third scale for 3DGS viewers.  ``format`` "compressed" or "splat" writes the lossy packed files of
    `lara_amd.splatpack` for web viewers instead (thickness 1e-3 when None; rows with non-finite words are dropped there and not
    counted here).  Returns the number of surfels written."""
    from . import splatio
    cloud = splatio.SurfelCloud.from_render_pkg(render_pkg_item)
    cloud = cloud if min_opacity is None else splatio.select(cloud, min_opacity=min_opacity)[0]
    if format == "ply":
        splatio.write_ply(path, cloud, thickness)
    else:
        from . import splatpack
        splatpack.write(path, cloud, format=format, thickness=thickness)
    return cloud.n_surfels


# ---------------------------------------------------------------------------------------------------------- accumulation

class Evaluator:
    """Accumulates scenes as the lists of evaluation.py:51-52 and writes the JSON of :164-176 (same keys, same means).
    ``lpips``: optional {'vgg': f, 'alex': f}.  A `lara_amd.lpips.LPIPS` instance scores the whole batch where the tensors lie
    (`lara_amd.lpips.scene_lpips`: no permuted copies, one host read per batch for all such networks); any other callable is used
    as f(img_gt * 2 - 1, images * 2 - 1) -> scalar on [1, 3, H, W'] tensors (:89-90); without them the LPIPS entries are written
    as null.  SSIM parity with `pytorch_msssim` and LPIPS parity with `lpips` are unpinned (module docstrings)."""

    def __init__(self, n_views, novel_view_only=True, eval_depth=(), lpips=None, prex="_fine"):
        self.n_views, self.novel_view_only, self.eval_depth, self.prex = int(n_views), bool(novel_view_only), list(eval_depth), prex
        self.lpips = dict(lpips or {})
        self.names, self.depth_accs = [], []
        self.psnrs, self.ssims, self.lpips_vggs, self.lpips_alexs = [], [], [], []
        self.geometry = []          # [(name, scores)] of add_geometry; empty: the JSON is the reference's
        self.volume = []            # [(name, volume_iou)] of add_volume; empty: no key of it is written
        self.topology = []          # [(name, report)] of add_topology; empty: no key of it is written

    def add_scores(self, name, psnr=None, ssim=None, depth_acc=None, lpips_vgg=None, lpips_alex=None):
        """One scene's numbers (evaluation.py:92-95, :111, :113)."""
        if psnr is not None:
            self.psnrs.append(float(psnr))
            self.ssims.append(float(ssim))
            self.lpips_vggs.append(None if lpips_vgg is None else float(lpips_vgg))
            self.lpips_alexs.append(None if lpips_alex is None else float(lpips_alex))
        if depth_acc is not None:
            self.depth_accs.append([float(x) for x in depth_acc])
        self.names.append(name)

    @torch.no_grad()
    def add(self, batch, output, names=None):
        """Scores every scene of the batch (``scene_scores``) and appends them; returns the per-scene dictionaries."""
        scores = scene_scores(batch, output, self.n_views, self.novel_view_only, self.eval_depth, self.prex)
        if names is None:
            names = [str(s).split(".")[0] for s in batch["meta"]["scene"]]            # evaluation.py:63
        skip = self.n_views if self.novel_view_only else 0
        from .lpips import LPIPS, scene_lpips
        ours = {k: f for k, f in self.lpips.items() if isinstance(f, LPIPS)}
        theirs = {k: f for k, f in self.lpips.items() if k not in ours}
        with_image = bool(scores) and scores[0]["psnr"] is not None
        on_device = scene_lpips(ours, output[f"image{self.prex}"], batch["tar_rgb"], skip) if ours and with_image else None
        for b, (name, s) in enumerate(zip(names, scores)):
            lp = {}
            if s["psnr"] is not None and theirs:
                W = batch["tar_rgb"].shape[3]
                img = output[f"image{self.prex}"][b].permute(2, 0, 1)[None][..., W * skip:]
                gt = batch["tar_rgb"][b].permute(1, 0, 2, 3).reshape(output[f"image{self.prex}"][b].shape).permute(2, 0, 1)[None][..., W * skip:]
                lp = {k: float(f(gt * 2 - 1, img * 2 - 1)) for k, f in theirs.items()}
            if on_device is not None:
                lp.update(on_device[b])
            self.add_scores(name, s["psnr"], s["ssim"], s["depth_acc"], lp.get("vgg"), lp.get("alex"))
        return scores

    def add_geometry(self, name, scores):
        """One scene's geometry scores: the dict `lara_amd.meshmetrics.surface_scores` returns (the extracted mesh against the
        ground truth).  Scenes scored here need not be the scenes of ``add``; their names go under ``geometry_name``."""
        keep = {k: scores[k] for k in self.GEOMETRY_SCALARS + self.GEOMETRY_LISTS}
        keep["thresholds"] = [float(t) for t in scores["thresholds"]]
        if self.geometry and keep["thresholds"] != self.geometry[0][1]["thresholds"]:
            raise ValueError("lara_amd.evaluate: the scenes of one Evaluator share their geometry thresholds")
        self.geometry.append((name, keep))

    def add_volume(self, name, scores):
        """One scene's volumetric IoU: the dict `lara_amd.meshsign.volume_scores` returns.  Written as ``volume_name``,
        ``volume_iou`` and ``volume_iou_mean`` (None where a scene has None), behind every other key."""
        iou = scores["volume_iou"]
        self.volume.append((name, None if iou is None else float(iou)))

    def _volume_summary(self):
        vals = [v for _, v in self.volume]
        return {"volume_name": [n for n, _ in self.volume], "volume_iou": vals, "volume_iou_mean": self._mean(vals)}

    def add_topology(self, name, report):
        """One scene's mesh connectivity: the dict `lara_amd.meshtopo.MeshTopology.report` returns.  Written as ``topology_name``,
        ``topology_closed``, ``topology_oriented``, ``topology_boundary_edges``, ``topology_nonmanifold_edges`` and
        ``topology_euler``, one entry per scene, behind every other key."""
        self.topology.append((name, {"closed": bool(report["is_closed"]), "oriented": bool(report["is_oriented"]),
                                     "boundary_edges": int(report["n_boundary"]), "nonmanifold_edges": int(report["n_nonmanifold"]),
                                     "euler": int(report["euler"])}))

    def _topology_summary(self):
        out = {"topology_name": [n for n, _ in self.topology]}
        for k in ("closed", "oriented", "boundary_edges", "nonmanifold_edges", "euler"):
            out["topology_" + k] = [r[k] for _, r in self.topology]
        return out

    GEOMETRY_SCALARS = ("accuracy", "completeness", "chamfer", "chamfer_sq", "normal_consistency")
    GEOMETRY_LISTS = ("precision", "recall", "fscore")          # one entry per threshold

    def _geometry_summary(self):
        """Per-scene lists and their means, as the image scores are written: a scalar key holds one number per scene, a
        per-threshold key one list per scene; ``<key>_mean`` the mean over scenes (None where a scene has None)."""
        out = {"geometry_name": [n for n, _ in self.geometry], "geometry_thresholds": list(self.geometry[0][1]["thresholds"])}
        for k in self.GEOMETRY_SCALARS:
            vals = [None if s[k] is None else float(s[k]) for _, s in self.geometry]
            out[k], out[k + "_mean"] = vals, self._mean(vals)
        for k in self.GEOMETRY_LISTS:
            vals = [[float(x) for x in s[k]] for _, s in self.geometry]
            out[k], out[k + "_mean"] = vals, [sum(c) / len(c) for c in zip(*vals)]
        return out

    @staticmethod
    def _mean(values):
        return None if any(v is None for v in values) else sum(values) / len(values)

    def summary(self):
        """The dictionary evaluation.py:167-172 dumps ('depth_acc' ends up holding the MEAN: the reference's update overwrites
        the per-scene list under the same key), or None when no scene had image scores (:164)."""
        if not self.psnrs:
            out = self._geometry_summary() if self.geometry else None
            if self.volume:
                out = dict(out or {}, **self._volume_summary())
            if self.topology:
                out = dict(out or {}, **self._topology_summary())
            return out
        if self.eval_depth and self.depth_accs:
            cols = list(zip(*self.depth_accs))
            mean_depth = [sum(c) / len(c) for c in cols]
        else:
            mean_depth = 0.0
        out = {"name": list(self.names), "psnr": list(self.psnrs), "ssim": list(self.ssims), "lpips_vgg": list(self.lpips_vggs),
               "lpips_alex": list(self.lpips_alexs), "depth_acc": mean_depth, "psnr_mean": self._mean(self.psnrs),
               "ssim_mean": self._mean(self.ssims), "lpips_vgg_mean": self._mean(self.lpips_vggs),
               "lpips_alex_mean": self._mean(self.lpips_alexs)}
        if self.geometry:          # (behind the reference's keys, and only when add_geometry was called)
            out.update(self._geometry_summary())
        if self.volume:            # (likewise, and only when add_volume was called)
            out.update(self._volume_summary())
        if self.topology:          # (likewise, and only when add_topology was called)
            out.update(self._topology_summary())
        return out

    def write(self, metric_path):
        """evaluation.py:164-176; returns the dictionary written (None, and no file, when there is nothing to write)."""
        scores = self.summary()
        if scores is None or metric_path is None:
            return scores
        d = os.path.dirname(metric_path)
        if d:
            os.makedirs(d, exist_ok=True)
        with open(metric_path, "w") as f:
            json.dump(scores, f, indent=4)
        return scores
