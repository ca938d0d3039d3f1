"""The mesh turntable of LaRa's evaluation loop (evaluation.py:150-155, tools/meshRender.py) on the device: a deterministic
z-buffer triangle rasteriser (include/lara_meshrender.h, csrc/meshrender.hip); opt-in like every module here.

The reference hands the mesh to Mitsuba (rough plastic under an HDR environment, 512 path-traced samples per pixel and frame).
Mitsuba is not available and its image is not imitated.  What a user of ``lara_amd.mesh.MeshExtractor`` gets here is the mesh
seen from the cameras of the surfel rasteriser, in its pixel convention: exact visibility (``face_id``), view-space ``depth``
(the convention ``TSDFVolume.integrate`` takes), world-space face ``normal`` and head-lit uint8 ``frames``.  Flat shading, no
anti-aliasing, no near-plane clipping (a triangle with a vertex at or behind ``znear`` is dropped and counted in ``info``).

  * ``render_mesh_views``  the outputs asked for, as a dict of device tensors; views run ``chunk`` at a time;
  * ``render_mesh``        the reference's ``tools/meshRender.render_mesh(cams, mesh, white_bg)`` signature: uint8 [N, H, W, 3].

No CPU path: tensors must live on the GPU.
"""
from __future__ import annotations

import os

import torch

from ._native import StreamWorkspace, call, host_array, query, require_device

ALBEDO = (0.25, 0.5, 0.8)               # configs/render/scene.xml: the bsdf's diffuse_reflectance
BACKGROUND = (0.722, 0.376, 0.161)      # tools/meshRender.py:44
AMBIENT, DIFFUSE = 0.25, 0.75
OUTPUTS = ("face_id", "depth", "normal", "frames", "info")
SUBPIXEL, RANGE, FAR = 256, 1 << 22, 1 << 30      # include/lara_meshrender.h

_workspace = StreamWorkspace()      # its own: sections of it stay alive across calls


def section_offsets(n_views, H, W, Nv, T):
    """Byte offsets of the workspace's (SNAP, KEYS, LIST, COUNT) sections (include/lara_meshrender.h)."""
    offs = host_array("l", 4)
    call("lara_meshrender_section_offsets", None, n_views, H, W, Nv, T, offs)
    return tuple(offs)


def workspace_sections(ws, n_views, H, W, Nv, T):
    """Views of a workspace a call has filled: (snap [n, Nv, 4] int32 -- x, y in 1/256 pixel, the bits of view z, 0 --,
    keys [n, H, W] int64 -- (depth bits << 32) | triangle id, -1 = background)."""
    o_snap, o_keys, _, _ = section_offsets(n_views, H, W, Nv, T)
    snap = ws[o_snap:o_snap + n_views * Nv * 16].view(torch.int32).view(n_views, Nv, 4)
    keys = ws[o_keys:o_keys + n_views * H * W * 8].view(torch.int64).view(n_views, H, W)
    return snap, keys


def camera_tensors(cams, dev):
    """(viewmatrix [n,16], projmatrix [n,16], eye [n,3]) of ``lara_amd.cameras`` cameras (or the reference's MiniCams): the two
    matrices the surfel rasteriser takes, and the camera's true position -- the translation of the inverse of
    world_view_transform^T, not ``camera_center`` (which the reference negates).  Batched; no host read."""
    view = torch.stack([torch.as_tensor(c.world_view_transform).detach().to(dev, torch.float32) for c in cams])
    proj = torch.stack([torch.as_tensor(c.full_proj_transform).detach().to(dev, torch.float32) for c in cams])
    c2w = torch.linalg.inv_ex(view.double().transpose(1, 2))[0]
    eye = c2w[:, :3, 3].float().contiguous()
    return view.reshape(-1, 16).contiguous(), proj.reshape(-1, 16).contiguous(), eye


@torch.no_grad()
def render_mesh_views(cams, vertices, triangles, colors=None, *, chunk=8, albedo=ALBEDO, background=BACKGROUND,
                      ambient=AMBIENT, diffuse=DIFFUSE, outputs=("frames",), znear=None, wave_box_area=0, check=True,
                      keep_workspace=False):
    """The mesh (``vertices`` [Nv,3] fp32 on the device, ``triangles`` [T,3] of any integer type, ``colors`` [Nv,3] or None for
    the constant ``albedo``) seen from ``cams`` (``lara_amd.cameras`` cameras: ``evaluate.video_cameras`` / ``mesh_cameras``,
    ``pipeline.scene_cameras``), which share one image size.  Returns a dict of device tensors for the names in ``outputs``:

      face_id [N,H,W] int32 (-1 = background), depth [N,H,W] fp32 (view-space z, 0 = background), normal [N,H,W,3] fp32 (unit
      face normal towards the camera, 0 = background), frames [N,H,W,3] uint8 (albedo x (ambient + diffuse x max(0, n.l)) under
      a head light, ``background`` elsewhere), info [N,4] int32 (triangles drawn, dropped behind ``znear``, degenerate, out of
      the +-2^22-unit coordinate range).

    Views run ``chunk`` at a time (the last chunk may be shorter) on a workspace cached per stream.  ``znear``: the cameras'
    own (default).  Triangles indexing outside [0, Nv) raise: the kernels drop them and set an error word, which is read ONCE
    per call, after every chunk has been enqueued -- the call's only host read; ``check=False`` skips it and returns the word as
    ``"error"`` (a device int32) instead.  ``wave_box_area``: the box area from which a wave draws a triangle (0: the library's
    constant; tests force both shapes).  ``keep_workspace``: also return ``"workspace"``, the last chunk's (bytes, n_views)."""
    cams = list(cams)
    outputs = tuple(outputs)
    for name in outputs:
        if name not in OUTPUTS:
            raise ValueError(f"lara_amd.meshrender: unknown output {name!r}; choose from {OUTPUTS}")
    require_device(vertices)
    dev = vertices.device
    V = vertices.detach().to(torch.float32).contiguous()
    if V.dim() != 2 or V.shape[1] != 3 or triangles.dim() != 2 or triangles.shape[1] != 3:
        raise RuntimeError("lara_amd.meshrender: expected vertices [Nv,3] and triangles [T,3]")
    Nv, T = V.shape[0], triangles.shape[0]
    if Nv >= 2 ** 30 or T >= 2 ** 30:
        raise RuntimeError("lara_amd.meshrender: meshes need Nv < 2^30 and T < 2^30")
    F = triangles.to(device=dev, dtype=torch.int32).contiguous()
    C = None if colors is None else colors.detach().to(dev, torch.float32).contiguous()
    if C is not None and tuple(C.shape) != (Nv, 3):
        raise RuntimeError("lara_amd.meshrender: expected colors [Nv,3]")
    N = len(cams)
    if N == 0:
        raise ValueError("lara_amd.meshrender: no cameras")
    H, W = int(cams[0].image_height), int(cams[0].image_width)
    if any((int(c.image_height), int(c.image_width)) != (H, W) for c in cams):
        raise ValueError("lara_amd.meshrender: the cameras of a call must share one image size")
    znear = float(cams[0].znear if znear is None else znear)
    shading = host_array("f", [float(x) for x in (*albedo, *background, ambient, diffuse)])
    view, proj, eye = camera_tensors(cams, dev)
    kinds = {"face_id": ((N, H, W), torch.int32), "depth": ((N, H, W), torch.float32), "normal": ((N, H, W, 3), torch.float32),
             "frames": ((N, H, W, 3), torch.uint8), "info": ((N, 4), torch.int32)}
    out = {k: torch.empty(kinds[k][0], dtype=kinds[k][1], device=dev) for k in outputs}
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    step = max(int(chunk), 1)
    nbytes = query("lara_meshrender_workspace_bytes", min(step, N), H, W, Nv, T,
                   error=ValueError("lara_amd.meshrender: sizes out of range for lara_meshrender_views"))
    ws = _workspace(dev, nbytes)
    n = 0
    for o in range(0, N, step):
        n = min(step, N - o)
        part = [out[k][o:o + n] if k in out else None for k in OUTPUTS]
        call("lara_meshrender_views", dev, n, H, W, Nv, T, V, F, C, view[o:o + n], proj[o:o + n], eye[o:o + n], znear, shading,
             int(wave_box_area), *part, err, ws)
    if check:
        if int(err.item()) & 1:          # the one host read of the call
            raise RuntimeError("lara_amd.meshrender.render_mesh_views: a triangle indexes a vertex outside [0, Nv)")
    else:
        out["error"] = err
    if keep_workspace:
        out["workspace"] = (ws, n)
    return out


def render_mesh(cams, mesh, white_bg=True):
    """``tools/meshRender.render_mesh(cams, mesh, white_bg)``: uint8 frames [N, H, W, 3] on the device.  ``mesh``: a path (read
    with ``lara_amd.mesh.read_obj``) or a (vertices, triangles[, colors]) tuple; vertex colours, where the mesh has them, are the
    albedo.  ``white_bg``: a white background, else the reference's (0.722, 0.376, 0.161)."""
    if isinstance(mesh, (str, os.PathLike)):
        from .mesh import read_obj
        mesh = read_obj(mesh)
    vertices, triangles = mesh[0], mesh[1]
    colors = mesh[2] if len(mesh) > 2 else None
    cams = list(cams)
    dev = vertices.device if isinstance(vertices, torch.Tensor) else torch.as_tensor(cams[0].world_view_transform).device
    if dev.type != "cuda" and not isinstance(vertices, torch.Tensor):
        dev = torch.device("cuda", torch.cuda.current_device())          # a file's mesh goes to the current device
    to = lambda a, dt: None if a is None else torch.as_tensor(a).to(dev, dt)
    bg = (1.0, 1.0, 1.0) if white_bg else BACKGROUND
    return render_mesh_views(cams, to(vertices, torch.float32), to(triangles, torch.int64), to(colors, torch.float32),
                             background=bg)["frames"]
