"""Ray queries on a mesh's triangles on the device: the first triangle a ray meets, whether it meets any, which eyes see a point
past the mesh, and depth maps of the mesh (include/lara_meshray.h, csrc/meshray.hip, csrc/raytri.h, csrc/raybox.h); opt-in
like every module here.  Every function takes a built ``meshbvh.TriangleBVH`` and walks the buffer it holds; nothing is added to it.

  * ``raycast``       per ray the smallest t with o + t d on a triangle, inside [t_min, t_max], and that triangle (an exact tie: the
                      smaller face id); d is not normalised.  Equal to brute force over all triangles bit for bit: the
                      ray-triangle function is one sequence of double operations, the same on the host, and the walk only skips
                      boxes a margined bound proves free of hits.  Watertight: a ray cannot slip between two triangles that share
                      an edge or a vertex;
  * ``occluded``      whether anything is hit in the window: the same walk, ended by the first hit;
  * ``visibility``    for N points and up to 64 eyes an int64 mask per point: bit e is set when the segment from eye e to the point,
                      less its last ``shrink``, meets no triangle (``faces``: the triangle each point lies on, ignored);
  * ``render_depth``  view-space depth and face maps through pixel centres, ``depthsurface.cameras``' convention.

``depthsurface.observe(occluder=...)`` and ``depthsurface.depth_scores(self_occlusion=True)`` come here.  No CPU path: tensors
must live on the GPU.  No host reads.
"""
from __future__ import annotations

import math

import torch

from ._native import call, rows3

MAX_EYES = 64                                                    # include/lara_meshray.h
MASKED_ORDER = 1


def _rays(bvh, origins, directions):
    O = origins.detach().to(bvh.device, torch.float32).contiguous()
    D = directions.detach().to(bvh.device, torch.float32).contiguous()
    if O.dim() != 2 or O.shape[1] != 3 or tuple(D.shape) != tuple(O.shape):
        raise RuntimeError("lara_amd.meshray: expected origins [R,3] and directions [R,3]")
    if O.shape[0] >= 1 << 30:
        raise ValueError("lara_amd.meshray: 2^30 rays and more")
    return O, D


def _window(bvh, x, default, R):
    """None for the library's default, else an [R] fp32 tensor: a scalar is spread, a tensor taken as it is."""
    if not isinstance(x, torch.Tensor):
        x = float(x)
        if x == default:
            return None
        return torch.full((R,), x, dtype=torch.float32, device=bvh.device)
    x = x.detach().to(bvh.device, torch.float32).contiguous()
    if tuple(x.shape) != (R,):
        raise RuntimeError("lara_amd.meshray: t_min and t_max are scalars or [R] tensors")
    return x


@torch.no_grad()
def raycast(bvh, origins, directions, t_min=0.0, t_max=math.inf, return_bary=False, *, other_order=False):
    """(t [R] fp32, face [R] int32[, bary [R,3] fp32]) of the rays ``origins`` + t ``directions`` against the triangles of
    ``bvh``: the first hit inside [t_min, t_max] (scalars or [R] tensors).  No hit -- also a ray with a component that is not
    finite or a zero direction, and a mesh without a valid triangle --: t = +inf, face = -1, bary = NaN.  ``other_order``: the
    sibling order the walk does not use by default; the same bits (for benches and tests)."""
    O, D = _rays(bvh, origins, directions)
    R = O.shape[0]
    t = torch.empty(R, dtype=torch.float32, device=bvh.device)
    face = torch.empty(R, dtype=torch.int32, device=bvh.device)
    bary = torch.empty(R, 3, dtype=torch.float32, device=bvh.device) if return_bary else None
    call("lara_meshray_cast_other_order" if other_order else "lara_meshray_cast", bvh.device, R, O, D, _window(bvh, t_min, 0.0, R),
         _window(bvh, t_max, math.inf, R), bvh.bvh, t, face, bary)
    return (t, face, bary) if return_bary else (t, face)


@torch.no_grad()
def occluded(bvh, origins, directions, t_min=0.0, t_max=math.inf):
    """bool [R]: the ray hits some triangle inside [t_min, t_max]; ``raycast(...)[1] >= 0`` without the search for the first."""
    O, D = _rays(bvh, origins, directions)
    R = O.shape[0]
    out = torch.empty(R, dtype=torch.uint8, device=bvh.device)
    call("lara_meshray_occluded", bvh.device, R, O, D, _window(bvh, t_min, 0.0, R), _window(bvh, t_max, math.inf, R), bvh.bvh, out)
    return out.bool()


@torch.no_grad()
def visibility(bvh, points, eyes, faces=None, shrink=2.0 ** -10):
    """int64 [N]: bit e is set when no triangle of ``bvh`` -- but ``faces[i]``, the one point i lies on -- meets the ray from
    ``eyes[e]`` to ``points[i]`` before the last ``shrink`` of it (d = fl32(point - eye), the window [0, 1 - shrink]).  A point
    with a coordinate that is not finite has 0.  At most 64 eyes."""
    P = rows3(points, bvh.device, "points", "meshray")
    E = torch.as_tensor(eyes).detach().to(bvh.device, torch.float32).contiguous()
    if E.dim() != 2 or E.shape[1] != 3 or E.shape[0] > MAX_EYES:
        raise ValueError(f"lara_amd.meshray: expected eyes [E,3] with E <= {MAX_EYES}")
    shrink = float(shrink)
    if not 0.0 <= shrink < 1.0:
        raise ValueError("lara_amd.meshray: shrink must lie in [0, 1)")
    N = P.shape[0]
    if N >= 1 << 30:
        raise ValueError("lara_amd.meshray: 2^30 points and more")
    skip = None
    if faces is not None:
        skip = faces.detach().to(bvh.device, torch.int32).contiguous()
        if tuple(skip.shape) != (N,):
            raise RuntimeError("lara_amd.meshray: faces must be [N]")
    seen = torch.empty(N, dtype=torch.int64, device=bvh.device)
    call("lara_meshray_visible", bvh.device, N, P, skip, E.shape[0], E, shrink, bvh.bvh, seen)
    return seen


def pixel_rays(ixt, c2w, H, W, device):
    """(origins, directions) [V,H,W,3] fp32 on ``device``: pixel (y, x) looks through (x + 0.5, y + 0.5); float64 operations in a
    fixed order, rounded once; the direction has view-space z = 1, so a hit's t is its view-space depth."""
    from .depthsurface import cameras
    k, pose = cameras(ixt, c2w)
    k = torch.from_numpy(k).to(device, torch.float64)
    M = torch.from_numpy(pose).to(device, torch.float64).view(-1, 4, 4)
    x = torch.arange(W, dtype=torch.float64, device=device)[None, None, :]
    y = torch.arange(H, dtype=torch.float64, device=device)[None, :, None]
    a = (((x + 0.5) - k[:, 2, None, None]) / k[:, 0, None, None]).expand(-1, H, W)
    b = (((y + 0.5) - k[:, 3, None, None]) / k[:, 1, None, None]).expand(-1, H, W)
    d = torch.stack([(M[:, j, 0, None, None] * a + M[:, j, 1, None, None] * b) + M[:, j, 2, None, None] for j in range(3)], -1)
    o = M[:, None, None, :3, 3].expand_as(d)
    return o.to(torch.float32).contiguous(), d.to(torch.float32).contiguous()


@torch.no_grad()
def render_depth(bvh, ixt, c2w, H, W):
    """(depth [V,H,W] fp32, face [V,H,W] int32) of the mesh from cameras ``ixt`` [V,3,3], ``c2w`` [V,4,4]: the view-space z of the
    first hit in front of the camera through every pixel centre; a miss gives 0 and face -1.  Torch makes the rays, the cast is
    ``raycast``."""
    H, W = int(H), int(W)
    o, d = pixel_rays(ixt, c2w, H, W, bvh.device)
    V = o.shape[0]
    t, face = raycast(bvh, o.view(-1, 3), d.view(-1, 3))
    depth = torch.where(face >= 0, t, torch.zeros_like(t))
    return depth.view(V, H, W), face.view(V, H, W)
