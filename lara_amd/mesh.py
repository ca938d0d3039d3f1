"""The reference's mesh path on the device: ``MeshExtractor.extract``
(tools/meshExtractor.py:51-135) renders 48 views, fuses them into Open3D's ``ScalableTSDFVolume``, extracts a mesh and
post-processes it on the CPU in Open3D (crop to the box, ``cluster_connected_triangles``, keep the 10 largest clusters,
``remove_unreferenced_vertices``) before writing it.  Here every step runs on library kernels:

* ``clean_mesh``  -- the post-processing (include/lara_meshclean.h, csrc/meshclean.hip), Open3D's semantics [RECALLED];
* ``write_obj``   -- the writer (vectorised text formatting);
* ``MeshExtractor`` -- a drop-in for the reference's class: ``lara_amd.renderer.Renderer.render_views`` for the views,
  ``lara_amd.tsdf.TSDFVolume`` for the fusion and marching cubes, then the two above.

One deliberate difference: the reference raises (``argmax`` of an empty array) when the crop leaves no triangle; here an
empty mesh is returned and written.  No CPU path."""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from ._native import call, host_array, require_device


def _compact(rows, keep, ends, n_out):
    """rows [n, ...] (4- or 8-byte elements) where keep != 0, in order (lara_mesh_compact_rows)."""
    out = torch.empty((n_out,) + tuple(rows.shape[1:]), dtype=rows.dtype, device=rows.device)
    if n_out == 0:
        return out
    width = rows[0].numel() * rows.element_size() // 4 if rows.shape[0] else 1
    call("lara_mesh_compact_rows", rows.device, rows.shape[0], width, rows, keep, ends, out)
    return out


def _raise_on(err_word, what):
    if err_word & 1:
        raise RuntimeError(f"lara_amd.mesh.{what}: a triangle indexes a vertex outside [0, Nv)")
    if err_word & 4:
        raise RuntimeError(f"lara_amd.mesh.{what}: a triangle area is not finite or >= 2^31")


@torch.no_grad()
def clean_mesh(vertices, triangles, colors=None, aabb=None, keep=10):
    """tools/meshExtractor.py:112-134 on the device: crop to ``aabb`` (the config's 6 numbers; scaled by 1.1 here, as
    ``MeshExtractor.__init__`` does; None = no crop), Open3D's ``cluster_connected_triangles``, drop the triangles of every
    cluster smaller than the ``keep``-th largest (ties stay), ``remove_unreferenced_vertices``.

    vertices [Nv,3] (fp32 on the device), triangles [T,3] (any integer type; int64 from ``extract_triangle_mesh``),
    colors [Nv,3] or None.  Returns (vertices, triangles int64, colors, info), ``info`` holding ``triangle_clusters``
    [T'] int32, ``cluster_n_triangles`` [C] int64 and ``cluster_area`` [C] fp64 of the cropped mesh, as the reference
    computes them.  Everything stays on the device; the host reads sizes only (and the kernels' error word with them),
    plus one word per union round inside ``lara_mesh_cluster_labels``."""
    dev = vertices.device
    require_device(dev)
    V = vertices.detach().to(torch.float32).contiguous()
    Nv = V.shape[0]
    if V.dim() != 2 or V.shape[1] != 3 or triangles.dim() != 2 or triangles.shape[1] != 3:
        raise RuntimeError("expected vertices [Nv,3] and triangles [T,3]")
    if Nv >= 2 ** 31 or triangles.shape[0] >= 2 ** 31 // 3:
        raise RuntimeError("lara_amd.mesh.clean_mesh: meshes need Nv < 2^31 and 3 T < 2^31 (int32 indices)")
    F = triangles.to(device=dev, dtype=torch.int32).contiguous()
    C_in = None if colors is None else colors.detach().to(dev).contiguous()
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        if aabb is not None and F.shape[0]:
            box = np.asarray(aabb, np.float64).reshape(2, 3) * 1.1          # meshExtractor.py:37, in double as numpy does
            cbox = host_array("d", box.reshape(-1).tolist())
            inside = torch.empty(F.shape[0], dtype=torch.int32, device=dev)
            call("lara_mesh_crop", dev, Nv, F.shape[0], V, F, cbox, inside, err)
            ends = torch.cumsum(inside, 0, dtype=torch.int64)
            n_in, e = torch.stack([ends[-1], err[0].long()]).tolist()       # host read: the cropped size
            _raise_on(e, "clean_mesh")
            F = _compact(F, inside, ends, n_in)
        T = F.shape[0]
        i32 = dict(dtype=torch.int32, device=dev)
        if T == 0:
            info = {"triangle_clusters": torch.zeros(0, **i32), "cluster_n_triangles": torch.zeros(0, dtype=torch.int64, device=dev),
                    "cluster_area": torch.zeros(0, dtype=torch.float64, device=dev)}
            return (V[:0].clone(), torch.zeros(0, 3, dtype=torch.int64, device=dev),
                    None if C_in is None else C_in[:0].clone(), info)
        cap = 1 << max(6, (6 * T - 1).bit_length())                           # a power of two >= twice the edges
        keys = torch.empty(cap, dtype=torch.int64, device=dev)
        owner = torch.empty(cap, **i32)
        adj = torch.empty(3 * T, **i32)
        label = torch.empty(T, **i32)
        work = torch.empty(2, **i32)
        rounds = host_array("i", 1)                                            # (host word the call writes)
        call("lara_mesh_cluster_labels", dev, T, F, cap, keys, owner, adj, label, work, rounds)
        del keys, owner, adj
        root_ends = torch.cumsum(label == torch.arange(T, **i32), 0, dtype=torch.int64)
        C = int(root_ends[-1])                                                 # host read: the number of clusters
        clusters = torch.empty(T, **i32)
        counts = torch.zeros(C, dtype=torch.int64, device=dev)
        acc = torch.zeros(2 * C, dtype=torch.int64, device=dev)
        area = torch.empty(C, dtype=torch.float64, device=dev)
        call("lara_mesh_cluster_stats", dev, Nv, T, V, F, label, root_ends, C, clusters, counts, acc, area, err)
        # meshExtractor.py:130: n = sort(counts)[-min(C, keep)] -- C is small, one sort; the threshold stays on the device
        i = (C - min(C, int(keep))) % C
        threshold = torch.sort(counts).values[i:i + 1]
        kept = torch.empty(T, **i32)
        referenced = torch.zeros(Nv, **i32)
        call("lara_mesh_keep_clusters", dev, Nv, T, F, clusters, counts, threshold, kept, referenced, err)
        tends = torch.cumsum(kept, 0, dtype=torch.int64)
        vends = torch.cumsum(referenced, 0, dtype=torch.int64)
        T2, Nv2, e = torch.stack([tends[-1], vends[-1], err[0].long()]).tolist()   # host read: the output sizes
        _raise_on(e, "clean_mesh")
        F2 = _compact(F, kept, tends, T2)
        out_t = torch.empty_like(F2)
        call("lara_mesh_remap", dev, Nv, T2, F2, vends, out_t, err)
        V2 = _compact(V, referenced, vends, Nv2)
        C2 = None if C_in is None else _compact(C_in, referenced, vends, Nv2)
    info = {"triangle_clusters": clusters, "cluster_n_triangles": counts, "cluster_area": area, "union_rounds": rounds[0]}
    return V2, out_t.long(), C2, info


def write_obj(path, vertices, triangles, colors=None):
    """Wavefront OBJ: one ``v x y z [r g b]`` line per vertex (``%.9g``: fp32 values read back to the same bits), one
    1-based ``f a b c`` line per triangle; the text is built by vectorised numpy formatting, not a loop per line.
    Open3D's own writer (``o3d.io.write_triangle_mesh``, meshExtractor.py:135) adds a header and picks its own number format;
    neither is pinned by the reference (Open3D absent, version unpinned), so this writer does not imitate them."""
    v = torch.as_tensor(vertices).detach().cpu().numpy().astype(np.float32, copy=False).reshape(-1, 3)
    t = torch.as_tensor(triangles).detach().cpu().numpy().astype(np.int64, copy=False).reshape(-1, 3)
    cols = [v[:, 0], v[:, 1], v[:, 2]]
    if colors is not None:
        c = torch.as_tensor(colors).detach().cpu().numpy().astype(np.float32, copy=False).reshape(-1, 3)
        cols += [c[:, 0], c[:, 1], c[:, 2]]
    parts = []
    if len(v):
        line = np.full(len(v), "v", dtype=object).astype(str)
        for col in cols:
            line = np.char.add(np.char.add(line, " "), np.char.mod("%.9g", col.astype(np.float64)))
        parts.append(line)
    if len(t):
        line = np.full(len(t), "f", dtype=object).astype(str)
        for col in (t + 1).T:
            line = np.char.add(np.char.add(line, " "), col.astype(str))
        parts.append(line)
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    with open(path, "w") as f:
        for p in parts:
            f.write("\n".join(p.tolist()))
            f.write("\n")


def read_obj(path):
    """(vertices [Nv,3] fp32, triangles [T,3] int64 0-based, colors [Nv,3] fp32 or None) of a file ``write_obj`` wrote."""
    vs, fs = [], []
    with open(path) as f:
        for line in f:
            if line.startswith("v "):
                vs.append(line.split()[1:])
            elif line.startswith("f "):
                fs.append(line.split()[1:4])
    v = np.array(vs, np.float64).reshape(-1, len(vs[0]) if vs else 3)
    t = np.array(fs, np.int64).reshape(-1, 3) - 1
    colors = v[:, 3:6].astype(np.float32) if v.shape[1] >= 6 else None
    return v[:, :3].astype(np.float32), t, colors


# ---- MeshExtractor ---------------------------------------------------------------------------------------------------------
# alpha >= 1/255 needs rho <= tau = 2 ln(255 opacity) <= 2 ln 255 (csrc/composite.hip: the same tau, with its margin)
_TAU = 2.0 * math.log(255.0) * 1.001 + 0.01


def _cam_c2w(cam):
    """camera-to-world of the reference's ``MiniCam`` (``view_world_transform``) or of a ``lara_amd.cameras.Camera``
    (the inverse of world_view_transform^T)."""
    c2w = getattr(cam, "view_world_transform", None)
    if c2w is None:
        c2w = torch.linalg.inv(cam.world_view_transform.detach().double().T)
    return torch.as_tensor(c2w).detach().float()


def _intrinsics(cam):
    """(fx, fy, cx, cy) as meshExtractor.py:69-74 builds Open3D's PinholeCameraIntrinsic."""
    W, H = int(cam.image_width), int(cam.image_height)
    return [W / (2 * math.tan(cam.FoVx / 2.0)), H / (2 * math.tan(cam.FoVy / 2.0)), W / 2, H / 2]


class MeshExtractor:
    """Drop-in for the reference's ``MeshExtractor`` (tools/meshExtractor.py:31-135) with every step on the device.
    ``gs_params`` = ``output['render_pkg'][1]`` of ``LaRaPipeline(..., return_buffer=True)`` or of the reference's network:
    (centers[mask], shs, opacity, scaling, rotation, mask).  ``render``: ``lara_amd.renderer.Renderer`` (the views go through
    ``render_views``, ``chunk`` at a time) or any object with the reference's ``render_img``.  As in the reference,
    ``bg_color`` is stored but the renderer's own background is what the views are rendered on."""

    BLOCK = 16        # Open3D's volume unit (ScalableTSDFVolume): the grid's origin and size snap to it

    def __init__(self, gs_params, render, aabb, bg_color=(1.0, 1.0, 1.0)):
        self.background = torch.tensor(bg_color, dtype=torch.float32, device="cuda")
        self.aabb_cfg = None if aabb is None else [float(x) for x in np.asarray(aabb, np.float64).reshape(-1)]
        self.aabb = None if aabb is None else np.array(aabb, np.float64).reshape(2, 3) * 1.1       # meshExtractor.py:37
        self.gs_params = gs_params
        self.render = render
        self.grid_pad_blocks = 0      # extra 16-voxel blocks on every side of the grid (a larger grid gives the same mesh)
        self.last_grid = None         # (origin, voxel_size, resolution) of the last extract
        self.timings = None           # set to a list to collect (stage, start event, end event)

    def _mark(self, name):
        if self.timings is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.timings.append((name, e))

    @staticmethod
    def _grid(lo, hi, voxel, pad_blocks=0):
        """The dense grid covering [lo, hi]: origin snapped outward to multiples of 16 voxels (Open3D's unit lattice), one
        resolution for the three axes, a multiple of 16."""
        unit = MeshExtractor.BLOCK * voxel
        b0 = np.floor(np.asarray(lo, np.float64) / unit) - pad_blocks
        b1 = np.ceil(np.asarray(hi, np.float64) / unit) + pad_blocks
        nb = int(max(1, (b1 - b0).max()))
        return tuple(float(x) for x in b0 * unit), MeshExtractor.BLOCK * nb

    def _gaussian_extent(self, cams, centers, scaling, voxel_size, sdf_trunc):
        """Without an aabb: a box no vertex of the extracted mesh can leave.  A rendered depth is the alpha-weighted mean of
        its pixel's hit depths, so the fused surface point lies on the pixel's ray between two hits and inside any convex set
        holding all hits.  A hit is either a point of the surfel plane with rho3d = |(u, v)|^2 <= tau, i.e. within
        sqrt(tau) * max(scale) of the centre, or (the screen-space low-pass, rho2d <= tau) the centre's depth on a ray
        within sqrt(tau / 2) pixels of the centre's projection (csrc/composite.hip).  The TSDF reads the depth of the pixel
        a voxel projects into (one more pixel of footprint) and marks voxels up to sdf_trunc behind it along the view axis
        (a distance <= sdf_trunc * |ray| with |ray| <= sqrt(1 + tan^2(fovx/2) + tan^2(fovy/2)) for a unit-z ray); a marching
        cubes vertex lies on a grid edge next to such a voxel.  Hence: the centres' box grown by sqrt(tau) * max scale, the
        footprint of sqrt(tau / 2) + 1 pixels at the farthest distance, the truncation along the ray, and two voxels."""
        s = torch.exp(scaling.detach().float()).amax(-1) * math.sqrt(_TAU)
        c = centers.detach().float()
        lo, hi = torch.stack([(c - s[:, None]).amin(0), (c + s[:, None]).amax(0)]).double().cpu().numpy()    # host read: the box
        mid, half = 0.5 * (lo + hi), 0.5 * np.linalg.norm(hi - lo)
        foot, ray = 0.0, 1.0
        for cam in cams:
            fx, fy, _, _ = _intrinsics(cam)
            dist = np.linalg.norm(_cam_c2w(cam)[:3, 3].cpu().numpy().astype(np.float64) - mid) + half
            foot = max(foot, dist * (math.sqrt(_TAU / 2) + 1.0) / min(fx, fy))
            ray = max(ray, math.sqrt(1 + math.tan(cam.FoVx / 2) ** 2 + math.tan(cam.FoVy / 2) ** 2))
        m = foot + sdf_trunc * ray + 2 * voxel_size
        return lo - m, hi + m

    @torch.no_grad()
    def extract(self, save_mesh_path, dataset_name, voxel_size=2 / 256, sdf_trunc=0.08, alpha_thres=0.08, depth_trunc=10,
                sample=None, fov=None, device='cuda', cams=None, chunk=8, *, simplify_voxel=None, simplify_target=None,
                simplify_contraction="quadric", writer="host", smooth_iterations=None, smooth_method="taubin", smooth_lambda=0.5,
                smooth_mu=-0.53, normals=False, texture_patch=None, texture_max_texels=None, texture_blend="weighted"):
        """tools/meshExtractor.py:51-135: render the views, fuse them into a block-sparse TSDF volume (Open3D's
        ``ScalableTSDFVolume`` semantics, lara_amd.tsdf), marching cubes, ``clean_mesh`` (crop to the box, the 10 largest
        clusters), ``write_obj(save_mesh_path)``.  ``cams``: the views (the reference's ``MiniCam``s or
        ``lara_amd.cameras.Camera``s); None = the reference's ``uni_mesh_path(16, dataset_name, sample, fov)``, imported
        from LaRa's own ``tools`` package at call time.  Returns (vertices, triangles, vertex_colors) of the written mesh
        (the reference returns None).  ``simplify_voxel`` (a cell size) or ``simplify_target`` (a triangle budget), one of
        them at most: the cleaned mesh goes through ``lara_amd.meshsimplify`` (``simplify_vertex_clustering`` / ``simplify_to``
        with ``simplify_contraction``) before it is written, and ``last_simplify_info`` holds its ``info``; with both None
        nothing changes.  ``writer``: "host" (the default) writes through ``write_obj``; "device" through
        ``lara_amd.meshio.write_mesh``, which builds the file's bytes on the device and takes the format from the path's extension
        (``.obj``: the same bytes; ``.ply``: binary PLY).  ``smooth_iterations`` (None: no smoothing): the cleaned mesh's vertices go
        through ``lara_amd.meshtopo`` before the simplification -- ``smooth_method`` "taubin" (``smooth_lambda``, ``smooth_mu``) or
        "laplacian" (``smooth_lambda``) -- and ``last_smooth_info`` says what ran; triangles and colours stay.  ``normals=True``
        (``writer="device"`` and a ``.ply`` path only) writes ``meshtopo.vertex_normals`` of the final mesh with it.  With the
        defaults nothing changes and ``lara_amd.meshtopo`` is not imported.  ``texture_patch`` (a patch size) or ``texture_max_texels``
        (a texel budget), one of them at most, a ``.obj`` path, the host writer and at most 64 views only: the views' float images and cameras are kept, the final mesh
        -- after smoothing and simplification -- is baked from them by ``lara_amd.meshtexture.bake`` (``texture_blend``, the vertex
        colours as the fallback) and written by ``write_textured_obj`` with its ``.mtl`` and ``.png``; ``last_texture`` holds the
        ``Texture``.  With both None ``lara_amd.meshtexture`` is not imported and the written bytes are what they were."""
        from .batch import build_rays, fov_to_ixt
        from .renderer import Renderer
        from .tsdf import TSDFVolume
        if simplify_voxel is not None and simplify_target is not None:
            raise ValueError("lara_amd.mesh.MeshExtractor: give simplify_voxel or simplify_target, not both")
        if writer not in ("host", "device"):
            raise ValueError('lara_amd.mesh.MeshExtractor: writer is "host" or "device"')
        if smooth_iterations is not None:
            if smooth_method not in ("taubin", "laplacian"):
                raise ValueError('lara_amd.mesh.MeshExtractor: smooth_method is "taubin" or "laplacian"')
            if int(smooth_iterations) < 0 or not all(math.isfinite(float(x)) for x in (smooth_lambda, smooth_mu)):
                raise ValueError("lara_amd.mesh.MeshExtractor: smooth_iterations must be >= 0, smooth_lambda and smooth_mu finite")
        if normals:
            if writer != "device":
                raise ValueError('lara_amd.mesh.MeshExtractor: normals=True needs writer="device" (the OBJ text of the host writer takes none)')
            if not str(save_mesh_path).lower().endswith(".ply"):
                raise ValueError("lara_amd.mesh.MeshExtractor: normals=True needs a .ply path (OBJ output takes no normals)")
        textured = texture_patch is not None or texture_max_texels is not None
        if textured:
            if texture_patch is not None and texture_max_texels is not None:
                raise ValueError("lara_amd.mesh.MeshExtractor: give texture_patch or texture_max_texels, not both")
            if not str(save_mesh_path).lower().endswith(".obj"):
                raise ValueError("lara_amd.mesh.MeshExtractor: a textured mesh needs a .obj path")
            if texture_blend not in ("weighted", "best"):
                raise ValueError('lara_amd.mesh.MeshExtractor: texture_blend is "weighted" or "best"')
            if texture_patch is not None and int(texture_patch) < 3:
                raise ValueError("lara_amd.mesh.MeshExtractor: texture_patch must be >= 3")
            if normals or writer != "host":
                raise ValueError('lara_amd.mesh.MeshExtractor: a textured mesh is written by the host writer (writer="host", no normals)')
        if cams is None:
            from tools.gen_video_path import uni_mesh_path          # LaRa's module (the reference's camera path)
            cams = uni_mesh_path(16, dataset_name, sample, fov)
        cams = list(cams)
        if textured and len(cams) > 64:
            raise ValueError("lara_amd.mesh.MeshExtractor: a texture is baked from at most 64 views")
        _centers, _shs, _opacity, _scaling, _rotation, mask = self.gs_params
        opacity, scaling, rotation = _opacity[mask], _scaling[mask], _rotation[mask]     # meshExtractor.py:85
        if self.aabb is not None:                                                        # meshExtractor.py:54-58
            center = self.aabb.mean(0)
            radius = np.linalg.norm(self.aabb[1] - self.aabb[0]) * 0.5
            voxel_size = radius / 256
            sdf_trunc = voxel_size * 2
            lo, hi = self.aabb[0] - voxel_size, self.aabb[1] + voxel_size
        else:
            lo, hi = self._gaussian_extent(cams, _centers, scaling, voxel_size, sdf_trunc)
        origin, res = self._grid(lo, hi, voxel_size, self.grid_pad_blocks)
        self.last_grid = (origin, voxel_size, res)
        vol = TSDFVolume(origin, voxel_size, sdf_trunc, res, device=device)
        self._mark("start")
        kept = []                     # (image [n,H,W,3], ixt [n,3,3], c2w [n,4,4]) of every chunk, for the texture
        for o in range(0, len(cams), chunk):
            part = cams[o:o + chunk]
            for cam in part:
                if hasattr(cam, "to_device"):
                    cam.to_device(device)
            # rays as tools/camera.py:54-57 builds them (one call for the chunk)
            c2w = torch.stack([_cam_c2w(cam) for cam in part]).to(device)
            ixt = torch.stack([fov_to_ixt(torch.tensor((cam.FoVx, cam.FoVy)), (cam.image_width, cam.image_height)) for cam in part])
            H, W = int(part[0].image_height), int(part[0].image_width)
            if any((int(c.image_height), int(c.image_width)) != (H, W) for c in part):
                raise RuntimeError("lara_amd.mesh.MeshExtractor: the views of a chunk must share one image size")
            rays = build_rays(c2w, ixt.to(device), H, W)
            if isinstance(self.render, Renderer):
                pkgs = self.render.render_views(part, rays, _centers, _shs, opacity, scaling, rotation, device)
            else:
                pkgs = [self.render.render_img(cam, rays[i], _centers, _shs, opacity, scaling, rotation, device)
                        for i, cam in enumerate(part)]
            self._mark("render")
            # each view as TSDFVolume.integrate_render prepares it (meshExtractor.py:89-108), the chunk in one call
            depth = torch.stack([p["depth"].reshape(H, W) for p in pkgs])
            acc = torch.stack([p["acc_map"].reshape(H, W) for p in pkgs])
            depth = torch.where(acc < alpha_thres, torch.zeros_like(depth), depth)
            color = (torch.stack([p["image"].reshape(H, W, 3) for p in pkgs]) * 255).to(torch.uint8).float()
            if textured:
                kept.append((torch.stack([p["image"].reshape(H, W, 3) for p in pkgs]).float(), ixt.float().cpu(), c2w.float().cpu()))
            K = torch.tensor([_intrinsics(cam) for cam in part])
            E = torch.stack([cam.world_view_transform.T for cam in part]).reshape(-1, 4, 4)
            if self.aabb is not None:                                                    # meshExtractor.py:95-97
                dtr = [float(np.linalg.norm(torch.as_tensor(cam.camera_center).detach().cpu().numpy() - center, axis=-1) + radius)
                       for cam in part]
            else:
                dtr = [float(depth_trunc)] * len(part)
            vol.integrate(depth, color, K, E, torch.tensor(dtr))
            self._mark("fuse")
        verts, tris, cols = vol.extract_triangle_mesh()
        self._mark("marching cubes")
        v, t, c, info = clean_mesh(verts, tris, cols, aabb=self.aabb_cfg, keep=10)
        self._mark("clean_mesh")
        self.last_info = info
        self.raw_mesh = (verts, tris, cols)
        self.last_smooth_info = None
        if smooth_iterations is not None:
            from . import meshtopo
            topo = meshtopo.MeshTopology(v, t)
            if smooth_method == "taubin":
                v = topo.smooth_taubin(smooth_iterations, smooth_lambda, smooth_mu)
            else:
                v = topo.smooth_laplacian(smooth_iterations, smooth_lambda)
            self.last_smooth_info = {"method": smooth_method, "iterations": int(smooth_iterations), "lambda": float(smooth_lambda),
                                     "mu": float(smooth_mu) if smooth_method == "taubin" else None, "n_edges": topo.n_edges}
            self._mark("smooth")
        self.last_simplify_info = None
        if simplify_voxel is not None or simplify_target is not None:
            from . import meshsimplify
            if simplify_voxel is not None:
                v, t, c, sinfo = meshsimplify.simplify_vertex_clustering(v, t, c, simplify_voxel, simplify_contraction)
            else:
                v, t, c, sinfo = meshsimplify.simplify_to(v, t, c, simplify_target, simplify_contraction)
            self.last_simplify_info = sinfo
            self._mark("simplify")
        self.last_texture = None
        if textured:
            from . import meshtexture
            if len({tuple(k[0].shape[1:]) for k in kept}) != 1:
                raise RuntimeError("lara_amd.mesh.MeshExtractor: a textured mesh needs views of one image size")
            self.last_texture = meshtexture.bake(v, t, torch.cat([k[0] for k in kept]), torch.cat([k[1] for k in kept]),
                                                 torch.cat([k[2] for k in kept]), patch=texture_patch, max_texels=texture_max_texels,
                                                 vertex_colors=c, blend=texture_blend)
            self._mark("texture")
            meshtexture.write_textured_obj(save_mesh_path, v, t, self.last_texture)
            self._mark("write_obj")
            return v, t, c
        if writer == "device":
            from . import meshio
            if normals:
                from . import meshtopo
                meshio.write_mesh(save_mesh_path, v, t, c, meshtopo.vertex_normals(v, t))
            else:
                meshio.write_mesh(save_mesh_path, v, t, c)
        else:
            write_obj(save_mesh_path, v, t, c)
        self._mark("write_obj")
        return v, t, c
