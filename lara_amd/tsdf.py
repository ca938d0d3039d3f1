"""TSDF fusion of rendered views and mesh extraction on the GPU: the
`volume.integrate(...)` loop and `volume.extract_triangle_mesh()` of the reference's ``MeshExtractor.extract``
(tools/meshExtractor.py:67-110) without leaving the device -- the reference copies depth, alpha and colour of every one
of its 48 views to the host and feeds Open3D's CPU ``ScalableTSDFVolume``.  Open3D's voxel conventions, per-voxel update
and block semantics (include/lara_tsdf.h): by default a view is integrated only into the 16^3-voxel blocks within
sdf_trunc of its back-projected depth samples, as ``ScalableTSDFVolume`` does (``block_sparse=False``: every voxel, as
``UniformTSDFVolume``).  ``extract_triangle_mesh()`` runs marching cubes on the device and returns welded vertices,
triangles and vertex colours; the post-processing (crop, cluster filter, meshExtractor.py:112-135) and the writer are
``lara_amd.mesh.clean_mesh`` / ``write_obj`` on the device, ``to_open3d_mesh()`` still hands the mesh to Open3D where it is
installed.  No CPU path."""
from __future__ import annotations

import math

import torch

from ._native import call, host_array, require_device


class TSDFVolume:
    """``TSDFVolume(origin, voxel_length, sdf_trunc, resolution)``: voxel (i,j,k) is centred at
    origin + voxel_length * (i + 0.5, j + 0.5, k + 0.5); `MeshExtractor.extract` uses voxel_length = radius / 256 and
    sdf_trunc = 2 voxels around the object's bounding box (tools/meshExtractor.py:54-58)."""

    BLOCK = 16      # voxels per block edge (ScalableTSDFVolume's volume_unit_resolution)

    def __init__(self, origin, voxel_length: float, sdf_trunc: float, resolution: int, device="cuda", block_sparse=True,
                 depth_sampling_stride=4):
        self.origin = tuple(float(o) for o in origin)
        self.voxel_length, self.sdf_trunc, self.res = float(voxel_length), float(sdf_trunc), int(resolution)
        self.block_sparse, self.stride = bool(block_sparse), int(depth_sampling_stride)
        if self.block_sparse and self.res % self.BLOCK:
            raise RuntimeError("block-sparse volumes need a resolution that is a multiple of 16")
        dev = torch.device(device)
        require_device(dev)
        n = self.res ** 3
        self.tsdf = torch.zeros(n, dtype=torch.float32, device=dev)
        self.weight = torch.zeros(n, dtype=torch.float32, device=dev)
        self.rgb = torch.zeros(n, 3, dtype=torch.float32, device=dev)
        nb = self.res // self.BLOCK
        self.allocated = torch.zeros(nb ** 3 if self.block_sparse else 0, dtype=torch.uint8, device=dev)   # blocks ever touched

    @torch.no_grad()
    def integrate(self, depth, color, intrinsics, extrinsics, depth_trunc):
        """depth [V,H,W] (0 = no measurement), color [V,H,W,3] in 0..255, intrinsics [V,4] = (fx, fy, cx, cy),
        extrinsics [V,4,4] world->camera, depth_trunc [V] or a float.  Views are folded in the given order."""
        dev = self.tsdf.device
        f = lambda t: torch.as_tensor(t, dtype=torch.float32, device=dev).contiguous()
        depth, color, intrinsics, extrinsics = f(depth), f(color), f(intrinsics), f(extrinsics)
        V, H, W = depth.shape
        if color.shape != (V, H, W, 3) or intrinsics.shape != (V, 4) or extrinsics.shape != (V, 4, 4):
            raise RuntimeError("expected depth [V,H,W], color [V,H,W,3], intrinsics [V,4], extrinsics [V,4,4]")
        depth_trunc = f(depth_trunc).expand(V).contiguous() if torch.as_tensor(depth_trunc).dim() == 0 else f(depth_trunc)
        origin = host_array("f", self.origin)
        if V > 64:          # (the kernels keep a view mask in 64 bits)
            for o in range(0, V, 64):
                self.integrate(depth[o:o + 64], color[o:o + 64], intrinsics[o:o + 64], extrinsics[o:o + 64], depth_trunc[o:o + 64])
            return
        if self.block_sparse:
            c2w = torch.linalg.inv_ex(extrinsics.double())[0].float().contiguous()
            touched = torch.empty(V * self.allocated.numel(), dtype=torch.uint8, device=dev)
            call("lara_tsdf_integrate_blocks", dev, self.res, origin, self.voxel_length, self.sdf_trunc, V, H, W, self.stride, depth,
                 color, intrinsics, extrinsics, c2w, depth_trunc, self.tsdf, self.weight, self.rgb, touched, self.allocated)
            self.last_touched = touched.view(V, -1)
            return
        call("lara_tsdf_integrate", dev, self.res, origin, self.voxel_length, self.sdf_trunc, V, H, W, depth, color, intrinsics,
             extrinsics, depth_trunc, self.tsdf, self.weight, self.rgb)

    def integrate_render(self, cam, render_pkg, alpha_thres=0.08, depth_trunc=10.0):
        """One rendered view as `MeshExtractor.extract` prepares it (meshExtractor.py:76-108): pinhole intrinsics from
        the camera's field of view, depth zeroed where acc_map < alpha_thres, colour quantised to 8 bits."""
        H, W = int(cam.image_height), int(cam.image_width)
        K = torch.tensor([[W / (2 * math.tan(cam.FoVx / 2.0)), H / (2 * math.tan(cam.FoVy / 2.0)), W / 2, H / 2]])
        depth = render_pkg["depth"].detach().reshape(1, H, W)
        depth = torch.where(render_pkg["acc_map"].detach().reshape(1, H, W) < alpha_thres, torch.zeros_like(depth), depth)
        color = (render_pkg["image"].detach().reshape(1, H, W, 3) * 255).to(torch.uint8).float()
        self.integrate(depth, color, K, cam.world_view_transform.T.reshape(1, 4, 4), depth_trunc)

    def volume(self):
        """(tsdf [R,R,R], weight [R,R,R], rgb [R,R,R,3]) indexed [x][y][z]."""
        r = self.res
        return self.tsdf.view(r, r, r), self.weight.view(r, r, r), self.rgb.view(r, r, r, 3)

    @torch.no_grad()
    def extract_triangle_mesh(self, weld=True):
        """`volume.extract_triangle_mesh()` (meshExtractor.py:110) on the device: (vertices [Nv,3], triangles [T,3] int64,
        vertex_colors [Nv,3] in 0..1).  ``weld=False``: three private vertices per triangle."""
        dev, r = self.tsdf.device, self.res
        if r % self.BLOCK:
            raise RuntimeError("mesh extraction needs a resolution that is a multiple of 16")
        origin = host_array("f", self.origin)
        alloc = self.allocated if self.block_sparse else None
        counts = torch.zeros(r ** 3, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            call("lara_tsdf_mesh_count", dev, r, origin, self.voxel_length, self.tsdf, self.weight, self.rgb, alloc, counts)
            ends = torch.cumsum(counts, 0, dtype=torch.int64)
            T = int(ends[-1])                    # the one host read: the output's size
            verts = torch.empty(T, 3, 3, dtype=torch.float32, device=dev)
            cols = torch.empty(T, 3, 3, dtype=torch.float32, device=dev)
            keys = torch.empty(T, 3, dtype=torch.int64, device=dev)
            if T:
                call("lara_tsdf_mesh_emit", dev, r, origin, self.voxel_length, self.tsdf, self.weight, self.rgb, alloc, counts, ends,
                     verts, cols, keys)
        if not weld:
            return verts.view(-1, 3), torch.arange(3 * T, device=dev).view(T, 3), cols.view(-1, 3)
        uniq, inverse = torch.unique(keys.view(-1), return_inverse=True)
        first = torch.full((uniq.numel(),), 3 * T, dtype=torch.int64, device=dev).scatter_reduce_(
            0, inverse, torch.arange(3 * T, device=dev), reduce="amin", include_self=True)
        return verts.view(-1, 3)[first], inverse.view(T, 3), cols.view(-1, 3)[first]

    def to_open3d_mesh(self):
        """The extracted mesh as an `open3d.geometry.TriangleMesh`, for the reference's own post-processing and writer
        (meshExtractor.py:112-135).  Needs Open3D (absent from this image; the reference needs it too)."""
        try:
            import open3d as o3d
        except ImportError as e:   # pragma: no cover
            raise RuntimeError("lara_amd.tsdf.TSDFVolume.to_open3d_mesh needs open3d") from e
        v, t, c = (x.cpu().numpy() for x in self.extract_triangle_mesh())
        mesh = o3d.geometry.TriangleMesh(o3d.utility.Vector3dVector(v.astype("float64")), o3d.utility.Vector3iVector(t.astype("int32")))
        mesh.vertex_colors = o3d.utility.Vector3dVector(c.astype("float64"))
        return mesh
