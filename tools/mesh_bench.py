"""Times LaRa's mesh path (tools/meshExtractor.py:51-135) on bench.py's mesh_eval object (trained-like scene, seed 123):
  extract:  lara_amd.mesh.MeshExtractor.extract with the default aabb (configs/infer.yaml) over 48 views @1024^2 (16 per
            elevation at 0, -30, +30 degrees): render, fuse, marching cubes, clean_mesh and write_obj (HIP events around
            the device parts, the host clock around the writer), triangles / clusters / vertices before and after;
  557k:     the mesh of bench.py's mesh_eval leg (256^3 volume over [-1, 1]): clean_mesh on the device against the numpy
            restatement (tests/meshclean_restate.py, scipy's connected components; the Open3D-style BFS with --bfs).
Open3D's own time is not measured (Open3D is absent).  Prints one JSON line.  Needs an MI355X.
    python tools/mesh_bench.py [--repeats 3] [--bfs]"""
import argparse
import json
import math
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

AABB = [-0.5, -0.5, -0.5, 0.5, 0.5, 0.5]        # configs/infer.yaml:52


def mesh_eval_scene(device="cuda"):
    from lara_amd import synthetic
    return synthetic.make_scene(grid=64, K=2, regime="trained", seed=123, device=device)


def mesh_eval_mesh(device="cuda"):
    """bench.py's mesh_eval object (48 turntable views @1024, 256^3 volume over [-1, 1], trunc 0.08, alpha 0.08) fused and
    extracted the way its leg does it: (vertices, triangles, colours) of ~557 k triangles."""
    from lara_amd import GaussianRasterizationSettings, cameras, rasterize_gaussians_views
    from lara_amd.tsdf import TSDFVolume
    dev = torch.device(device)
    res, n_views, chunk, grid = 1024, 48, 8, 256
    sc = mesh_eval_scene(dev)
    cams = cameras.make_cameras(cameras.turntable_c2w(n_views), res, res, 0.75, 0.75, 1.906 - 0.8, 1.906 + 0.8, device=dev)
    settings = [GaussianRasterizationSettings(
        image_height=res, image_width=res, tanfovx=math.tan(c.FoVx * 0.5), tanfovy=math.tan(c.FoVy * 0.5),
        bg=torch.ones(3, device=dev), scale_modifier=1.0, viewmatrix=c.world_view_transform.contiguous(),
        projmatrix=c.full_proj_transform.contiguous(), sh_degree=1, campos=c.camera_center.contiguous(), prefiltered=False,
        debug=False) for c in cams]
    K = torch.tensor([[res / (2 * math.tan(c.FoVx / 2.0)), res / (2 * math.tan(c.FoVy / 2.0)), res / 2, res / 2] for c in cams],
                     device=dev)
    ext = torch.stack([c.world_view_transform.T for c in cams]).contiguous()
    vol = TSDFVolume((-1.0, -1.0, -1.0), 2.0 / grid, 0.08, grid, device=dev)
    with torch.no_grad():
        opac, scales = torch.sigmoid(sc["opacity"]), torch.exp(sc["scales"])
        rots = torch.nn.functional.normalize(sc["rotations"])
        for i in range(0, n_views, chunk):
            color, _, allmap = rasterize_gaussians_views(settings[i:i + chunk], sc["centers"], None, opac, shs=sc["shs"],
                                                         scales=scales, rotations=rots)
            acc = allmap[:, 1]
            depth = torch.where(acc < 0.08, torch.zeros_like(acc), allmap[:, 0] / acc.clamp_min(1e-8))
            rgb8 = (color.clamp(0, 1).permute(0, 2, 3, 1) * 255).to(torch.uint8).float()
            vol.integrate(depth, rgb8, K[i:i + chunk], ext[i:i + chunk], 10.0)
    return vol.extract_triangle_mesh()


def turntable_cams(res=1024, device="cuda"):
    """uni_mesh_path(16, ...)'s layout (tools/gen_video_path.py:117-129): 16 views at each of 0, -30 and +30 degrees."""
    from lara_amd import cameras
    c2w = torch.cat([cameras.turntable_c2w(16, e) for e in (0.0, -30.0, 30.0)])
    return cameras.make_cameras(c2w, res, res, 0.75, 0.75, 1.906 - 0.8, 1.906 + 0.8, device=device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--bfs", action="store_true", help="also time the Open3D-style BFS restatement (slow)")
    args = ap.parse_args()
    from lara_amd.mesh import MeshExtractor, clean_mesh
    from lara_amd.renderer import Renderer
    from tests import meshclean_restate as R
    out = {}
    sc = mesh_eval_scene()
    mask = torch.sigmoid(sc["opacity"][:, 0]) > 0.005
    params = (sc["centers"][mask], sc["shs"][mask], sc["opacity"], sc["scales"], sc["rotations"], mask)
    cams = turntable_cams()
    render = Renderer(sh_degree=1, white_background=True)
    with tempfile.TemporaryDirectory() as d:
        runs = []
        for rep in range(args.repeats + 1):
            ex = MeshExtractor(params, render, AABB)
            ex.timings = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            v, t, c = ex.extract(os.path.join(d, "mesh.obj"), None, cams=cams)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            ev = ex.timings
            stages = {}
            for (_, a), (name, b) in zip(ev[:-1], ev[1:]):
                if name != "write_obj":
                    stages[name] = stages.get(name, 0.0) + a.elapsed_time(b)
            runs.append((wall, stages))
            if rep == 0:
                rv, rt, rc = ex.raw_mesh
                info = ex.last_info
        t_w = time.perf_counter()
        from lara_amd.mesh import write_obj
        write_obj(os.path.join(d, "again.obj"), v, t, c)
        t_write = time.perf_counter() - t_w
    walls = sorted(r[0] for r in runs[1:])
    med = runs[1:][[r[0] for r in runs[1:]].index(walls[len(walls) // 2])][1]
    out["extract"] = {"views": len(cams), "res": 1024, "aabb": AABB, "grid": list(ex.last_grid[1:]) + [list(ex.last_grid[0])],
                      "ms_per_object_wall": round(1e3 * walls[len(walls) // 2], 1),
                      "ms_device": {k: round(x, 2) for k, x in med.items()}, "write_obj_ms": round(1e3 * t_write, 1),
                      "triangles_before": int(rt.shape[0]), "vertices_before": int(rv.shape[0]),
                      "clusters": int(info["cluster_n_triangles"].numel()), "triangles_after": int(t.shape[0]),
                      "vertices_after": int(v.shape[0]), "union_rounds": info.get("union_rounds")}
    rv_np, rt_np = rv.cpu().numpy(), rt.cpu().numpy()
    t0 = time.perf_counter()
    R.clean_mesh(rv_np, rt_np, rc.cpu().numpy(), AABB, clusters=R.cluster_scipy)
    out["extract"]["clean_cpu_restatement_scipy_ms"] = round(1e3 * (time.perf_counter() - t0), 1)

    v5, t5, c5 = mesh_eval_mesh()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    clean_mesh(v5, t5, c5)
    torch.cuda.synchronize()
    times = []
    for _ in range(max(1, args.repeats)):
        t0 = time.perf_counter()
        a.record()
        res = clean_mesh(v5, t5, c5)
        b.record()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0, a.elapsed_time(b)))
    times.sort()
    info = res[3]
    o = {"triangles_before": int(t5.shape[0]), "vertices_before": int(v5.shape[0]), "clusters": int(info["cluster_n_triangles"].numel()),
         "triangles_after": int(res[1].shape[0]), "vertices_after": int(res[0].shape[0]), "union_rounds": info["union_rounds"],
         "clean_mesh_ms_wall": round(1e3 * times[len(times) // 2][0], 2), "clean_mesh_ms_events": round(times[len(times) // 2][1], 2)}
    vn, tn, cn = v5.cpu().numpy(), t5.cpu().numpy(), c5.cpu().numpy()
    t0 = time.perf_counter()
    R.clean_mesh(vn, tn, cn, clusters=R.cluster_scipy)
    o["clean_cpu_restatement_scipy_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
    if args.bfs:
        t0 = time.perf_counter()
        R.clean_mesh(vn, tn, cn)
        o["clean_cpu_restatement_bfs_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
    out["mesh_eval_557k"] = o
    out["note"] = "Open3D's clean-up time is not measured (Open3D is absent); the CPU numbers are the numpy restatement's"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
