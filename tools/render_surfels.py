"""Renders a 2DGS ``point_cloud.ply`` -- one `lara_amd.splatio.write_ply` wrote, or one trained by the 2DGS code base -- or a packed
cloud of `lara_amd.splatpack` (a compressed PLY, a ``.splat`` file; the input is loaded through `splatpack.read`) on one
MI355X without running any network: the orbit of `evaluate.video_cameras`, ``Renderer.render_views`` in chunks of 8
(`evaluate.render_turntable`), RGB and normal frames as PNG (`meshtexture.write_png`), and a small JSON with the surfel count,
the SH degree, the frame count and wall times (one run each: no spread is measured).  ``--mesh`` also extracts the TSDF mesh from
the loaded surfels (`MeshExtractor.extract` on ``cloud.gs_params()`` with `evaluate.mesh_cameras`).  ``--quick``: 2 frames of
32 x 32 (what tests/test_splatio_gpu.py runs).  ``--transform FILE`` (16 numbers, ``.npy`` or text: a 4x4 similarity) moves the
loaded cloud by `lara_amd.splatxform.transform` before anything is rendered; the cameras stay where they are.
    python tools/render_surfels.py scene.ply --dataset gobjeverse --frames 24 --size 512 --out DIR [--mesh out.obj] [--quick]
                                   [--transform T.npy]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHUNK = 8


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("ply")
    ap.add_argument("--dataset", default="gobjeverse", help="the camera path's family (evaluate.video_cameras)")
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out", required=True, help="directory for rgb_####.png, normal_####.png and render_surfels.json")
    ap.add_argument("--mesh", default=None, help="also extract the TSDF mesh to this .obj path")
    ap.add_argument("--quick", action="store_true", help="2 frames of 32 x 32")
    ap.add_argument("--transform", default=None, help="a 4x4 similarity (16 numbers, .npy or text) applied to the cloud first")
    args = ap.parse_args()
    if args.quick:
        args.frames, args.size = 2, 32
    if not torch.cuda.is_available():
        sys.exit("tools/render_surfels.py needs an MI355X")

    from lara_amd import evaluate, meshtexture, splatpack
    from lara_amd.renderer import Renderer

    dev = torch.device("cuda", 0)
    wall = {}
    t0 = time.perf_counter()
    cloud, info = splatpack.read(args.ply, device=dev)           # (a plain point_cloud.ply goes to splatio.read_ply as before)
    torch.cuda.synchronize()
    wall["read_ply_s"] = time.perf_counter() - t0
    T = None
    if args.transform:
        import numpy as np
        from lara_amd import splatxform
        T = np.load(args.transform) if args.transform.endswith(".npy") else np.loadtxt(args.transform)
        if T.size != 16:
            sys.exit(f"tools/render_surfels.py: {args.transform} holds {T.size} numbers, a 4x4 has 16")
        T = np.asarray(T, np.float64).reshape(4, 4)
        cloud = splatxform.transform(cloud, T, out=cloud)

    renderer = Renderer(sh_degree=cloud.sh_degree, white_background=True)
    cams = evaluate.video_cameras(args.frames, args.dataset, (args.size, args.size), device=dev)
    t0 = time.perf_counter()
    frames, normals = evaluate.render_turntable(renderer, cloud.render_args(), cams, chunk=CHUNK)
    frames, normals = frames.cpu(), normals.cpu()                      # (waits for the stream)
    wall["render_s"] = time.perf_counter() - t0

    os.makedirs(args.out, exist_ok=True)
    t0 = time.perf_counter()
    alpha = torch.full(tuple(frames.shape[:3]) + (1,), 255, dtype=torch.uint8)
    for name, maps in (("rgb", frames), ("normal", normals)):
        rgba = torch.cat([maps, alpha], dim=-1)
        for i in range(rgba.shape[0]):
            meshtexture.write_png(os.path.join(args.out, f"{name}_{i:04d}.png"), rgba[i])
    wall["write_png_s"] = time.perf_counter() - t0

    res = {"ply": os.path.abspath(args.ply), "n_surfels": cloud.n_surfels, "sh_degree": cloud.sh_degree, "frames": len(cams),
           "size": args.size, "dataset": args.dataset, "chunk": CHUNK, "dropped_third_scale": info["dropped_third_scale"],
           "skipped_properties": info.get("skipped_properties", []), "mesh": None}
    if args.mesh:
        from lara_amd.mesh import MeshExtractor
        t0 = time.perf_counter()
        mcams = evaluate.mesh_cameras(16, args.dataset, (args.size, args.size), device=dev)
        v, t, _ = MeshExtractor(cloud.gs_params(), renderer, None).extract(args.mesh, args.dataset, cams=mcams, chunk=CHUNK,
                                                                          device=dev)
        torch.cuda.synchronize()
        wall["mesh_s"] = time.perf_counter() - t0
        res["mesh"] = {"path": os.path.abspath(args.mesh), "views": len(mcams), "vertices": int(v.shape[0]), "triangles": int(t.shape[0])}
    if T is not None:
        res["transform"] = T.tolist()
    res["wall_s"] = wall
    with open(os.path.join(args.out, "render_surfels.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
