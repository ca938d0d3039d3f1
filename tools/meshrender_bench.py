"""Times `lara_amd.meshrender` on one MI355X with HIP events after warm-up: the mesh bench.py's mesh_eval leg extracts
(tools/mesh_bench.py: mesh_eval_mesh, ~0.5 M triangles) as a 120-frame turntable at 512^2 in chunks of 8.

Per-stage times come from calls that stop early, as differences: no triangles (fill + stage V), no pixel outputs (+ stage R),
every output (+ stage S).  Algorithmic bytes per frame: 12 Nv + 12 T read; per pixel 8 (key written) + 8 (key read) + 4
(face_id) + 4 (depth) + 12 (normal) + 3 (frame) written.  The fraction of the HBM rate is those bytes over the event time
against the 6.29 TB/s a float4 copy reaches.  Nothing in the package rendered a mesh before; the only neighbour is
`evaluate.render_turntable` of a surfel scene for the same cameras, reported beside it as context, not as a ratio.
    python tools/meshrender_bench.py [--steps 5] [--warmup 2] [--frames 120] [--out profiles/meshrender_bench.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_GBPS = 6290.0


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("meshrender_bench: needs an MI355X")
    from lara_amd import evaluate, meshrender, synthetic
    from lara_amd.renderer import Renderer
    from tools.mesh_bench import mesh_eval_mesh
    dev = torch.device("cuda:0")
    S, N = a.size, a.frames
    v, t, c = mesh_eval_mesh(dev)
    cams = evaluate.video_cameras(N, "gobjeverse", (S, S), device=dev)
    none = t[:0]
    every = ("face_id", "depth", "normal", "frames", "info")
    run = lambda tris, outputs, **kw: meshrender.render_mesh_views(cams, v, tris, c, chunk=8, outputs=outputs, check=False, **kw)
    info = run(t, ("info",))["info"].sum(0).tolist()
    res = {"frames": N, "size": S, "chunk": 8, "Nv": int(v.shape[0]), "T": int(t.shape[0]), "info_sum": info}
    res["fill_snap_ms"] = timed(lambda: run(none, ("info",)), a.steps, a.warmup)
    through_r = timed(lambda: run(t, ("info",)), a.steps, a.warmup)
    res["stage_r_ms"] = through_r - res["fill_snap_ms"]
    res["all_outputs_ms"] = timed(lambda: run(t, every), a.steps, a.warmup)
    res["stage_s_ms"] = res["all_outputs_ms"] - through_r
    res["frames_only_ms"] = timed(lambda: run(t, ("frames",)), a.steps, a.warmup)
    res["stage_r_all_threads_ms"] = timed(lambda: run(t, ("info",), wave_box_area=1 << 30), a.steps, a.warmup) - res["fill_snap_ms"]
    res["stage_r_threshold_16_ms"] = timed(lambda: run(t, ("info",), wave_box_area=16), a.steps, a.warmup) - res["fill_snap_ms"]
    per_frame = 12.0 * res["Nv"] + 12.0 * res["T"] + S * S * (8 + 8 + 4 + 4 + 12 + 3)
    res["algorithmic_bytes_per_frame"] = per_frame
    res["all_outputs_GBps"] = per_frame * N / (res["all_outputs_ms"] * 1e-3) / 1e9
    res["fraction_of_hbm_copy_rate"] = res["all_outputs_GBps"] / HBM_COPY_GBPS
    res["ms_per_frame_all_outputs"] = res["all_outputs_ms"] / N
    # context: the surfel turntable of eval_bench's scene for the same cameras
    sc = synthetic.make_scene(grid=64, K=2, regime="trained", seed=0, device=dev)
    gs = (sc["centers"], sc["shs"], sc["opacity"], sc["scales"], sc["rotations"])
    renderer = Renderer(sh_degree=1, white_background=True)
    res["surfel_turntable_ms_context"] = timed(lambda: evaluate.render_turntable(renderer, gs, cams, chunk=8), max(2, a.steps // 2), 1)
    line = json.dumps({k: (round(x, 4) if isinstance(x, float) else x) for k, x in res.items()})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
