"""Times `lara_amd.meshsimplify.simplify_vertex_clustering` on one MI355X with HIP events after warm-up, on a mesh built here: the UV
sphere of tools/meshmetrics_bench.py (about 557 k triangles of about one TSDF voxel each, the size of bench.py's mesh_eval mesh;
radius 1, so the extractor's default voxel of 2 / 256 puts 256 voxels across it), with per-vertex colours.  h = 2, 4 and 8 voxels,
both contractions.

Per h and contraction: the whole call (`ms`; it includes its three host reads) and the stages between the events the call records
(cells and clusters / triangles / bucket and sums / solve / compaction); the algorithmic bytes (every input and output once) over the
whole call as a fraction of the device's copy rate, measured here on a 1 GiB buffer; the sizes; `surface_scores(simplified, original)`
(Chamfer, F-score at 0.005 / 0.01 / 0.02); `write_obj` wall time of the original and of the simplified mesh.

There is no baseline: nothing simplified a mesh before.  As CONTEXT only: `clean_mesh` on the same mesh (the stage in front), and
the numpy restatement (tests/meshsimplify_restate.py) of one configuration on the host, once.  Nothing is read from outside the repository.
    python tools/meshsimplify_bench.py [--steps 20] [--warmup 3] [--quick] [--out profiles/meshsimplify_bench.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.meshmetrics_bench import sphere_pair, timed  # noqa: E402

STAGES = ("cells and clusters", "triangles", "bucket and sums", "solve", "compaction")


def copy_rate(dev, nbytes=1 << 30, steps=10):
    """bytes read + written per second of a device-to-device copy."""
    a = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    b = torch.empty_like(a)
    return 2.0 * nbytes / (timed(lambda: b.copy_(a), steps, 2) * 1e-3)


def wall(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="a small sphere, one step (the test suite's run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("meshsimplify_bench: needs an MI355X")
    from lara_amd import mesh, meshmetrics, meshsimplify
    dev = torch.device("cuda:0")
    n_lat, n_lon = (64, 128) if a.quick else (374, 746)
    steps, warmup = (1, 1) if a.quick else (a.steps, a.warmup)
    voxel = 2.0 / 256 * (374 / n_lat)
    V, F, _ = sphere_pair(n_lat, n_lon, dev)
    C = (0.5 * V + 0.5).contiguous()
    Nv, T = int(V.shape[0]), int(F.shape[0])
    rate = copy_rate(dev, (1 << 26) if a.quick else (1 << 30))
    res = {"Nv": Nv, "T": T, "voxel": voxel, "steps": steps, "warmup": warmup, "copy_rate_GBps": rate / 1e9, "runs": []}
    tmp = tempfile.mkdtemp()
    res["write_obj_original_ms"] = wall(lambda: mesh.write_obj(os.path.join(tmp, "original.obj"), V, F, C))
    res["original_obj_MB"] = os.path.getsize(os.path.join(tmp, "original.obj")) / 1e6
    res["context_clean_mesh_ms"] = timed(lambda: mesh.clean_mesh(V, F, C), steps, warmup)
    for mult in (2, 4, 8):
        h = mult * voxel
        for mode in ("quadric", "average"):
            run = lambda marks=None: meshsimplify.simplify_vertex_clustering(V, F, C, h, mode, _marks=marks)
            V2, F2, C2, info = run()
            row = {"h_voxels": mult, "h": h, "contraction": mode, "vertices": int(V2.shape[0]), "triangles": int(F2.shape[0]),
                   "n_cells": info["n_cells"], "n_clamped": info["n_clamped"]}
            row["ms"] = timed(run, steps, warmup)
            acc = dict.fromkeys(STAGES, 0.0)
            for _ in range(steps):
                marks = []
                run(marks)
                torch.cuda.synchronize()
                for (_, e0), (name, e1) in zip(marks[:-1], marks[1:]):
                    acc[name] += e0.elapsed_time(e1) / steps
            row["stage_ms"] = acc
            nbytes = Nv * (12 + 12 + 4) + T * 12 + int(V2.shape[0]) * 24 + int(F2.shape[0]) * 24
            row["algorithmic_MB"] = nbytes / 1e6
            row["fraction_of_copy_rate"] = nbytes / (row["ms"] * 1e-3) / rate
            s = meshmetrics.surface_scores((V2, F2), (V, F), n=20000 if a.quick else 200000)
            row["chamfer"], row["fscore"], row["thresholds"] = s["chamfer"], s["fscore"], s["thresholds"]
            path = os.path.join(tmp, "simplified.obj")
            row["write_obj_ms"] = wall(lambda: mesh.write_obj(path, V2, F2, C2))
            row["obj_MB"] = os.path.getsize(path) / 1e6
            res["runs"].append(row)
    # context: the numpy restatement on the host, one configuration, once
    from tests import meshsimplify_restate as R
    Vn, Fn = V.cpu().numpy(), F.cpu().numpy()
    res["context_numpy_restatement_ms"] = wall(lambda: R.simplify(Vn, Fn, None, 4 * voxel, "quadric", check_exact=False))
    res["context_numpy_restatement_config"] = "h = 4 voxels, quadric, no colours"

    def rounded(x):
        if isinstance(x, float):
            return round(x, 6)
        if isinstance(x, dict):
            return {k: rounded(v) for k, v in x.items()}
        if isinstance(x, list):
            return [rounded(v) for v in x]
        return x
    line = json.dumps(rounded(res))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
