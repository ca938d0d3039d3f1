"""Times `lara_amd.meshalign` on one MI355X with HIP events after warm-up.  The target is the sphere of tools/meshsimplify_bench.py
(about 557 k triangles) under the asymmetric warp of tests/meshalign_restate.py -- a plain sphere cannot pin a rotation, and the
plane solve refuses it --, the source 2 x 10^5 samples of it moved by a known 10 degree motion.

  * the stages of one iteration separately: transform, the triangle query (closest points; at the start, 10 degrees off, where
    many queries are farther from the surface than the rings reach and fall back to brute force, and at the end, on it),
    accumulate, and the host solve (host clock: it is numpy on 48 doubles); accumulate next to the device's copy rate measured in
    the same run (44 bytes a pair: source, target, face, distance, normal);
  * one whole `icp` call (plane mode), by HIP events and by the host clock -- the loop reads its row once per iteration, so the
    host clock is the honest figure --, its iterations and its error against the known motion;
  * as CONTEXT only: transform + the same sums in torch operators (float64) on the same correspondences.

Nothing aligned meshes here before: there is no baseline and no time ratio to meet.  Nothing is read from outside the repository.
    python tools/meshalign_bench.py [--steps 10] [--warmup 2] [--quick] [--out profiles/meshalign_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.meshmetrics_bench import sphere_pair, timed  # noqa: E402
from tools.meshsimplify_bench import copy_rate  # noqa: E402


def warp(V):
    """The warp of tests/meshalign_restate.py (float64 on the device, stored as fp32)."""
    P = V.double()
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    w = 1.0 + 0.25 * x + 0.15 * y * z + 0.1 * torch.sin(3.0 * z + 1.0) * x * y
    return (P * w.unsqueeze(1) * torch.tensor([1.0, 0.8, 0.6], dtype=torch.float64, device=V.device)).float().contiguous()


def torch_row(S, T, closest, normals, face, d, max_dist):
    """Transform + the sums of the reduction row with torch operators in float64 (no origin, every pair has a normal)."""
    A = torch.as_tensor(T[:3], dtype=torch.float64, device=S.device)
    p = (S.double() @ A[:, :3].T + A[:, 3]).float().double()
    keep = (d <= max_dist).double().unsqueeze(1)
    q, n = closest.double(), normals[face.long()].double()
    J = torch.cat([torch.linalg.cross(p, n), n], 1) * keep
    r = ((p - q) * n).sum(1, keepdim=True) * keep
    return torch.cat([keep.sum().reshape(1), ((p - q) ** 2 * keep).sum().reshape(1), (p * keep).sum(0), (q * keep).sum(0),
                      ((p * keep).T @ q).reshape(-1), (J.T @ J).reshape(-1), (J * r).sum(0), (r * r).sum().reshape(1)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="a small sphere, one step (the test suite's run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("meshalign_bench: needs an MI355X")
    from lara_amd import meshalign, meshdist, meshmetrics
    dev = torch.device("cuda:0")
    n_lat, n_lon = (64, 128) if a.quick else (374, 746)
    n = 20000 if a.quick else 200000
    steps, warmup = (1, 1) if a.quick else (a.steps, a.warmup)
    max_dist = 0.3
    V, F, _ = sphere_pair(n_lat, n_lon, dev)
    V = warp(V)
    axis = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    truth = np.eye(4)
    truth[:3, :3], truth[:3, 3] = meshalign.rodrigues(axis * np.deg2rad(10.0)), (0.04, -0.04, 0.04)
    S = meshalign.transform_points(meshmetrics.sample_surface(V, F, n, seed=0)[0], np.linalg.inv(truth))
    rate = copy_rate(dev, (1 << 26) if a.quick else (1 << 30))
    res = {"Nv": int(V.shape[0]), "T": int(F.shape[0]), "n": n, "steps": steps, "warmup": warmup, "max_dist": max_dist,
           "copy_rate_GBps": rate / 1e9, "one_run": True}

    grid = meshdist.TriangleGrid(V, F)
    normals = grid.face_normals
    buf = torch.empty_like(S)
    many = steps if a.quick else 100 * steps          # the short stages: a window of a tenth of a second, not of a millisecond
    res["short_stage_steps"] = many
    res["transform_ms"] = timed(lambda: meshalign.transform_points(S, np.eye(4), out=buf), many, warmup)
    res["query_ms"] = timed(lambda: grid.query(S, return_closest=True), steps, warmup)
    d, face, closest, fb = grid.query(S, return_closest=True, return_fallbacks=True)
    res["fallback_share"] = int(fb.item()) / n
    Sa = meshalign.transform_points(S, truth)          # the same samples where the loop ends: on the surface
    res["query_aligned_ms"] = timed(lambda: grid.query(Sa, return_closest=True), steps if a.quick else 10 * steps, warmup)
    res["fallback_share_aligned"] = int(grid.query(Sa, return_fallbacks=True)[2].item()) / n
    origin = meshalign.moments(V)[1]
    res["accumulate_ms"] = timed(lambda: meshalign.accumulate(S, closest, None, d, max_dist, normals, face, origin), many, warmup)
    res["accumulate_fraction_of_copy_rate"] = n * 44 / (res["accumulate_ms"] * 1e-3) / rate
    row = meshalign.accumulate(S, closest, None, d, max_dist, normals, face, origin).cpu().numpy()
    t0 = time.perf_counter()
    for _ in range(100):
        meshalign.solve_plane(row, origin)
    res["solve_plane_host_ms"] = (time.perf_counter() - t0) * 10.0
    t0 = time.perf_counter()
    for _ in range(100):
        meshalign.solve_point(row, True, origin)
    res["solve_point_host_ms"] = (time.perf_counter() - t0) * 10.0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    meshalign.accumulate(S, closest, None, d, max_dist, normals, face, origin).cpu()
    res["accumulate_and_host_read_wall_ms"] = (time.perf_counter() - t0) * 1e3

    def whole():
        return meshalign.icp(S, (V, F), max_dist=max_dist)
    reg = whole()
    res["icp"] = {"iterations": reg["iterations"], "converged": reg["converged"], "fitness": reg["fitness"],
                  "inlier_rmse": reg["inlier_rmse"], "fallbacks": reg["fallbacks"],
                  "fallbacks_by_search": [h["fallbacks"] for h in reg["history"]],
                  "max_abs_error_against_the_known_motion": float(np.abs(reg["transformation"][:3] - truth[:3]).max())}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res["icp"]["events_ms"] = timed(whole, steps, 0)
    res["icp"]["wall_ms"] = (time.perf_counter() - t0) * 1e3 / steps
    res["icp"]["grid_build_ms"] = timed(lambda: meshdist.TriangleGrid(V, F), steps, warmup)
    stages = {k: res[k] for k in ("transform_ms", "query_ms", "accumulate_ms", "solve_plane_host_ms")}
    res["binding_stage"] = max(stages, key=stages.get)
    ref = torch_row(S, np.eye(4), closest, normals, face, d, max_dist)
    res["torch_operators"] = {"transform_and_sums_ms": timed(lambda: torch_row(S, np.eye(4), closest, normals, face, d, max_dist), steps, warmup),
                              "kernels_ms": res["transform_ms"] + res["accumulate_ms"],
                              "kept_pairs_equal": bool(int(ref[0].item()) == int(row[0]))}

    def rounded(x):
        if isinstance(x, float):
            return float(f"{x:.6g}")
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
