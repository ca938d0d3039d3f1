"""Times `lara_amd.meshbvh.TriangleBVH` against `lara_amd.meshdist.TriangleGrid` on one MI355X: the same process, the two
structures alternating row by row, HIP events after warm-up.  The meshes are those of tools/meshdist_bench.py (the UV sphere of
about 557 k triangles, queries sampled from its rippled copy) and tools/meshalign_bench.py (the same sphere under the asymmetric
warp, the source 2 x 10^5 samples of it moved by a known 10 degree motion).

  * build time and bytes of both structures;
  * 2 x 10^5 and 10^6 near-surface queries;
  * 64 queries at the pole of the UV sphere, where the grid's cell lists are longest;
  * the 2 x 10^5 queries 10 degrees off (with closest points, as `icp` asks for them), where a third of the grid's queries fall
    back to brute force, and the same samples once aligned;
  * 4 096 queries deep inside the sphere: the grid's brute-force route alone;
  * one whole `icp` call (plane mode) with search="grid" and search="bvh", by HIP events and by the host clock;
  * for every row: whether the two searches returned the same bits.

Every figure is the mean of --steps runs in ONE process run: no spread is measured.  Nothing is read from outside the repository.
    python tools/meshbvh_bench.py [--steps 10] [--warmup 2] [--quick] [--out profiles/meshbvh_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.meshalign_bench import warp  # noqa: E402
from tools.meshmetrics_bench import sphere_pair, timed  # noqa: E402


def same_bits(a, b):
    return all(torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)) for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="a small sphere, one step (the test suite's run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("meshbvh_bench: needs an MI355X")
    from lara_amd import meshalign, meshbvh, meshdist, meshmetrics
    dev = torch.device("cuda:0")
    n_lat, n_lon = (64, 128) if a.quick else (374, 746)
    steps, warmup = (1, 1) if a.quick else (a.steps, a.warmup)
    V, F, Vr = sphere_pair(n_lat, n_lon, dev)
    T = int(F.shape[0])
    res = {"Nv": int(V.shape[0]), "T": T, "steps": steps, "warmup": warmup, "one_run": True, "rows": []}

    def both(name, grid, bvh, Q, closest, n_steps=None):
        """One row: the two queries timed in turn (grid, bvh, grid, bvh: the means of the two turns each), and compared."""
        n_steps = n_steps or steps
        g = grid.query(Q, return_closest=closest, return_fallbacks=True)
        b = bvh.query(Q, return_closest=closest, return_fallbacks=True)
        t = {"grid": [], "bvh": []}
        for _ in range(2):
            t["grid"].append(timed(lambda: grid.query(Q, return_closest=closest), n_steps, warmup))
            t["bvh"].append(timed(lambda: bvh.query(Q, return_closest=closest), n_steps, warmup))
        row = {"row": name, "n": int(Q.shape[0]), "with_closest": closest, "grid_ms": float(np.mean(t["grid"])),
               "bvh_ms": float(np.mean(t["bvh"])), "grid_fallback_share": int(g[-1].item()) / Q.shape[0],
               "bvh_fallbacks": int(b[-1].item()), "same_bits": same_bits(g[:-1], b[:-1]), "mean_distance": float(g[0].double().mean())}
        row["grid_over_bvh"] = row["grid_ms"] / row["bvh_ms"]
        res["rows"].append(row)
        return row

    grid, bvh = meshdist.TriangleGrid(V, F), meshbvh.TriangleBVH(V, F)
    counts = bvh.counts.cpu().tolist()
    res["build"] = {"grid_ms": timed(lambda: meshdist.TriangleGrid(V, F), steps, warmup),
                    "bvh_ms": timed(lambda: meshbvh.TriangleBVH(V, F), steps, warmup),
                    "grid_bytes": int(grid.grid.numel()), "bvh_bytes": int(bvh.nbytes), "bvh_bytes_per_triangle": bvh.nbytes / T,
                    "bvh_levels": counts[3], "bvh_valid_triangles": counts[1], "bvh_refused_triangles": counts[0]}
    keys = bvh.keys.clone()
    res["build"]["bvh_sort_alone_ms"] = timed(lambda: torch.sort(keys), steps, warmup)
    for n in ((20000,) if a.quick else (200000, 1000000)):
        both(f"{n} near-surface queries", grid, bvh, meshmetrics.sample_surface(Vr, F, n, seed=0)[0], False)
    g = torch.Generator(device=dev).manual_seed(3)
    pole = torch.tensor([0.0, 0.0, 1.0], device=dev) + (torch.rand(64, 3, device=dev, generator=g) - 0.5) * 2e-3
    both("64 queries at the pole", grid, bvh, pole.contiguous(), False)
    Qin = (meshmetrics.sample_surface(Vr, F, 4096, seed=0)[0] * 0.2).contiguous()
    both("4096 queries deep inside (the grid's brute-force route)", grid, bvh, Qin, False, 1 if a.quick else max(1, steps // 5))

    # the registration of tools/meshalign_bench.py
    n = 20000 if a.quick else 200000
    max_dist = 0.3
    Vw = warp(V)
    axis = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    truth = np.eye(4)
    truth[:3, :3], truth[:3, 3] = meshalign.rodrigues(axis * np.deg2rad(10.0)), (0.04, -0.04, 0.04)
    S = meshalign.transform_points(meshmetrics.sample_surface(Vw, F, n, seed=0)[0], np.linalg.inv(truth))
    gridw, bvhw = meshdist.TriangleGrid(Vw, F), meshbvh.TriangleBVH(Vw, F)
    both(f"{n} queries 10 degrees off", gridw, bvhw, S, True, 1 if a.quick else max(1, steps // 2))
    both(f"{n} queries aligned", gridw, bvhw, meshalign.transform_points(S, truth), True)
    res["icp"] = {}
    regs = {}
    for _ in range(2 if not a.quick else 1):
        for search in ("grid", "bvh"):
            def whole():
                return meshalign.icp(S, (Vw, F), max_dist=max_dist, search=search)
            regs[search] = whole()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev = timed(whole, 1 if a.quick else max(1, steps // 2), 0)
            wall = (time.perf_counter() - t0) * 1e3 / (1 if a.quick else max(1, steps // 2))
            r = res["icp"].setdefault(search, {"events_ms": [], "wall_ms": []})
            r["events_ms"].append(ev)
            r["wall_ms"].append(wall)
    for search, reg in regs.items():
        r = res["icp"][search]
        r["events_ms"], r["wall_ms"] = float(np.mean(r["events_ms"])), float(np.mean(r["wall_ms"]))
        r.update({"iterations": reg["iterations"], "converged": reg["converged"], "fallbacks": reg["fallbacks"],
                  "fallbacks_by_search": [h["fallbacks"] for h in reg["history"]],
                  "max_abs_error_against_the_known_motion": float(np.abs(reg["transformation"][:3] - truth[:3]).max())})
    res["icp"]["same_transformation_bits"] = bool(np.array_equal(regs["grid"]["transformation"].view(np.int64),
                                                                 regs["bvh"]["transformation"].view(np.int64)))
    res["icp"]["grid_over_bvh"] = res["icp"]["grid"]["wall_ms"] / res["icp"]["bvh"]["wall_ms"]
    res["all_rows_same_bits"] = all(r["same_bits"] for r in res["rows"])

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
