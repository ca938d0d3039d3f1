"""Times `lara_amd.meshmetrics.surface_scores` on one MI355X with HIP events after warm-up, at 2 x 10^5 and 10^6 samples per side,
on a synthetic pair built here: a UV sphere of about 557 k triangles (the size of bench.py's mesh_eval mesh) and a copy whose radius
is perturbed by a smooth 1 % ripple.

Beside it the only device route the package had before: chunked `torch.cdist` + `min` over the same samples, both directions
(chunks of 2^30 / M query rows, i.e. a 4 GiB distance block at a time).  That baseline is O(N M); it runs once after a warm-up on
one chunk (10 s at 10^6), the grid route --steps times (a window of 0.1 s and more).  `grid_ms` is the whole call (sampling both meshes, its two 16-byte host reads, both searches, the reduction and its host
read); `sample_ms`, `nearest_ms` and `reduce_ms` are the parts, timed on their own.  `fallback_share`: queries of either direction
the brute-force kernel resolved.  Nothing is read from outside the repository.
    python tools/meshmetrics_bench.py [--steps 50] [--warmup 5] [--quick] [--out profiles/meshmetrics_bench.json]"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def sphere_pair(n_lat, n_lon, dev):
    """(vertices, triangles) of a closed UV sphere and the perturbed copy's vertices: r = 1 + 0.01 sin(5 theta) cos(7 phi)."""
    th = torch.arange(1, n_lat, device=dev, dtype=torch.float64) * (math.pi / n_lat)
    ph = torch.arange(n_lon, device=dev, dtype=torch.float64) * (2 * math.pi / n_lon)
    T, P = torch.meshgrid(th, ph, indexing="ij")
    body = torch.stack([T.sin() * P.cos(), T.sin() * P.sin(), T.cos()], -1).reshape(-1, 3)
    poles = torch.tensor([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0]], device=dev, dtype=torch.float64)
    V = torch.cat([poles[:1], body, poles[1:]])
    ripple = torch.cat([torch.zeros(1, device=dev, dtype=torch.float64), (5 * T).sin().reshape(-1) * (7 * P).cos().reshape(-1),
                        torch.zeros(1, device=dev, dtype=torch.float64)])
    i = torch.arange(n_lat - 2, device=dev).reshape(-1, 1)
    j = torch.arange(n_lon, device=dev).reshape(1, -1)
    a, b = 1 + i * n_lon + j, 1 + i * n_lon + (j + 1) % n_lon
    c, d = a + n_lon, b + n_lon
    quads = torch.cat([torch.stack([a, c, d], -1).reshape(-1, 3), torch.stack([a, d, b], -1).reshape(-1, 3)])
    j1, j2 = j.reshape(-1), (j.reshape(-1) + 1) % n_lon
    south, last = V.shape[0] - 1, 1 + (n_lat - 2) * n_lon
    caps = torch.cat([torch.stack([torch.zeros_like(j1), 1 + j1, 1 + j2], -1),
                      torch.stack([torch.full_like(j1, south), last + j2, last + j1], -1)])
    return V.float(), torch.cat([quads, caps]).long(), (V * (1 + 0.01 * ripple).unsqueeze(1)).float()


def cdist_directed(Q, P):
    """min_j |Q_i - P_j| for every i, a chunk of query rows at a time."""
    step = max(1, (1 << 30) // max(P.shape[0], 1))
    return torch.cat([torch.cdist(Q[o:o + step], P).min(1).values for o in range(0, Q.shape[0], step)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="one size of 2 x 10^4 samples on a small sphere (the test suite's run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("meshmetrics_bench: needs an MI355X")
    from lara_amd import meshmetrics
    dev = torch.device("cuda:0")
    n_lat, n_lon = (64, 128) if a.quick else (374, 746)
    sizes = (20000,) if a.quick else (200000, 1000000)
    steps, warmup = (1, 1) if a.quick else (a.steps, a.warmup)
    V, F, V2 = sphere_pair(n_lat, n_lon, dev)
    res = {"Nv": int(V.shape[0]), "T": int(F.shape[0]), "steps": steps, "warmup": warmup, "sizes": []}
    for n in sizes:
        run = lambda: meshmetrics.surface_scores((V2, F), (V, F), n=n)
        scores = run()
        row = {"samples_per_side": n, "grid_resolution": meshmetrics.grid_resolution(n), "chamfer": scores["chamfer"],
               "fscore": scores["fscore"], "thresholds": scores["thresholds"],
               "fallback_share": scores["fallbacks"] / (2.0 * n)}
        row["grid_ms"] = timed(run, steps, warmup)
        row["sample_ms"] = timed(lambda: (meshmetrics.sample_surface(V2, F, n), meshmetrics.sample_surface(V, F, n)), steps, warmup)
        P, Pn, _ = meshmetrics.sample_surface(V2, F, n)
        G, Gn, _ = meshmetrics.sample_surface(V, F, n)
        row["nearest_ms"] = timed(lambda: (meshmetrics.nearest(P, G), meshmetrics.nearest(G, P)), steps, warmup)
        row["reduce_ms"] = timed(lambda: meshmetrics.surface_scores((P, Pn), (G, Gn)), steps, warmup) - row["nearest_ms"]
        # the baseline: warm-up on one chunk of each direction, then one timed pass (it is O(N M))
        step = max(1, (1 << 30) // n)
        cdist_directed(P[:step], G), cdist_directed(G[:step], P)
        seen = {}

        def both():
            seen["chamfer"] = cdist_directed(P, G).double().mean() + cdist_directed(G, P).double().mean()
        row["cdist_ms"] = timed(both, 1, 0)
        row["cdist_chamfer"] = float(seen["chamfer"])
        row["cdist_over_grid"] = row["cdist_ms"] / row["nearest_ms"]
        res["sizes"].append(row)
    res["sizes"] = [{k: (round(x, 6) if isinstance(x, float) else x) for k, x in row.items()} for row in res["sizes"]]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
