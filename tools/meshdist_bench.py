"""Times `lara_amd.meshdist` on one MI355X with HIP events after warm-up, on the sphere of tools/meshsimplify_bench.py (about 557 k
triangles of about one TSDF voxel each), with queries sampled from its 1 % rippled copy:

  * the build and the query separately (2 x 10^5 and 10^6 queries), and one whole `mesh_scores` call; each next to the device's
    copy rate measured in the same run: the algorithmic bytes (every input and output once) over the time, as a fraction of it;
  * the grid's figures: (triangle, cell) pairs per triangle, the large list's length, the share of queries that fell back.  The
    triangle tests per query are NOT measured (the kernels keep no such counter); tests/test_meshdist.py prints the restated
    search's figure for its cases;
  * as CONTEXT only: the same queries through `meshmetrics.nearest` against 10^6 samples of the sphere (the route this one
    replaces in meaning, not in speed); the brute-force kernel alone, on 4 096 of the queries pulled to a fifth of their radius so
    that every one of them falls back; the same computation in torch operators (float64, written here) on 64 of the queries;
  * THE ACCURACY TABLE: `mesh_scores` and `surface_scores` of the sphere simplified at 2, 4 and 8 voxels against the input, and
    of the input against itself (the same surface with its triangles in another order, so that the two sides' samples differ).

Nothing computed this before: there is no baseline and no time ratio to meet.  Nothing is read from outside the repository.
    python tools/meshdist_bench.py [--steps 10] [--warmup 2] [--quick] [--out profiles/meshdist_bench.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.meshmetrics_bench import sphere_pair, timed  # noqa: E402
from tools.meshsimplify_bench import copy_rate  # noqa: E402


def _dot(a, b):
    return (a * b).sum(-1)


def torch_point_triangle(q, p0, p1, p2):
    """[N, T] squared distances in float64 with torch operators: q [N,1,3] against p0, p1, p2 [1,T,3]."""
    def segment(a, b):
        ab, aq = b - a, q - a
        den = _dot(ab, ab)
        t = torch.where(den > 0, (_dot(aq, ab) / den.clamp_min(1e-300)).clamp(0.0, 1.0), torch.zeros_like(den))
        d = q - (a + t.unsqueeze(-1) * ab)
        return _dot(d, d)
    n = torch.linalg.cross(p1 - p0, p2 - p0)
    nn = _dot(n, n)
    inside = (nn > 0) & (_dot(torch.linalg.cross((p1 - p0).expand_as(q - p0), q - p0), n) >= 0) \
        & (_dot(torch.linalg.cross((p2 - p1).expand_as(q - p1), q - p1), n) >= 0) \
        & (_dot(torch.linalg.cross((p0 - p2).expand_as(q - p2), q - p2), n) >= 0)
    s = _dot(n, q - p0)
    edges = torch.minimum(torch.minimum(segment(p0, p1), segment(p1, p2)), segment(p2, p0))
    return torch.where(inside, s * s / nn.clamp_min(1e-300), edges)


def torch_distances(Q, V, F, chunk=8):
    p = [V[F[:, k]].double().unsqueeze(0) for k in range(3)]
    return torch.cat([torch_point_triangle(Q[o:o + chunk].double().unsqueeze(1), *p).min(1).values.sqrt() for o in range(0, Q.shape[0], chunk)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="a small sphere, one step (the test suite's run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("meshdist_bench: needs an MI355X")
    from lara_amd import meshdist, meshmetrics, meshsimplify
    dev = torch.device("cuda:0")
    n_lat, n_lon = (64, 128) if a.quick else (374, 746)
    steps, warmup = (1, 1) if a.quick else (a.steps, a.warmup)
    voxel = 2.0 / 256 * (374 / n_lat)
    V, F, Vr = sphere_pair(n_lat, n_lon, dev)
    Nv, T = int(V.shape[0]), int(F.shape[0])
    rate = copy_rate(dev, (1 << 26) if a.quick else (1 << 30))
    grid = meshdist.TriangleGrid(V, F)
    bad, n_large, pairs, _ = grid.counts.cpu().tolist()
    res = {"Nv": Nv, "T": T, "steps": steps, "warmup": warmup, "copy_rate_GBps": rate / 1e9,
           "grid_resolution": meshdist.grid_resolution(T), "grid_MB": grid.grid.numel() / 1e6, "refused_triangles": bad,
           "large_list": n_large, "pairs_per_triangle": (pairs & 0xffffffff) / max(T - n_large - bad, 1), "tests_per_query": None}
    res["build_ms"] = timed(lambda: meshdist.TriangleGrid(V, F), steps, warmup)
    res["build_fraction_of_copy_rate"] = (Nv * 12 + T * 12 + T * 48 + pairs * 4) / (res["build_ms"] * 1e-3) / rate

    def normals():
        grid._normals = None
        return grid.face_normals
    res["face_normals_ms"] = timed(normals, steps, warmup)
    res["queries"] = []
    n_context = 20000 if a.quick else 1000000
    targets = meshmetrics.sample_surface(V, F, n_context, seed=1)[0]
    for n in ((20000,) if a.quick else (200000, 1000000)):
        Q = meshmetrics.sample_surface(Vr, F, n, seed=0)[0]
        d, face, fb = grid.query(Q, return_fallbacks=True)
        row = {"n": n, "fallback_share": int(fb.item()) / n, "mean_distance": float(d.double().mean())}
        row["query_ms"] = timed(lambda: grid.query(Q), steps, warmup)
        row["query_with_closest_ms"] = timed(lambda: grid.query(Q, return_closest=True), steps, warmup)
        row["queries_per_second"] = n / (row["query_ms"] * 1e-3)
        row["fraction_of_copy_rate"] = (n * (12 + 8)) / (row["query_ms"] * 1e-3) / rate
        row["context_nearest_ms"], row["context_nearest_targets"] = timed(lambda: meshmetrics.nearest(Q, targets), steps, warmup), n_context
        res["queries"].append(row)
    # the brute-force kernel alone: 4 096 queries deep inside the sphere, where the rings find nothing
    Qb = (Q[:4096] * 0.2).contiguous()
    fb = grid.query(Qb, return_fallbacks=True)[2]
    ms = timed(lambda: grid.query(Qb), steps, warmup)
    res["brute_force"] = {"queries": int(Qb.shape[0]), "fallbacks": int(fb.item()), "ms": ms,
                          "ms_scaled_to_the_largest_query_set": ms * res["queries"][-1]["n"] / Qb.shape[0],
                          "grid_query_ms_of_that_set": res["queries"][-1]["query_ms"]}
    # the same computation in torch operators (float64), on 64 of the queries
    Qt = Q[:64].contiguous()
    ref = torch_distances(Qt, V, F)
    res["torch_operators"] = {"queries": 64, "ms": timed(lambda: torch_distances(Qt, V, F), 1, 1),
                              "grid_query_ms": timed(lambda: grid.query(Qt), steps, warmup),
                              "worst_difference": float((grid.query(Qt)[0].double() - ref).abs().max())}
    # the accuracy table: point mode against triangle mode
    n_s = 20000 if a.quick else 200000
    keys = ("accuracy", "completeness", "chamfer", "fscore", "normal_consistency")
    C = (0.5 * V + 0.5).contiguous()
    perm = torch.randperm(T, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    pairs_ = [("input against itself", (V, F[perm]))]
    for mult in (8, 4, 2):
        V2, F2, _, _ = meshsimplify.simplify_vertex_clustering(V, F, C, mult * voxel, "quadric")
        pairs_.append((f"simplified at {mult} voxels against the input", (V2, F2)))
    res["accuracy_table"] = []
    for name, pred in pairs_:
        row = {"pair": name, "triangles": int(pred[1].shape[0]), "samples_per_side": n_s}
        for mode in ("point", "triangle"):
            s = meshmetrics.surface_scores(pred, (V, F), n=n_s, distance=mode)
            row[mode] = {k: s[k] for k in keys}
            row[mode]["fallbacks"] = s["fallbacks"]
        res["accuracy_table"].append(row)
    V2, F2 = pairs_[2][1]
    res["mesh_scores_ms"] = timed(lambda: meshdist.mesh_scores((V2, F2), (V, F), n=n_s), steps, warmup)
    res["surface_scores_point_ms"] = timed(lambda: meshmetrics.surface_scores((V2, F2), (V, F), n=n_s), steps, warmup)
    res["mesh_scores_pair"] = pairs_[2][0]

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
