"""Times `lara_amd.meshwind` on one MI355X: HIP events after warm-up, the UV sphere of about 557 k triangles of the neighbouring
benches (tools/meshbvh_bench.py, tools/meshsign_bench.py).  Nothing computed a winding number in this package before, so no time is
gated and no row has a baseline; `meshsign.crossings` on the same points stands beside the rows as context only.

  * the moments build (`WindingField` on a built hierarchy);
  * `winding` of 2 x 10^5 random points in [-1.3, 1.3]^3 for beta = 2 and 3, with the mean counters; beta = inf (the exact sum in
    tree order: every triangle for every point) on the first 2 000 of them;
  * how far beta = 2 and 3 are from beta = inf on those 2 000 points, and that `contains` agrees with the analytic sphere beyond
    the mesh's sagitta;
  * `volume_scores` at 128^3 against the rippled copy;
  * context: `meshsign.crossings` (3 rays) of the same points.

Every figure is the mean of --steps runs in ONE process run: no spread is measured.  Nothing is read from outside the repository.
    python tools/meshwind_bench.py [--steps 10] [--warmup 2] [--quick] [--out profiles/meshwind_bench.json]"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.meshmetrics_bench import sphere_pair, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="a small sphere, 20 000 points, 32^3, one step")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("meshwind_bench: needs an MI355X")
    from lara_amd import meshbvh, meshsign, meshwind
    dev = torch.device("cuda:0")
    n_lat, n_lon = (64, 128) if a.quick else (374, 746)
    N, R, N_exact = (20000, 32, 500) if a.quick else (200000, 128, 2000)
    steps, warmup = (1, 1) if a.quick else (a.steps, a.warmup)
    V, F, V2 = sphere_pair(n_lat, n_lon, dev)
    T = int(F.shape[0])
    bvh, bvh2 = meshbvh.TriangleBVH(V, F), meshbvh.TriangleBVH(V2, F)
    g = torch.Generator(device=dev).manual_seed(7)
    P = (torch.rand(N, 3, device=dev, generator=g) * 2.6 - 1.3).contiguous()
    Pe = P[:N_exact].contiguous()
    field, field2 = meshwind.WindingField(bvh), meshwind.WindingField(bvh2)
    res = {"Nv": int(V.shape[0]), "T": T, "points": N, "points_exact": N_exact, "resolution": R, "steps": steps, "warmup": warmup,
           "one_run": True, "bvh_bytes": int(bvh.nbytes), "moments_bytes": int(field.moments.shape[0])}
    res["moments_ms"] = timed(lambda: meshwind.WindingField(bvh), steps, warmup)
    exact = meshwind.winding(field, Pe, float("inf"))
    res["rows_ms"], res["mean_triangles_tested"], res["mean_far_nodes"], res["max_error_against_beta_inf"] = {}, {}, {}, {}
    for beta in (2.0, 3.0):
        w, n_tri, n_far = meshwind.winding(field, P, beta, return_counts=True)
        key = f"{beta:g}"
        res["rows_ms"][key] = timed(lambda: meshwind.winding(field, P, beta), steps, warmup)
        res["mean_triangles_tested"][key] = float(n_tri.float().mean())
        res["mean_far_nodes"][key] = float(n_far.float().mean())
        res["max_error_against_beta_inf"][key] = float((w[:N_exact] - exact).abs().max())
    res["rows_Mpoints_per_s"] = {k: N / v / 1e3 for k, v in res["rows_ms"].items()}
    res["rows_ms"]["inf"] = timed(lambda: meshwind.winding(field, Pe, float("inf")), max(1, steps // 5), 1)
    res["rows_inf_Gterms_per_s"] = N_exact * T / res["rows_ms"]["inf"] / 1e6
    inside, status = meshwind.contains(field, P, return_status=True)
    r = P.double().norm(dim=1)
    # every face spans less than `ang` on the unit sphere, so the mesh lies between the radii cos(ang) and 1
    ang = math.hypot(math.pi / n_lat, 2 * math.pi / n_lon)
    res["sagitta_bound"] = 1 - math.cos(ang)
    clear = (r - 1).abs() > res["sagitta_bound"]
    res["inside_share"] = float(inside.float().mean())
    res["agrees_with_the_analytic_sphere_beyond_the_bound"] = bool(torch.equal(inside[clear], (r < 1)[clear]))
    res["points_in_the_band"] = int((status & 1).sum())
    res["signed_distance_ms"] = timed(lambda: meshwind.signed_distance(field, P), steps, warmup)
    scores = meshwind.volume_scores(field, field2, resolution=R)
    res["volume_scores"] = {k: scores[k] for k in ("volume_iou", "volume_pred", "volume_gt", "volume_pred_mesh", "volume_gt_mesh",
                                                   "decided_pred", "decided_gt", "n_lattice")}
    res["volume_scores_ms"] = timed(lambda: meshwind.volume_scores(field, field2, resolution=R), max(1, steps // 2), 1)
    # context rows, not baselines
    res["context_meshsign_crossings_3_rays_ms"] = timed(lambda: meshsign.crossings(bvh, P), steps, warmup)
    res["context_meshsign_volume_iou"] = meshsign.volume_scores(bvh, bvh2, resolution=R)["volume_iou"]

    def rounded(x):
        if isinstance(x, float):
            return float(f"{x:.6g}")
        if isinstance(x, dict):
            return {k: rounded(v) for k, v in x.items()}
        return x
    line = json.dumps(rounded(res))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
