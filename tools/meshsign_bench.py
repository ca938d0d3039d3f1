"""Times `lara_amd.meshsign` on one MI355X: HIP events after warm-up, the UV sphere of about 557 k triangles of the neighbouring
benches (tools/meshbvh_bench.py, tools/meshray_bench.py).  Nothing classified a point in this package before, so no time is gated
and there is no baseline; two rows give context only.

  * the rows (crossings and winding sums) of 2 x 10^5 random points in [-1.3, 1.3]^3 under 3 rays;
  * `signed_distance` of the same points (the query, the rows, the vote);
  * `volume_scores` at 128^3 against the rippled copy: the whole call, and its stages one by one;
  * `mesh_volume`;
  * the rows' algorithmic bytes per ray (12 read, 8 written) over their time, as a fraction of the device-to-device copy rate
    measured beside them;
  * context: the first-hit cast of the same rays (`meshray.raycast`), and the same rows in torch operators (float64, all
    triangles) for 64 of the points.

Every figure is the mean of --steps runs in ONE process run: no spread is measured.  Nothing is read from outside the repository.
    python tools/meshsign_bench.py [--steps 10] [--warmup 2] [--quick] [--out profiles/meshsign_bench.json]"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.meshmetrics_bench import sphere_pair, timed  # noqa: E402
from tools.meshsimplify_bench import copy_rate  # noqa: E402


def torch_rows(P, V, F, directions):
    """(cross [N,K], wind [N,K]) of the header's crossing in torch operators, float64, every point against every triangle; a
    touching ray is -1, 0."""
    tri = V[F].double()                                              # [T, 3, 3]
    mn, mx = tri.min(1).values, tri.max(1).values
    o = P.double()
    cross, wind = [], []
    for d in directions:
        d = torch.tensor(d, dtype=torch.float64, device=P.device)
        kz = int(d.abs().argmax())
        kx, ky = (kz + 1) % 3, (kz + 2) % 3
        if d[kz] < 0:
            kx, ky = ky, kx
        Sx, Sy, Sz = d[kx] / d[kz], d[ky] / d[kz], 1.0 / d[kz]

        def shear(p):
            a = p[None] - o[:, None]                                 # [N, T, 3]
            return a[..., kx] - Sx * a[..., kz], a[..., ky] - Sy * a[..., kz], Sz * a[..., kz]
        (Ax, Ay, Az), (Bx, By, Bz), (Cx, Cy, Cz) = shear(tri[:, 0]), shear(tri[:, 1]), shear(tri[:, 2])
        U, Vv, W = Cx * By - Cy * Bx, Ax * Cy - Ay * Cx, Bx * Ay - By * Ax
        det = (U + Vv) + W
        t = ((U * Az + Vv * Bz) + W * Cz) / det
        hit = (((U >= 0) & (Vv >= 0) & (W >= 0)) | ((U <= 0) & (Vv <= 0) & (W <= 0))) & (det != 0) & (t >= 0)
        x = o[:, None] + t[..., None] * d
        m = 2.0 ** -20 * torch.maximum(o.abs()[:, None], torch.maximum(mn.abs(), mx.abs())[None])
        hit &= ((x >= mn[None] - m) & (x <= mx[None] + m)).all(-1)
        touched = (hit & ((U == 0) | (Vv == 0) | (W == 0))).any(1)
        c = hit.sum(1)
        w = (hit * torch.where(det < 0, 1, -1)).sum(1)
        cross.append(torch.where(touched, -1, c))
        wind.append(torch.where(touched, 0, w))
    return torch.stack(cross, 1).int(), torch.stack(wind, 1).int()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="a small sphere, 20 000 points, 32^3, one step")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("meshsign_bench: needs an MI355X")
    from lara_amd import _native, meshbvh, meshray, meshsign
    dev = torch.device("cuda:0")
    n_lat, n_lon = (64, 128) if a.quick else (374, 746)
    N, R = (20000, 32) if a.quick else (200000, 128)
    steps, warmup = (1, 1) if a.quick else (a.steps, a.warmup)
    V, F, V2 = sphere_pair(n_lat, n_lon, dev)
    T = int(F.shape[0])
    rate = copy_rate(dev, (1 << 26) if a.quick else (1 << 30))
    bvh, bvh2 = meshbvh.TriangleBVH(V, F), meshbvh.TriangleBVH(V2, F)
    g = torch.Generator(device=dev).manual_seed(7)
    P = (torch.rand(N, 3, device=dev, generator=g) * 2.6 - 1.3).contiguous()
    K = meshsign.MAX_RAYS
    res = {"Nv": int(V.shape[0]), "T": T, "points": N, "rays": K, "resolution": R, "steps": steps, "warmup": warmup, "one_run": True,
           "copy_rate_GBps": rate / 1e9, "bvh_bytes": int(bvh.nbytes)}
    cross, wind = meshsign.crossings(bvh, P)
    inside, status = meshsign.contains(bvh, P, return_status=True)
    r = P.double().norm(dim=1)
    # every face spans less than `ang` on the unit sphere, so the mesh lies between the radii cos(ang) and 1
    ang = math.hypot(math.pi / n_lat, 2 * math.pi / n_lon)
    res["sagitta_bound"] = 1 - math.cos(ang)
    clear = (r - 1).abs() > res["sagitta_bound"]
    res["inside_share"] = float(inside.float().mean())
    res["agrees_with_the_analytic_sphere_beyond_the_bound"] = bool(torch.equal(inside[clear], (r < 1)[clear]))
    res["unusable_rays"] = int((cross < 0).sum())
    res["points_with_disagreeing_rays"] = int((status & 1).sum())
    res["mean_crossings_per_ray"] = float(cross.clamp(min=0).float().mean())
    res["rows_ms"] = timed(lambda: meshsign.crossings(bvh, P), steps, warmup)
    res["rows_Mrays_per_s"] = N * K / res["rows_ms"] / 1e3
    res["rows_bytes_per_ray"] = 20
    res["rows_fraction_of_copy_rate"] = N * K * 20 / (res["rows_ms"] * 1e-3) / rate
    res["rows_one_ray_ms"] = timed(lambda: meshsign.crossings(bvh, P, 1), steps, warmup)
    res["query_ms"] = timed(lambda: bvh.query(P), steps, warmup)
    res["signed_distance_ms"] = timed(lambda: meshsign.signed_distance(bvh, P), steps, warmup)
    res["mesh_volume_ms"] = timed(lambda: meshsign.mesh_volume(bvh), steps, warmup)
    res["mesh_volume"] = meshsign.mesh_volume(bvh).cpu().tolist()
    # volume_scores: the whole call, then its stages
    scores = meshsign.volume_scores(bvh, bvh2, resolution=R)
    res["volume_scores"] = {k: scores[k] for k in ("volume_iou", "volume_pred", "volume_gt", "volume_pred_mesh", "volume_gt_mesh",
                                                   "unanimous_pred", "unanimous_gt", "n_lattice")}
    res["volume_scores_ms"] = timed(lambda: meshsign.volume_scores(bvh, bvh2, resolution=R), max(1, steps // 2), 1)
    lo, hi = meshsign.union_box(torch.stack([meshsign.root_box(bvh), meshsign.root_box(bvh2)]).cpu().numpy())
    L = meshsign.lattice(lo, hi, R, dev)[0].view(-1, 3)
    rows_a, rows_b = meshsign.crossings(bvh, L), meshsign.crossings(bvh2, L)
    va, vb = meshsign.vote(bvh, *rows_a, 0), meshsign.vote(bvh2, *rows_b, 0)
    counts = torch.empty(8, dtype=torch.int64, device=dev)
    res["volume_scores_stages_ms"] = {
        "lattice": timed(lambda: meshsign.lattice(lo, hi, R, dev), steps, warmup),
        "rows_pred": timed(lambda: meshsign.crossings(bvh, L), steps, warmup),
        "rows_gt": timed(lambda: meshsign.crossings(bvh2, L), steps, warmup),
        "vote_each": timed(lambda: meshsign.vote(bvh, *rows_a, 0), steps, warmup),
        "counts": timed(lambda: _native.call("lara_meshsign_counts", dev, L.shape[0], va[0], va[1], vb[0], vb[1], counts), steps, warmup),
        "mesh_volume_each": res["mesh_volume_ms"]}
    res["lattice_rows_Mrays_per_s"] = L.shape[0] * K / res["volume_scores_stages_ms"]["rows_pred"] / 1e3
    # context rows, not baselines
    D = torch.tensor(meshsign.DIRECTIONS, dtype=torch.float32, device=dev)
    o, d = P.repeat_interleave(K, 0).contiguous(), D.repeat(N, 1).contiguous()
    res["context_first_hit_same_rays_ms"] = timed(lambda: meshray.raycast(bvh, o, d), steps, warmup)
    pick = torch.randint(0, N, (64,), device=dev, generator=g)
    Pt = P[pick].contiguous()
    tc, tw = torch_rows(Pt, V, F, meshsign.DIRECTIONS)
    kc, kw = meshsign.crossings(bvh, Pt)
    res["context_torch_64_points"] = {"ms": timed(lambda: torch_rows(Pt, V, F, meshsign.DIRECTIONS), max(1, steps // 5), 1),
                                      "kernel_ms": timed(lambda: meshsign.crossings(bvh, Pt), steps, warmup),
                                      "same_rows": bool(torch.equal(tc, kc) and torch.equal(tw, kw))}

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
