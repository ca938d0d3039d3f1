"""Times `lara_amd.meshray` on one MI355X: HIP events after warm-up, the UV sphere of about 557 k triangles of the neighbouring
benches (tools/meshdist_bench.py, tools/meshbvh_bench.py).  Nothing cast a ray in this package before, so no time is gated and
there is no baseline; two rows give context only.

  * first hit for 8 views of 512 x 512 primary rays (the orbit of `evaluate.video_cameras`), with the sibling order the walk uses
    and with the other one, the two alternating, and whether they returned the same bits;
  * any hit on the same rays;
  * `visibility` of 2 x 10^5 surface samples (their faces skipped) against the 8 camera centres;
  * every row's algorithmic bytes over its time, as a fraction of the device-to-device copy rate measured beside it;
  * context: `meshrender`'s depth output for the same cameras (a rasteriser: all pixels of a frame at once), and the same cast in
    torch operators (float64, all triangles) on 64 of the rays.

Every figure is the mean of --steps runs in ONE process run: no spread is measured.  Nothing is read from outside the repository.
    python tools/meshray_bench.py [--steps 10] [--warmup 2] [--quick] [--out profiles/meshray_bench.json]"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.meshmetrics_bench import sphere_pair, timed  # noqa: E402
from tools.meshsimplify_bench import copy_rate  # noqa: E402


def torch_first_hit(o, d, V, F):
    """(t [R], face [R]) of the header's ray-triangle function in torch operators, float64, every ray against every triangle."""
    o, d = o.double(), d.double()
    kz = d.abs().argmax(1)
    kx, ky = (kz + 1) % 3, (kz + 2) % 3
    neg = d.gather(1, kz[:, None])[:, 0] < 0
    kx, ky = torch.where(neg, ky, kx), torch.where(neg, kx, ky)
    dz = d.gather(1, kz[:, None])
    Sx, Sy, Sz = d.gather(1, kx[:, None]) / dz, d.gather(1, ky[:, None]) / dz, 1.0 / dz
    P = V[F].double()                                               # [T, 3, 3]
    mn, mx = P.min(1).values, P.max(1).values

    def shear(p):
        a = p[None] - o[:, None]                                    # [R, T, 3]
        pick = lambda k: a.gather(2, k[:, None, None].expand(-1, a.shape[1], 1))[..., 0]
        az = pick(kz)
        return pick(kx) - Sx * az, pick(ky) - Sy * az, Sz * az
    (Ax, Ay, Az), (Bx, By, Bz), (Cx, Cy, Cz) = shear(P[:, 0]), shear(P[:, 1]), shear(P[:, 2])
    U, W_, Vv = Cx * By - Cy * Bx, Bx * Ay - By * Ax, Ax * Cy - Ay * Cx
    det = (U + Vv) + W_
    t = ((U * Az + Vv * Bz) + W_ * Cz) / det
    hit = (((U >= 0) & (Vv >= 0) & (W_ >= 0)) | ((U <= 0) & (Vv <= 0) & (W_ <= 0))) & (det != 0) & (t >= 0)
    x = o[:, None] + t[..., None] * d[:, None]
    m = 2.0 ** -20 * torch.maximum(o.abs()[:, None], torch.maximum(mn.abs(), mx.abs())[None])
    hit &= ((x >= mn[None] - m) & (x <= mx[None] + m)).all(-1)
    t = torch.where(hit, t, torch.full_like(t, math.inf))
    best = t.min(1)
    return best.values, torch.where(torch.isfinite(best.values), best.indices, torch.full_like(best.indices, -1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="a small sphere, 128 x 128 views, one step (the test suite's size)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("meshray_bench: needs an MI355X")
    from lara_amd import evaluate, meshbvh, meshmetrics, meshray, meshrender
    dev = torch.device("cuda:0")
    n_lat, n_lon = (64, 128) if a.quick else (374, 746)
    S, n_samples = (128, 20000) if a.quick else (512, 200000)
    steps, warmup = (1, 1) if a.quick else (a.steps, a.warmup)
    V, F, _ = sphere_pair(n_lat, n_lon, dev)
    T, n_views = int(F.shape[0]), 8
    rate = copy_rate(dev, (1 << 26) if a.quick else (1 << 30))
    bvh = meshbvh.TriangleBVH(V, F)
    cams = evaluate.video_cameras(n_views, "gobjeverse", (S, S), device=dev)
    c2w = torch.stack([torch.linalg.inv_ex(c.world_view_transform.double().t())[0] for c in cams]).cpu().numpy()
    ixt = np.zeros((n_views, 3, 3))
    ixt[:, 0, 0], ixt[:, 1, 1] = S / (2 * math.tan(cams[0].FoVx / 2)), S / (2 * math.tan(cams[0].FoVy / 2))
    ixt[:, 0, 2], ixt[:, 1, 2], ixt[:, 2, 2] = S / 2, S / 2, 1.0
    o, d = meshray.pixel_rays(ixt, c2w, S, S, dev)
    o, d = o.view(-1, 3), d.view(-1, 3)
    R = int(o.shape[0])
    res = {"Nv": int(V.shape[0]), "T": T, "views": n_views, "size": S, "rays": R, "steps": steps, "warmup": warmup, "one_run": True,
           "copy_rate_GBps": rate / 1e9, "bvh_bytes": int(bvh.nbytes), "masked_order_is_the_default": bool(meshray.MASKED_ORDER)}
    first = meshray.raycast(bvh, o, d, return_bary=True)
    other = meshray.raycast(bvh, o, d, return_bary=True, other_order=True)
    res["hit_share"] = float((first[1] >= 0).float().mean())
    res["both_orders_same_bits"] = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(first, other))
    t = {"default": [], "other": []}
    for _ in range(2):          # the two orders alternate; the mean of the two turns each
        t["default"].append(timed(lambda: meshray.raycast(bvh, o, d), steps, warmup))
        t["other"].append(timed(lambda: meshray.raycast(bvh, o, d, other_order=True), steps, warmup))
    names = ("sign_mask", "stored") if meshray.MASKED_ORDER else ("stored", "sign_mask")
    res["first_hit_ms"] = {names[0]: float(np.mean(t["default"])), names[1]: float(np.mean(t["other"]))}
    res["first_hit_fraction_of_copy_rate"] = R * 32 / (res["first_hit_ms"][names[0]] * 1e-3) / rate
    res["first_hit_Mrays_per_s"] = R / res["first_hit_ms"][names[0]] / 1e3
    occ = meshray.occluded(bvh, o, d)
    res["any_hit_equals_first_hit"] = bool(torch.equal(occ, first[1] >= 0))
    res["any_hit_ms"] = timed(lambda: meshray.occluded(bvh, o, d), steps, warmup)
    res["any_hit_fraction_of_copy_rate"] = R * 25 / (res["any_hit_ms"] * 1e-3) / rate
    P, _, faces = meshmetrics.sample_surface(V, F, n_samples, seed=0)
    eyes = torch.from_numpy(c2w[:, :3, 3]).to(dev, torch.float32)
    seen = meshray.visibility(bvh, P, eyes, faces)
    res["visibility"] = {"samples": n_samples, "eyes": n_views, "ms": timed(lambda: meshray.visibility(bvh, P, eyes, faces), steps, warmup),
                         "visible_share_of_pairs": float(sum(((seen >> e) & 1).float().mean() for e in range(n_views)) / n_views)}
    res["visibility"]["fraction_of_copy_rate"] = n_samples * 24 / (res["visibility"]["ms"] * 1e-3) / rate
    res["visibility"]["Mrays_per_s"] = n_samples * n_views / res["visibility"]["ms"] / 1e3
    # context rows, not baselines
    res["context_meshrender_depth_ms"] = timed(lambda: meshrender.render_mesh_views(cams, V, F, None, chunk=8, outputs=("depth",), check=False),
                                               steps, warmup)
    g = torch.Generator(device=dev).manual_seed(5)
    pick = torch.randint(0, R, (64,), device=dev, generator=g)
    ot, dt = o[pick].contiguous(), d[pick].contiguous()
    tt, ft = torch_first_hit(ot, dt, V, F)
    kt, kf = meshray.raycast(bvh, ot, dt)
    res["context_torch_64_rays"] = {"ms": timed(lambda: torch_first_hit(ot, dt, V, F), max(1, steps // 5), 1),
                                    "kernel_ms": timed(lambda: meshray.raycast(bvh, ot, dt), steps, warmup),
                                    "same_faces": bool(torch.equal(ft.int(), kf)), "same_t_as_fp32": bool(torch.equal(tt.float(), kt))}

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
