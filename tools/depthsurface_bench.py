"""Times `lara_amd.depthsurface` on one MI355X with HIP events after warm-up, on a scene built here: 8 views at 512 x 512 of the unit
sphere, ray-cast analytically on the device (cameras on a ring and above / below, looking at the origin), and 10^5 and 10^6 samples of
the UV sphere of tools/meshmetrics_bench.py (its rippled copy: the prediction).

Per stage -- `backproject` (with depth normals; its one host read included), `thin` (voxel = 2 / 256; its host read included),
`observe`, `reduce` (both directions) -- and for the whole `depth_scores` call (the nearest-neighbour searches of
`lara_amd.meshmetrics` included, on an already sampled point set): milliseconds; the algorithmic bytes of the streaming stages
(every input and output once) as a fraction of the device's copy rate, measured here on a 1 GiB buffer; the share of samples no
view observed.

Nothing did this before, so the comparison is the same computation written in torch operators, here: a boolean-index
back-projection (points only: the normals have no short torch form), `torch.unique` thinning with a scatter-min for the winners,
a projected gather per view for the observation test.  Nothing is read from outside the repository.
    python tools/depthsurface_bench.py [--steps 20] [--warmup 3] [--quick] [--out profiles/depthsurface_bench.json]"""
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


def copy_rate(dev, nbytes=1 << 30, steps=10):
    """bytes read + written per second of a device-to-device copy."""
    a = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    b = torch.empty_like(a)
    return 2.0 * nbytes / (timed(lambda: b.copy_(a), steps, 2) * 1e-3)


def look_at(eye):
    eye = np.asarray(eye, np.float64)
    f = -eye / np.linalg.norm(eye)
    r = np.cross(f, [0.0, 0.0, 1.0])
    r /= np.linalg.norm(r)
    M = np.eye(4)
    M[:3, 0], M[:3, 1], M[:3, 2], M[:3, 3] = r, np.cross(f, r), f, eye
    return M


def scene(V, S, dev):
    """(depth [V,S,S] fp32, mask uint8, ixt [V,3,3], c2w [V,4,4] float64 numpy) of the unit sphere, ray-cast in float64 on the device."""
    eyes = [(3.0 * math.cos(a), 3.0 * math.sin(a), z) for a, z in zip(np.linspace(0, 2 * math.pi, V, endpoint=False), [0.4, 1.5, -0.8, 2.0] * V)]
    c2w = np.stack([look_at(e) for e in eyes])
    K = np.zeros((V, 3, 3))
    K[:, 0, 0] = K[:, 1, 1] = 1.2 * S
    K[:, 0, 2] = K[:, 1, 2] = S / 2
    K[:, 2, 2] = 1.0
    M = torch.from_numpy(c2w).to(dev)
    px = (torch.arange(S, device=dev, dtype=torch.float64) + 0.5 - S / 2) / (1.2 * S)
    dirs = torch.stack([px[None, :].expand(S, S), px[:, None].expand(S, S), torch.ones(S, S, device=dev, dtype=torch.float64)], -1)
    dirs = torch.einsum("vij,yxj->vyxi", M[:, :3, :3], dirs)
    o = M[:, None, None, :3, 3]
    a, b = (dirs * dirs).sum(-1), (dirs * o).sum(-1)
    disc = b * b - a * ((o * o).sum(-1) - 1.0)
    s = (-b - disc.clamp_min(0).sqrt()) / a
    hit = (disc >= 0) & (s > 0)
    return torch.where(hit, s, torch.zeros_like(s)).float().contiguous(), hit.to(torch.uint8).contiguous(), K, c2w


# ---- the same computation in torch operators ----------------------------------------------------------------------------------

def backproject_torch(depth, mask, k, pose):
    V, H, W = depth.shape
    ok = (mask != 0) & torch.isfinite(depth) & (depth > 0)
    pixel = ok.reshape(-1).nonzero().reshape(-1)
    d = depth.reshape(-1)[pixel]
    v, y, x = pixel // (H * W), (pixel // W) % H, pixel % W
    kv, R = k[v], pose.reshape(V, 4, 4)[v]
    a, b = (x.float() + 0.5 - kv[:, 2]) / kv[:, 0], (y.float() + 0.5 - kv[:, 3]) / kv[:, 1]
    px, py = a * d, b * d
    pts = torch.stack([((R[:, i, 0] * px + R[:, i, 1] * py) + R[:, i, 2] * d) + R[:, i, 3] for i in range(3)], 1)
    return pts, pixel


def thin_torch(points, voxel):
    lo = points.min(0).values
    cell = torch.floor((points - lo) / voxel).long()
    R = cell.max(0).values + 1
    word = (cell[:, 2] * R[1] + cell[:, 1]) * R[0] + cell[:, 0]
    uniq, inv = torch.unique(word, return_inverse=True)
    first = torch.full((uniq.shape[0],), points.shape[0], dtype=torch.long, device=points.device)
    first.scatter_reduce_(0, inv, torch.arange(points.shape[0], device=points.device), "amin")
    kept = first.sort().values
    return points[kept], kept


def observe_torch(P, depth, mask, k, w2c, tau):
    V, H, W = depth.shape
    ok = (mask != 0) & torch.isfinite(depth) & (depth > 0)
    seen = torch.zeros(P.shape[0], dtype=torch.int64, device=P.device)
    for v in range(V):
        Wm = w2c[v].reshape(4, 4)
        q = [((Wm[i, 0] * P[:, 0] + Wm[i, 1] * P[:, 1]) + Wm[i, 2] * P[:, 2]) + Wm[i, 3] for i in range(3)]
        zc = q[2]
        u, w = (q[0] * k[v, 0]) / zc + k[v, 2], (q[1] * k[v, 1]) / zc + k[v, 3]
        inside = (zc > 0) & (u >= 0) & (u < W) & (w >= 0) & (w < H)
        col, row = torch.where(inside, u.floor(), 0).long(), torch.where(inside, w.floor(), 0).long()
        d, on = depth[v, row, col], ok[v, row, col]
        obs = inside & torch.where(on, zc <= d + tau, torch.ones_like(on))
        seen |= obs.long() << v
    return seen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="8 views at 64 x 64, 2 x 10^4 samples, one step (the test suite's run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("depthsurface_bench: needs an MI355X")
    from lara_amd import depthsurface, meshmetrics
    dev = torch.device("cuda:0")
    V, S = 8, 64 if a.quick else 512
    sizes = (20000,) if a.quick else (100000, 1000000)
    steps, warmup = (1, 1) if a.quick else (a.steps, a.warmup)
    n_lat, n_lon = (64, 128) if a.quick else (374, 746)
    voxel, tau = 2.0 / 256 * (512 / S), 0.02
    depth, mask, K, c2w = scene(V, S, dev)
    views = (depth, mask, K, c2w)
    rate = copy_rate(dev, (1 << 26) if a.quick else (1 << 30))
    k_np, pose_np = depthsurface.cameras(K, c2w)
    _, w2c_np = depthsurface.cameras(K, c2w, invert=True)
    k, pose, w2c = (torch.from_numpy(x).to(dev) for x in (k_np, pose_np, w2c_np))

    G, Gn, pixel = depthsurface.backproject(*views, normals="depth")
    Gt, Gtn, kept = depthsurface.thin(G, Gn, voxel)
    n_raw, n_thin = int(G.shape[0]), int(Gt.shape[0])
    res = {"views": V, "image": S, "voxel": voxel, "tau": tau, "steps": steps, "warmup": warmup, "copy_rate_GBps": rate / 1e9,
           "n_gt_raw": n_raw, "n_gt": n_thin, "sizes": []}
    hip = {"backproject": timed(lambda: depthsurface.backproject(*views, normals="depth"), steps, warmup),
           "backproject_points_only": timed(lambda: depthsurface.backproject(*views), steps, warmup),
           "thin": timed(lambda: depthsurface.thin(G, Gn, voxel), steps, warmup)}
    tor = {"backproject_points_only": timed(lambda: backproject_torch(depth, mask, k, pose), steps, warmup),
           "thin": timed(lambda: thin_torch(G, voxel), steps, warmup)}
    tp, tpix = backproject_torch(depth, mask, k, pose)
    tk = thin_torch(G, voxel)[1]
    agrees = bool(torch.equal(tpix, pixel.long())) and bool(torch.allclose(tp, G, rtol=0, atol=1e-5)) and bool(torch.equal(tk, kept.long()))
    bp_bytes = V * S * S * 5 * 3 + n_raw * 28          # (the depth normals read the four neighbours: counted as two more passes)
    res["backproject_MB"], res["backproject_fraction_of_copy_rate"] = bp_bytes / 1e6, bp_bytes / (hip["backproject"] * 1e-3) / rate
    res["gt_stages_hip_ms"], res["gt_stages_torch_ms"] = hip, tor

    Vm, Fm, Vp = sphere_pair(n_lat, n_lon, dev)
    for n in sizes:
        P, Pn, _ = meshmetrics.sample_surface(Vp, Fm, n, seed=0)
        seen = depthsurface.observe(P, *views, tau)
        seen_t = observe_torch(P, depth, mask, k, w2c, tau)
        differ = float((seen != seen_t).float().mean())          # (fp32 both, but torch contracts nothing either: expected 0)
        d_p, i_p = meshmetrics.nearest(P, Gt)
        d_g, i_g = meshmetrics.nearest(Gt, P)
        keep = (seen != 0).to(torch.uint8)
        rows = torch.empty(2 * depthsurface.ROW, dtype=torch.float64, device=dev)
        thr = depthsurface.host_array("f", list(meshmetrics.THRESHOLDS))

        def reduce_both():
            depthsurface._reduce(dev, d_p, i_p, n_thin, keep, Pn, Gtn, thr, 3, rows[:depthsurface.ROW])
            depthsurface._reduce(dev, d_g, i_g, n, None, Gtn, Pn, thr, 3, rows[depthsurface.ROW:])

        def reduce_torch():
            kp = keep.bool()
            dd = d_p.double()
            out = [kp.sum(), dd[kp].sum(), (dd * dd)[kp].sum(), (Pn.double() * Gtn.double()[i_p.long()]).sum(1).abs()[kp].sum()]
            out += [(kp & (d_p <= t)).sum() for t in meshmetrics.THRESHOLDS]
            dg = d_g.double()
            out += [dg.sum(), (dg * dg).sum(), (Gtn.double() * Pn.double()[i_g.long()]).sum(1).abs().sum()]
            return torch.stack([o.double() for o in out + [(d_g <= t).sum() for t in meshmetrics.THRESHOLDS]])

        whole = lambda: depthsurface.depth_scores((P, Pn), *views, voxel=voxel, tau=tau)

        def whole_torch():
            g, _ = backproject_torch(depth, mask, k, pose)
            g, _ = thin_torch(g, voxel)
            observe_torch(P, depth, mask, k, w2c, tau)
            meshmetrics.nearest(P, g), meshmetrics.nearest(g, P)
            return reduce_torch().cpu()

        scores = whole()
        row = {"samples": n, "unobserved_share": scores["n_pred_unobserved"] / n, "accuracy": scores["accuracy"],
               "completeness": scores["completeness"], "fscore": scores["fscore"], "observe_differs_from_torch": differ,
               "hip_ms": {"observe": timed(lambda: depthsurface.observe(P, *views, tau), steps, warmup),
                          "nearest_both": timed(lambda: (meshmetrics.nearest(P, Gt), meshmetrics.nearest(Gt, P)), steps, warmup),
                          "reduce": timed(reduce_both, steps, warmup), "whole": timed(whole, steps, warmup)},
               "torch_ms": {"observe": timed(lambda: observe_torch(P, depth, mask, k, w2c, tau), steps, warmup),
                            "reduce": timed(reduce_torch, steps, warmup), "whole": timed(whole_torch, steps, warmup)}}
        ob_bytes = n * (12 + 8) + n * V * 5
        row["observe_MB"], row["observe_fraction_of_copy_rate"] = ob_bytes / 1e6, ob_bytes / (row["hip_ms"]["observe"] * 1e-3) / rate
        row["torch_agrees"] = agrees and differ < 1e-3
        res["sizes"].append(row)

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
