"""Times `lara_amd.splatxform.transform` on one MI355X: HIP events after warm-up, windows of at least 0.1 s, at 524 288 surfels (the
headline cloud) and at 8 388 608 (past the 256 MiB Infinity Cache), SH degrees 1 and 3.  Nothing in this package moved a cloud
before, so no time is gated and there is no parent figure.  In the same process:

  * the device-to-device copy rate, as the neighbouring tools measure it (bytes read + written per second);
  * the share of that rate the kernel reaches over its algorithmic bytes, 2 * 4 * (10 + 3 n) * P (every word read once and written
    once);
  * the in-place call (``out=cloud``), the call that allocates its result, and the call that is handed the 4x4 instead of the plan
    and builds the plan first (float64 numpy and a few hundred polynomial terms on the host);
  * the same map written in torch operators (float64, ``einsum`` for the bands): the only baseline there is.

One process run gives one figure per row.  ``--out FILE`` appends the run to the file's list of runs and rewrites the summary
(min and max of every time over the runs): run it at least twice for a spread.
    python tools/splatxform_bench.py [--quick] [--out profiles/splatxform_bench.json]"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.meshmetrics_bench import timed  # noqa: E402
from tools.meshsimplify_bench import copy_rate  # noqa: E402

WINDOW_S = 0.1


def windowed(fn):
    """ms per call over a window of at least WINDOW_S, after warm-up; (ms, calls in the window)."""
    once = timed(fn, 2, 2)
    steps = max(3, int(math.ceil(1.2 * WINDOW_S * 1e3 / max(once, 1e-3))))
    return timed(fn, steps, 1), steps


def torch_map(cloud, plan):
    """The per-surfel map in torch operators, float64, one rounding per output."""
    dev = cloud.device
    p = torch.from_numpy(plan).to(dev)
    A, t, r, log_s = p[0:9].view(3, 3), p[9:12], p[12:16], p[16]
    L = torch.stack([torch.stack([r[0], -r[1], -r[2], -r[3]]), torch.stack([r[1], r[0], -r[3], r[2]]),
                     torch.stack([r[2], r[3], r[0], -r[1]]), torch.stack([r[3], -r[2], r[1], r[0]])])
    blocks = (p[17:26].view(3, 3), p[26:51].view(5, 5), p[51:100].view(7, 7))
    shs = cloud.shs.double()
    parts = [cloud.shs[:, :1]]
    for l in range(1, cloud.sh_degree + 1):
        parts.append(torch.einsum("ij,pjc->pic", blocks[l - 1], shs[:, l * l:(l + 1) ** 2]).float())
    return ((cloud.centers.double() @ A.T + t).float(), torch.cat(parts, dim=1), cloud.opacity.clone(),
            (cloud.scales.double() + log_s).float(), (cloud.rotations.double() @ L.T).float())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="65 536 surfels, short windows")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("splatxform_bench: needs an MI355X")
    global WINDOW_S
    from lara_amd import splatio, splatxform
    dev = torch.device("cuda:0")
    if a.quick:
        WINDOW_S = 0.005
    sizes = (1 << 16,) if a.quick else (1 << 19, 1 << 23)
    rate = copy_rate(dev, (1 << 26) if a.quick else (1 << 30))
    T = np.eye(4)
    th, axis = math.radians(111.0), np.array([-2.0, 1.0, 0.5]) / np.linalg.norm([-2.0, 1.0, 0.5])
    K = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    T[:3, :3] = 1.7 * (np.eye(3) + math.sin(th) * K + (1.0 - math.cos(th)) * (K @ K))
    T[:3, 3] = (0.3, -0.2, 0.1)
    plan = splatxform.similarity(T)
    run = {"copy_rate_GBps": rate / 1e9, "window_s": WINDOW_S, "rows": []}
    g = torch.Generator(device="cpu").manual_seed(0)
    for P in sizes:
        for degree in (1, 3):
            n = (degree + 1) ** 2
            cloud = splatio.SurfelCloud(*(torch.randn(P, *shape, generator=g).to(dev) for shape in ((3,), (n, 3), (1,), (2,), (4,))))
            out = splatio.SurfelCloud(*(torch.empty_like(t) for t in cloud.render_args()))
            scratch = splatio.SurfelCloud(*(t.clone() for t in cloud.render_args()))
            nbytes = 2 * 4 * (10 + 3 * n) * P
            ms, calls = windowed(lambda: splatxform.transform(cloud, plan, out=out))
            ms_in, _ = windowed(lambda: splatxform.transform(scratch, plan, out=scratch))
            ms_new, _ = windowed(lambda: splatxform.transform(cloud, plan))
            ms_planned, _ = windowed(lambda: splatxform.transform(cloud, T, out=out))
            ms_torch, calls_torch = windowed(lambda: torch_map(cloud, plan))
            ref = torch_map(cloud, plan)
            got = splatxform.transform(cloud, T)
            diff = max(float((x - y).abs().max()) for x, y in zip(got.render_args(), ref))
            run["rows"].append({"P": P, "sh_degree": degree, "bytes": nbytes, "transform_ms": ms, "calls_in_window": calls,
                                "GBps": nbytes / (ms * 1e-3) / 1e9, "fraction_of_copy_rate": nbytes / (ms * 1e-3) / rate,
                                "in_place_ms": ms_in, "with_allocation_ms": ms_new, "with_planning_ms": ms_planned,
                                "torch_float64_ms": ms_torch,
                                "torch_calls_in_window": calls_torch, "torch_over_kernel": ms_torch / ms,
                                "max_abs_difference_to_torch": diff})
            del cloud, out, scratch, ref, got
            torch.cuda.empty_cache()

    def rounded(x):
        if isinstance(x, float):
            return float(f"{x:.6g}")
        if isinstance(x, dict):
            return {k: rounded(v) for k, v in x.items()}
        if isinstance(x, list):
            return [rounded(v) for v in x]
        return x
    run = rounded(run)
    print(json.dumps(run))
    if a.out:
        doc = {"runs": []}
        if os.path.exists(a.out):
            with open(a.out) as f:
                doc = json.load(f)
        doc["runs"].append(run)
        keys = ("transform_ms", "in_place_ms", "with_allocation_ms", "with_planning_ms", "torch_float64_ms", "fraction_of_copy_rate")
        doc["process_runs"] = len(doc["runs"])
        doc["spread"] = [{"P": row["P"], "sh_degree": row["sh_degree"],
                          **{k: [min(r["rows"][i][k] for r in doc["runs"]), max(r["rows"][i][k] for r in doc["runs"])] for k in keys}}
                         for i, row in enumerate(run["rows"])]
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
