"""Measures the image half of the loader, each leg on the machine where it can run.  Nothing is gated.

``workers --reference <LaRa checkout>`` (CPU; needs the reference's dataset class, so the build machine only): items per second of
the class on ``make_store(res=512)`` through a real DataLoader with ``collate_cpu`` and ``skip_cpu_rays``, plain and under
``raw_views``, with 1 and with 8 workers, and the bytes of images, normals and masks one item ships.  The figures are those of that
machine's CPU (its core count is recorded), not of a GPU host's.

``device`` (one MI355X; no reference: synthetic raw batches at B = 4, V = 8, 512 x 512): host-to-device time of the raw batch against
the float batch (pinned and pageable host memory), ``finish_images`` with HIP events after warm-up in windows of at least 0.1 s, its
share of a device-to-device copy rate measured in the same process over its algorithmic bytes (7 in, 25 out per pixel), and the
same arithmetic written in torch operators on the device as context.  One process run gives one figure per row; ``--out FILE`` appends
the run to the file and rewrites the spread (min and max over the runs): run it at least twice.
    python tools/loader_bench.py workers --reference <LaRa checkout> [--items 40] [--out profiles/batchfinish_bench.json]
    python tools/loader_bench.py device [--quick] [--out profiles/batchfinish_bench.json]"""
import argparse
import json
import math
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOW_S = 0.1
IMAGE_KEYS = ("tar_rgb", "tar_msk", "tar_nrm", "tar_nrm_u8")


def rounded(x):
    if isinstance(x, float):
        return float(f"{x:.6g}")
    if isinstance(x, dict):
        return {k: rounded(v) for k, v in x.items()}
    if isinstance(x, list):
        return [rounded(v) for v in x]
    return x


def merge(path, key, run, spread_keys=None):
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    if spread_keys is None:
        doc[key] = run
    else:
        runs = doc.setdefault(key, {"runs": []})["runs"]
        runs.append(run)
        doc[key]["process_runs"] = len(runs)
        doc[key]["spread"] = {k: [min(r[k] for r in runs), max(r[k] for r in runs)] for k in spread_keys}
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


# ------------------------------------------------------------------------------------------------------------------ the worker leg

class Repeat(torch.utils.data.Dataset):
    """``n`` items of ``ds``, round and round (module-level: workers unpickle it under spawn)."""

    def __init__(self, ds, n):
        self.ds, self.n = ds, n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return self.ds[i % len(self.ds)]


def workers_leg(a):
    from lara_amd import dataset
    from tests.helpers_store import make_store
    ref_root = os.path.abspath(a.reference)
    store = make_store(seed=5, res=512)
    h5 = types.ModuleType("h5py")
    h5.File = lambda path, mode="r": store
    sys.modules["h5py"] = h5
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    pkg = types.ModuleType("dataLoader")                 # a bare package: only the loader module and dataLoader.utils are executed
    pkg.__path__ = [os.path.join(ref_root, "dataLoader")]
    sys.modules["dataLoader"] = pkg
    sys.path.insert(0, ref_root)
    import dataLoader.gobjverse as ref
    dataset.skip_cpu_rays(ref)
    torch.set_num_threads(1)

    def make(raw):
        cfg = types.SimpleNamespace(data_root="mem", split="train", img_size=(512, 512), n_group=4, n_scenes=100, load_normal=True)
        ds = ref.gobjverse(cfg)
        return dataset.raw_views(ds) if raw else ds
    run = {"machine": "the build machine's CPU (no GPU host was measured)", "cpu_count": os.cpu_count(), "views": 8, "resolution": 512,
           "items_timed": a.items, "batch_size": 4, "collate": "lara_amd.dataset.collate_cpu, skip_cpu_rays applied", "rows": []}
    for raw in (False, True):
        ds = make(raw)
        item = ds[0]
        nbytes = sum(np.asarray(item[k]).nbytes for k in IMAGE_KEYS if k in item)
        t = time.perf_counter()
        for i in range(4):
            ds[i]
        inline = (time.perf_counter() - t) / 4
        row = {"dataset": "raw_views(gobjverse)" if raw else "gobjverse", "image_bytes_per_item": nbytes, "getitem_ms_in_process": inline * 1e3}
        for nw in (1, 8):
            loader = torch.utils.data.DataLoader(Repeat(ds, a.items + 8 * nw), batch_size=4, num_workers=nw, collate_fn=dataset.collate_cpu)
            it = iter(loader)
            for _ in range(2 * nw):                      # the workers are up and their queues are full
                next(it)
            t = time.perf_counter()
            n = 0
            for batch in it:
                n += batch["tar_rgb"].shape[0]
            row[f"items_per_s_{nw}_workers"] = n / (time.perf_counter() - t)
            row[f"items_{nw}_workers"] = n
        run["rows"].append(row)
    run = rounded(run)
    print(json.dumps(run))
    if a.out:
        merge(a.out, "worker_leg", run)


# ------------------------------------------------------------------------------------------------------------------ the device leg

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


def windowed(fn):
    """ms per call over a window of at least WINDOW_S, after warm-up; (ms, calls in the window)."""
    once = timed(fn, 2, 2)
    steps = max(3, int(math.ceil(1.2 * WINDOW_S * 1e3 / max(once, 1e-3))))
    return timed(fn, steps, 1), steps


def torch_finish(rgba, bg, n_u8, rot):
    """The arithmetic of include/lara_batchfinish.h in torch operators on the device (fp32; the matmul sums in torch's order)."""
    f = rgba.float() / 255.0
    a = f[..., 3:4]
    rgb = f[..., :3] * a + bg[:, :, None, None, :] * (1.0 - a)
    msk = (rgba[..., 3] > 0).to(torch.uint8)
    n = n_u8.float() / 255.0 * 2.0 - 1.0
    B, V, H, W, _ = n.shape
    nrm = torch.einsum("bvhwk,bjk->bvhwj", n, rot).permute(0, 2, 1, 3, 4).reshape(B, H, V * W, 3)
    return rgb, msk, nrm


def device_leg(a):
    global WINDOW_S
    if not torch.cuda.is_available():
        raise SystemExit("loader_bench device: needs an MI355X")
    from lara_amd import dataset
    dev = torch.device("cuda:0")
    B, V, H, W = (1, 2, 64, 64) if a.quick else (4, 8, 512, 512)
    if a.quick:
        WINDOW_S = 0.005
    g = torch.Generator().manual_seed(0)
    host = {"rgba": torch.randint(0, 256, (B, V, H, W, 4), dtype=torch.uint8, generator=g),
            "n_u8": torch.randint(0, 256, (B, V, H, W, 3), dtype=torch.uint8, generator=g)}
    bg = torch.rand(B, V, 3, generator=g).to(dev)
    rot = torch.linalg.qr(torch.randn(B, 3, 3, generator=g))[0].contiguous().to(dev)
    rgba, n_u8 = host["rgba"].to(dev), host["n_u8"].to(dev)
    ref = dataset.finish_images(rgba, bg, n_u8, rot)
    alt = torch_finish(rgba, bg, n_u8, rot)
    float_host = {"tar_rgb": ref[0].cpu(), "tar_msk": ref[1].cpu(), "tar_nrm": ref[2].cpu()}
    N = B * V * H * W
    nbytes = N * (7 + 25) + 4 * (3 * B * V + 9 * B)
    run = {"B": B, "V": V, "H": H, "W": W, "window_s": WINDOW_S, "raw_bytes": sum(t.numel() * t.element_size() for t in host.values()),
           "float_bytes": sum(t.numel() * t.element_size() for t in float_host.values()), "algorithmic_bytes": nbytes}
    n_copy = 1 << (26 if a.quick else 30)
    src, dst = torch.empty(n_copy, dtype=torch.uint8, device=dev), torch.empty(n_copy, dtype=torch.uint8, device=dev)
    rate = 2.0 * n_copy / (timed(lambda: dst.copy_(src), 10, 2) * 1e-3)          # bytes read + written per second
    del src, dst
    run["copy_rate_GBps"] = rate / 1e9
    for kind in ("pinned", "pageable"):
        for name, tensors in (("raw", host), ("float", float_host)):
            src = [t.pin_memory() if kind == "pinned" else t for t in tensors.values()]
            dst = [torch.empty_like(t, device=dev) for t in src]
            ms, _ = windowed(lambda: [d.copy_(s, non_blocking=True) for d, s in zip(dst, src)])
            run[f"h2d_{name}_{kind}_ms"] = ms
            del src, dst
    outs = [torch.empty_like(t) for t in ref]
    ms, calls = windowed(lambda: dataset._finish_into(rgba, bg, n_u8, rot, *outs))
    run.update({"finish_ms": ms, "calls_in_window": calls, "finish_GBps": nbytes / (ms * 1e-3) / 1e9,
                "fraction_of_copy_rate": nbytes / (ms * 1e-3) / rate})
    run["finish_images_with_allocation_ms"], _ = windowed(lambda: dataset.finish_images(rgba, bg, n_u8, rot))
    run["finish_rgb_only_ms"], _ = windowed(lambda: dataset._finish_into(rgba, bg, None, None, outs[0], outs[1], None))
    run["torch_operators_ms"], run["torch_calls_in_window"] = windowed(lambda: torch_finish(rgba, bg, n_u8, rot))
    run["torch_over_kernel"] = run["torch_operators_ms"] / ms
    run["msk_equals_torch_operators"] = bool(torch.equal(ref[1], alt[1]))
    run["rgb_words_differing_from_torch_operators"] = int((ref[0].view(torch.int32) != alt[0].view(torch.int32)).sum())
    run["max_abs_rgb_difference_to_torch_operators"] = float((ref[0] - alt[0]).abs().max())
    run["max_abs_nrm_difference_to_torch_operators"] = float((ref[2] - alt[2]).abs().max())
    run = rounded(run)
    print(json.dumps(run))
    if a.out:
        merge(a.out, "device_leg", run, ("finish_ms", "finish_images_with_allocation_ms", "finish_rgb_only_ms", "fraction_of_copy_rate",
                                         "torch_operators_ms", "copy_rate_GBps", "h2d_raw_pinned_ms", "h2d_float_pinned_ms",
                                         "h2d_raw_pageable_ms", "h2d_float_pageable_ms"))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="leg", required=True)
    w = sub.add_parser("workers")
    w.add_argument("--reference", required=True, help="path of a LaRa checkout")
    w.add_argument("--items", type=int, default=40)
    w.add_argument("--out", default=None)
    d = sub.add_parser("device")
    d.add_argument("--quick", action="store_true", help="a small batch, short windows")
    d.add_argument("--out", default=None)
    a = ap.parse_args()
    (workers_leg if a.leg == "workers" else device_leg)(a)


if __name__ == "__main__":
    main()
