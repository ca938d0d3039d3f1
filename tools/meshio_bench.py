"""Times `lara_amd.meshio.write_mesh` against the unchanged host writer `lara_amd.mesh.write_obj` on one MI355X, in the same run, on
the mesh of tools/meshsimplify_bench.py: the UV sphere of 278 260 vertices and 556 516 triangles (the size of bench.py's mesh_eval
mesh) with per-vertex colours.

Whole calls are wall time (a device synchronise in front, the file closed at the end), the median of `--steps` calls after `--warmup`;
the device stages are HIP events recorded inside the call (lengths / scan + host read / emit, or pack / host read; then the
device-to-host copy into the pinned buffer), averaged over the same calls; the file write is the wall time of one `f.write` of the
same bytes; the emit and pack kernels are also timed alone (HIP events over `--steps` launches) and their bytes (every input and
output once) set against the device's copy rate measured here.  `read_obj` against `read_ply` of the files just written, once each.
Nothing is read from outside the repository.
    python tools/meshio_bench.py [--steps 10] [--warmup 2] [--quick] [--out profiles/meshio_bench.json]
Prints one JSON line, then the README table."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.meshmetrics_bench import sphere_pair, timed  # noqa: E402
from tools.meshsimplify_bench import copy_rate  # noqa: E402


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def whole_call(meshio, path, V, F, C, steps, warmup):
    """(median wall ms, {stage: mean ms}) of write_mesh(path, V, F, C)."""
    walls, acc = [], {}
    for i in range(warmup + steps):
        marks = []
        ms = wall(lambda: meshio.write_mesh(path, V, F, C, _marks=marks))
        torch.cuda.synchronize()
        if i >= warmup:
            walls.append(ms)
            for (_, e0), (name, e1) in zip(marks[:-1], marks[1:]):
                acc[name] = acc.get(name, 0.0) + e0.elapsed_time(e1) / steps
    return statistics.median(walls), min(walls), max(walls), acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="a small sphere, one step")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("meshio_bench: needs an MI355X")
    from lara_amd import _native, mesh, meshio
    dev = torch.device("cuda:0")
    n_lat, n_lon = (64, 128) if a.quick else (374, 746)
    steps, warmup = (1, 1) if a.quick else (a.steps, a.warmup)
    V, F, _ = sphere_pair(n_lat, n_lon, dev)
    C = (0.5 * V + 0.5).contiguous()
    Nv, T = int(V.shape[0]), int(F.shape[0])
    rate = copy_rate(dev, (1 << 26) if a.quick else (1 << 30))
    res = {"Nv": Nv, "T": T, "steps": steps, "warmup": warmup, "copy_rate_GBps": rate / 1e9}
    tmp = tempfile.mkdtemp()
    host_obj, dev_obj, dev_ply = (os.path.join(tmp, n) for n in ("host.obj", "device.obj", "device.ply"))

    # the baseline, in the same run: the unchanged host writer
    base = [wall(lambda: mesh.write_obj(host_obj, V, F, C)) for _ in range(1 if a.quick else 3)]
    res["write_obj_ms"], res["write_obj_ms_all"] = statistics.median(base), base

    for name, path in (("obj", dev_obj), ("ply", dev_ply)):
        med, lo, hi, stages = whole_call(meshio, path, V, F, C, steps, warmup)
        data = open(path, "rb").read()
        scratch = os.path.join(tmp, "scratch.bin")

        def write_once():
            with open(scratch, "wb") as f:
                f.write(data)
        writes = [wall(write_once) for _ in range(steps)]
        res[name] = {"whole_call_ms": med, "whole_call_ms_min": lo, "whole_call_ms_max": hi, "stage_ms": stages,
                     "file_write_ms": statistics.median(writes), "file_MB": len(data) / 1e6}
    res["obj"]["equals_write_obj"] = open(dev_obj, "rb").read() == open(host_obj, "rb").read()
    res["obj"]["speedup_over_write_obj"] = res["write_obj_ms"] / res["obj"]["whole_call_ms"]
    res["ply"]["speedup_over_write_obj"] = res["write_obj_ms"] / res["ply"]["whole_call_ms"]

    # the kernels alone, against the copy rate
    F32 = F.to(torch.int32)
    ws = torch.empty(_native.query("lara_meshio_obj_workspace_bytes", Nv, T) // 8, dtype=torch.int64, device=dev)
    nb = ws.numel() - 1
    _native.call("lara_meshio_obj_lengths", dev, Nv, V, C, T, F, 8, ws)
    totals = ws[:nb].clone()
    offsets = torch.cumsum(totals, 0) - totals
    out = torch.empty(int(totals.sum()), dtype=torch.uint8, device=dev)
    in_bytes = Nv * 24 + T * 24
    k = {}
    k["obj_lengths_ms"] = timed(lambda: _native.call("lara_meshio_obj_lengths", dev, Nv, V, C, T, F, 8, ws), steps * 5, warmup)
    k["obj_emit_ms"] = timed(lambda: _native.call("lara_meshio_obj_emit", dev, Nv, V, C, T, F, 8, offsets, out), steps * 5, warmup)
    k["obj_emit_fraction_of_copy_rate"] = (in_bytes + out.numel()) / (k["obj_emit_ms"] * 1e-3) / rate
    body = _native.query("lara_meshio_ply_body_bytes", Nv, T, 0, 1)
    pout = torch.empty(body, dtype=torch.uint8, device=dev)
    pws = torch.empty(1, dtype=torch.int64, device=dev)
    k["ply_pack_ms"] = timed(lambda: _native.call("lara_meshio_ply_pack", dev, Nv, V, None, C, T, F, 8, pout, pws), steps * 5, warmup)
    k["ply_pack_fraction_of_copy_rate"] = (in_bytes + body) / (k["ply_pack_ms"] * 1e-3) / rate
    k["ply_pack_int32_indices_ms"] = timed(lambda: _native.call("lara_meshio_ply_pack", dev, Nv, V, None, C, T, F32, 4, pout, pws),
                                           steps * 5, warmup)
    dst = torch.empty(out.numel(), dtype=torch.uint8, pin_memory=True)
    k["pinned_copy_obj_ms"] = timed(lambda: dst.copy_(out), steps, warmup)
    res["kernels"] = k

    # reading the files back
    res["read_obj_ms"] = wall(lambda: mesh.read_obj(dev_obj))
    res["read_ply_ms"] = wall(lambda: meshio.read_ply(dev_ply))

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
    o, p = res["obj"], res["ply"]
    st = lambda d: " / ".join(f"{n} {v:.3f}" for n, v in d["stage_ms"].items())
    print("| what | time | file |")
    print("|---|---|---|")
    print(f"| `write_obj` (host, unchanged) | {res['write_obj_ms']:.1f} ms | {os.path.getsize(host_obj) / 1e6:.1f} MB |")
    print(f"| `write_mesh` OBJ, whole call | **{o['whole_call_ms']:.2f} ms** ({o['speedup_over_write_obj']:.1f}x) | {o['file_MB']:.1f} MB |")
    print(f"| -- stages (ms): {st(o)} / file write {o['file_write_ms']:.3f} | | |")
    print(f"| `write_mesh` PLY, whole call | **{p['whole_call_ms']:.2f} ms** ({p['speedup_over_write_obj']:.1f}x) | {p['file_MB']:.1f} MB |")
    print(f"| -- stages (ms): {st(p)} / file write {p['file_write_ms']:.3f} | | |")
    print(f"| `read_obj` / `read_ply` | {res['read_obj_ms']:.1f} / {res['read_ply_ms']:.2f} ms | |")
    print(f"| emit / pack kernels alone | {k['obj_emit_ms']:.4f} / {k['ply_pack_ms']:.4f} ms = {100 * k['obj_emit_fraction_of_copy_rate']:.1f} % / "
          f"{100 * k['ply_pack_fraction_of_copy_rate']:.1f} % of the {rate / 1e12:.2f} TB/s copy rate | |")
    if o["whole_call_ms"] >= res["write_obj_ms"]:
        print("**THE DEVICE OBJ WRITER IS NOT FASTER THAN write_obj IN THIS RUN.**")


if __name__ == "__main__":
    main()
