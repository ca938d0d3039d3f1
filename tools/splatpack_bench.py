"""Times `lara_amd.splatpack` on one MI355X: HIP events after warm-up, windows of at least 0.1 s, at 524 288 surfels (the headline
cloud) and 8 388 608 (a densified one), SH degrees 1 and 3.  In the same process, alternating over ``--rounds`` rounds (each round
times every variant once, in turn; min, median and max over the rounds are reported):

  * ``pack``: the whole route through the module -- bounds, Morton keys, ``torch.sort``, the host read of the dropped count, the
    allocations, encode;
  * ``encode``: the encode entry alone into preallocated outputs, with the order made beforehand;
  * ``unpack``: the decode entry alone into preallocated outputs;
  * ``splat_encode``: the ``.splat`` encode entry alone into preallocated rows;
  * ``torch_pack``: the same pack in torch operators, written below (masks, ``amin`` / ``amax`` over padded chunks, double arithmetic);
  * the device-to-device copy rate, as the neighbouring tools measure it (bytes read + written per second), and the share of it
    ``encode`` and ``unpack`` reach over their algorithmic bytes (every fp32 word of the cloud and every byte of the packed arrays
    once, the order's 8 bytes per row).

Beside them, at 524 288 surfels only: the sizes of the three files and the wall time of ``write_ply``, ``write_compressed_ply`` and
``write_splat`` into a temporary directory (one run each: no spread).  Nothing is gated.

``--resources`` (no GPU needed): the compiler's VGPR, SGPR, LDS and scratch figures of every kernel of csrc/splatpack.hip, from
hipcc's -Rpass-analysis=kernel-resource-usage, printed and merged into ``--out``.
    python tools/splatpack_bench.py [--quick] [--rounds 5] [--out profiles/splatpack_bench.json] [--resources]"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import splatrefine_bench as B  # noqa: E402
from tools.meshsimplify_bench import copy_rate  # noqa: E402

THICKNESS = 1e-3
C0 = 0.28209479177387814


def workload(P, degree, dev):
    """A cloud with the decoder's statistics (tests/splatio_cases.py), every row valid."""
    n = (degree + 1) ** 2
    g = torch.Generator(device=dev).manual_seed(degree)
    r = lambda *s: torch.randn(*s, generator=g, device=dev)
    return [torch.rand(P, 3, generator=g, device=dev) - 0.5, r(P, n, 3) * 0.5, r(P, 1) - 2.2, r(P, 2) * 0.3 - 5.0, r(P, 4)]


def _quantise(x, bits):
    m = float((1 << bits) - 1)
    return torch.floor(x * m + 0.5).clamp_(0.0, m).long()


def torch_pack(ts, s2):
    """(chunks, words, sh, order) in torch operators: the formulas of csrc/lara_splatpack.h in double."""
    c, shs, op, sc, rot = ts
    P, n = c.shape[0], shs.shape[1]
    dev = c.device
    ok = torch.isfinite(c).all(1) & torch.isfinite(shs).flatten(1).all(1) & torch.isfinite(op[:, 0]) & torch.isfinite(sc).all(1) & torch.isfinite(rot).all(1)
    ok &= rot.double().square().sum(1) > 0
    cv = c + 0.0
    inf = torch.tensor(float("inf"), device=dev)
    lo, hi = torch.where(ok[:, None], cv, inf).amin(0).double(), torch.where(ok[:, None], cv, -inf).amax(0).double()
    q = torch.floor((cv.double() - lo) / (hi - lo) * 1024.0).nan_to_num_(0.0).clamp_(0.0, 1023.0).long()
    code = torch.zeros(P, dtype=torch.int64, device=dev)
    for b in range(9, -1, -1):
        for a in range(3):
            code = (code << 1) | ((q[:, a] >> b) & 1)
    row = torch.arange(P, device=dev)
    keys = torch.where(ok, (code << 32) | row, (1 << 62) | row)
    order = (torch.sort(keys)[0] & 0x7FFFFFFF)[:int(ok.sum())]                 # (the host read of the count)
    P_out = order.shape[0]
    C = (P_out + 255) // 256
    k = (0.5 + C0 * shs[order, 0, :].double()).float() + 0.0
    third = torch.full((P_out, 1), s2, dtype=torch.float32, device=dev)
    v = torch.cat([cv[order], torch.cat([sc[order], third], 1).clamp(-20.0, 20.0) + 0.0, k], 1)        # [P_out, 9]
    pad = C * 256 - P_out
    vmin = torch.cat([v, v.new_full((pad, 9), float("inf"))]).view(C, 256, 9).amin(1)
    vmax = torch.cat([v, v.new_full((pad, 9), float("-inf"))]).view(C, 256, 9).amax(1)
    chunks = torch.stack([vmin[:, 0:3], vmax[:, 0:3], vmin[:, 3:6], vmax[:, 3:6], vmin[:, 6:9], vmax[:, 6:9]], 1).reshape(C, 18)
    ch = torch.arange(P_out, device=dev) // 256
    lo9, hi9 = vmin[ch].double(), vmax[ch].double()
    u = torch.where(hi9 == lo9, torch.zeros_like(lo9), (v.double() - lo9) / (hi9 - lo9))
    p11, p10, p8 = _quantise(u, 11), _quantise(u, 10), _quantise(u, 8)
    alpha = _quantise(1.0 / (1.0 + torch.exp(-op[order, 0].double())), 8)
    qn = rot[order].double()
    qn = qn / qn.square().sum(1, keepdim=True).sqrt()
    L = qn.abs().argmax(1)
    qn = torch.where(qn.gather(1, L[:, None]) < 0, -qn, qn)
    others = torch.tensor([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]], device=dev)[L]
    pr = _quantise(qn.gather(1, others) * 0.70710678118654752 + 0.5, 10)
    words = torch.stack([p11[:, 0] << 21 | p10[:, 1] << 11 | p11[:, 2], L << 30 | pr[:, 0] << 20 | pr[:, 1] << 10 | pr[:, 2],
                         p11[:, 3] << 21 | p10[:, 4] << 11 | p11[:, 5], p8[:, 6] << 24 | p8[:, 7] << 16 | p8[:, 8] << 8 | alpha], 1)
    words = torch.where(words >= 1 << 31, words - (1 << 32), words).int()          # (the uint32 words, held as int32)
    rest = shs[order, 1:, :].transpose(1, 2).reshape(P_out, 3 * (n - 1)).double()
    sh = torch.floor((rest / 8.0 + 0.5) * 256.0).clamp_(0.0, 255.0).to(torch.uint8)
    return chunks, words, sh, order


def rows(P, degree, dev, rounds, rate):
    from lara_amd import splatpack as sp
    from lara_amd._native import host_array
    ts = workload(P, degree, dev)
    packed = sp.pack(ts, THICKNESS)
    P_out, W = packed.n_surfels, sp.sh_width(degree)
    plan_c, ins = sp._plan_row(sp.plan(THICKNESS)), host_array("p", ts)
    chunks, words, sh = (torch.empty_like(t) for t in (packed.chunks, packed.words, packed.sh))
    decoded = [torch.empty_like(t) for t in ts]
    outs = host_array("p", decoded)
    valid, _, _ = sp.bounds(ts)
    sorder = sp.order_of(sp.importance_keys(ts, valid, THICKNESS), 0)
    splat = torch.empty(P_out, 32, dtype=torch.uint8, device=dev)
    s2 = float(sp.plan(THICKNESS)[0])
    variants = {
        "pack_ms": lambda: sp.pack(ts, THICKNESS),
        "encode_ms": lambda: sp._call_on("lara_splatpack_encode", dev, plan_c, degree, P, P_out, ins, packed.order, chunks, words, sh),
        "unpack_ms": lambda: sp._call_on("lara_splatpack_decode", dev, degree, P_out, packed.chunks, packed.words, packed.sh, outs),
        "splat_encode_ms": lambda: sp._call_on("lara_splatpack_splat_encode", dev, plan_c, degree, P, P_out, ins, sorder, splat),
        "torch_pack_ms": lambda: torch_pack(ts, s2),
    }
    times, calls = {k: [] for k in variants}, {}
    for _ in range(rounds):
        for k, fn in variants.items():                   # alternating: every variant once per round
            ms, calls[k] = B.windowed(fn)
            times[k].append(ms)
    cloud_bytes = 4 * sum(t.shape[1:].numel() for t in ts) * P_out
    packed_bytes = 16 * P_out + W * P_out + 72 * ((P_out + 255) // 256)
    nbytes = {"encode": cloud_bytes + packed_bytes + 8 * P_out, "unpack": cloud_bytes + packed_bytes}
    out = {"P": P, "sh_degree": degree, "P_out": P_out, "rounds": rounds, "calls_in_window": calls, **{k: B.spread(v) for k, v in times.items()},
           "cloud_bytes": cloud_bytes, "packed_bytes": packed_bytes, "splat_bytes": 32 * P_out}
    for k, nb in nbytes.items():
        out[k + "_GBps"] = nb / (out[k + "_ms"]["median"] * 1e-3) / 1e9
        out[k + "_fraction_of_copy_rate"] = out[k + "_GBps"] * 1e9 / rate
    out["torch_over_pack"] = out["torch_pack_ms"]["median"] / out["pack_ms"]["median"]
    t = torch_pack(ts, s2)
    same = [bool(torch.equal(t[3], packed.order)), float((t[1] == packed.words).float().mean()) if t[1].shape == packed.words.shape else 0.0,
            bool(torch.equal(t[2], packed.sh))]
    out["torch_pack_agrees"] = {"order": same[0], "share_of_equal_words": same[1], "sh": same[2]}
    return out


def files(P, degree, dev):
    """Sizes and wall times of the three writers, one run each, into a temporary directory."""
    from lara_amd import splatio, splatpack as sp
    cloud = splatio.SurfelCloud(*workload(P, degree, dev))
    out = {"P": P, "sh_degree": degree}
    with tempfile.TemporaryDirectory() as tmp:
        for name, fn in (("write_ply", lambda p: splatio.write_ply(p, cloud, THICKNESS)),
                         ("write_compressed_ply", lambda p: sp.write_compressed_ply(p, cloud, THICKNESS)),
                         ("write_splat", lambda p: sp.write_splat(p, cloud, THICKNESS))):
            path = os.path.join(tmp, name)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            nbytes = fn(path)
            out[name] = {"bytes": nbytes, "wall_s": time.perf_counter() - t0}
            os.remove(path)
    return out


def kernel_resources():
    """{kernel: {"VGPRs", "SGPRs", "scratch_bytes_per_lane", "LDS_bytes_per_block", "occupancy_waves_per_SIMD"}} of the unit, from the compiler."""
    csrc = os.path.join(ROOT, "lara_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    run = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-ffp-contract=off",
                          "-Rpass-analysis=kernel-resource-usage", "-c", "splatpack.hip", "-o", os.devnull], cwd=csrc, capture_output=True, text=True)
    if run.returncode != 0:
        raise SystemExit(run.stderr[-2000:])
    keys = {"VGPRs": "VGPRs", "TotalSGPRs": "SGPRs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane", "LDS Size [bytes/block]": "LDS_bytes_per_block",
            "Occupancy [waves/SIMD]": "occupancy_waves_per_SIMD"}
    out, name = {}, None
    for line in run.stderr.splitlines():
        m = re.search(r"remark: (?:\s*)([^:]+): (\S+) \[-Rpass", line)
        if m is None:
            continue
        if m.group(1).strip() == "Function Name":
            d = subprocess.run(["c++filt", m.group(2)], capture_output=True, text=True).stdout.strip() or m.group(2)
            name = re.sub(r"\(anonymous namespace\)::|\(.*$|^void ", "", d)
            out[name] = {}
        elif name is not None and m.group(1).strip() in keys:
            out[name][keys[m.group(1).strip()]] = int(m.group(2))
    return {k: v for k, v in out.items() if k.startswith("sp_")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="65 536 surfels only, short windows")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--resources", action="store_true", help="only the compiler's figures per kernel (no GPU), merged into --out")
    a = ap.parse_args()
    if a.resources:
        run = {}
        if a.out and os.path.exists(a.out):
            with open(a.out) as f:
                run = json.load(f)
        run["compiler_resources_gfx950"] = kernel_resources()
        print(json.dumps(run["compiler_resources_gfx950"]))
    else:
        if not torch.cuda.is_available():
            raise SystemExit("splatpack_bench: needs an MI355X")
        dev = torch.device("cuda:0")
        if a.quick:
            B.WINDOW_S = 0.005
        sizes = (1 << 16,) if a.quick else (1 << 19, 1 << 23)
        rate = copy_rate(dev, (1 << 26) if a.quick else (1 << 30))
        run = {"copy_rate_GBps": rate / 1e9, "window_s": B.WINDOW_S, "thickness": THICKNESS,
               "rows": [rows(P, d, dev, a.rounds, rate) for P in sizes for d in (1, 3)],
               "files": [files(sizes[0], d, dev) for d in (1, 3)],
               "not_measured": "the arrays of 524 288 surfels (46 and 122 MB of fp32 words) fit the 256 MiB cache, so those rows say nothing about HBM: "
                               "the 8 388 608-surfel rows do; clouds with dropped rows, SH degrees 0 and 2, .splat decode, the keys and "
                               "bounds kernels on their own, torch.sort's share of pack, counters of the memory system, file writes at "
                               "8 388 608 surfels, any viewer's load time; pack allocates its outputs and reads one count on the host, the "
                               "torch pack does the same"}

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
        with open(a.out, "w") as f:
            json.dump(run, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
