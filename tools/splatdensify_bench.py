"""Times `lara_amd.splatdensify` on one MI355X: HIP events after warm-up, windows of at least 0.1 s, at 524 288 surfels (the headline
cloud), SH degrees 1 and 3, with statistics under which about 10 % of the surfels are cloned, 10 % split in two and 5 % pruned.  In
the same process, alternating over ``--rounds`` rounds (each round times every variant once, in turn; min, median and max over the
rounds are reported):

  * ``accumulate``: the statistics of one render call of 4 views;
  * ``decide``: the decide kernel, the three-launch scan and the pass that stores the exclusive offsets and the counts;
  * ``apply``: the two launches of the apply entry into preallocated outputs (no host read, no allocation);
  * ``densify``: the whole round through the module -- decide, the host read of the counts, the allocations, apply -- with the noise
    made beforehand;
  * ``torch``: the same round in torch operators, written below: the rules as boolean masks, then boolean index and ``cat`` over the
    15 tensors (``repeat_interleave`` for the children, quaternion to matrix for their centres);
  * the device-to-device copy rate, as the neighbouring tools measure it (bytes read + written per second), and the share of it
    ``apply`` reaches over its algorithmic bytes: per output word of a parameter three words written, and read one word (clones and
    children) or three (kept rows), plus 5 bytes written and read per output row (row_source, row_child) and 5 read per source row.

``--resources`` (no GPU needed): the compiler's VGPR, SGPR, LDS and scratch figures of every kernel of csrc/splatdensify.hip, from
hipcc's -Rpass-analysis=kernel-resource-usage, printed and merged into ``--out``.
    python tools/splatdensify_bench.py [--quick] [--rounds 5] [--out profiles/splatdensify_bench.json] [--resources]"""
import argparse
import json
import os
import re
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import splatrefine_bench as B  # noqa: E402
from tools.meshsimplify_bench import copy_rate  # noqa: E402

VIEWS = 4
THRESHOLD, LOG_DENSE, LOGIT_MIN = 0.5, -5.0, -5.3


def workload(P, degree, dev):
    """The cloud with its moments, the statistics and one render call's gradient and radii: 5 % of the surfels below the opacity limit,
    20 % hot, half of those above the size limit."""
    n = (degree + 1) ** 2
    g = torch.Generator(device="cpu").manual_seed(degree)
    shapes = ((3,), (n, 3), (1,), (2,), (4,))
    params = [torch.randn(P, *s, generator=g) for s in shapes]
    u = torch.rand(P, generator=g)
    params[2] = torch.where(u < 0.05, -10.0, 0.0)[:, None].contiguous()
    params[3] = (torch.randn(P, 2, generator=g) * 0.3 + LOG_DENSE - 0.6).contiguous()
    params[3][:, 0] = torch.where(torch.rand(P, generator=g) < 0.5, LOG_DENSE + 1.0, LOG_DENSE - 1.0)
    hot = torch.rand(P, generator=g) < 0.2 / 0.95
    cloud = {"params": [t.to(dev) for t in params], "exp_avg": [(torch.randn_like(t) * 1e-3).to(dev) for t in params],
             "exp_avg_sq": [(torch.rand_like(t) * 1e-5).to(dev) for t in params],
             "grad_sum": hot.float().to(dev), "seen": torch.ones(P, dtype=torch.int32).to(dev),
             "max_radius": torch.randint(0, 30, (P,), generator=g, dtype=torch.int32).to(dev),
             "grad": (torch.randn(P, 3, generator=g) * 1e-3).to(dev),
             "radii": torch.randint(-2, 30, (VIEWS, P), generator=g, dtype=torch.int32).to(dev),
             "noise": torch.randn(P, 2, 2, generator=g).to(dev)}
    return cloud


def torch_round(w, row):
    """The round in torch operators: (params', exp_avg', exp_avg_sq')."""
    p, n = w["params"], int(row[6])
    op, sc = p[2][:, 0], p[3]
    avg = torch.where(w["seen"] > 0, w["grad_sum"] / w["seen"].clamp(min=1), torch.zeros_like(w["grad_sum"]))
    hot = avg >= row[0]
    smax = sc.max(1).values
    gone = (op < row[2]) | ~torch.isfinite(op) | ~torch.isfinite(sc).all(1)
    split = hot & (smax > row[1]) & ~gone
    clone = hot & (smax <= row[1]) & ~gone
    survive = ~gone & ~split
    q = torch.nn.functional.normalize(p[4][split].double())
    qw, qx, qy, qz = q.unbind(1)
    r0 = torch.stack([1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy + qw * qz), 2 * (qx * qz - qw * qy)], 1)
    r1 = torch.stack([2 * (qx * qy - qw * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz + qw * qx)], 1)
    uv = torch.exp(sc[split].double())[:, None, :] * w["noise"][split].double()                      # [S, N, 2]
    centres = (p[0][split].double()[:, None, :] + r0[:, None, :] * uv[..., :1] + r1[:, None, :] * uv[..., 1:]).float().reshape(-1, 3)
    outs = []
    for group, ts in enumerate((p, w["exp_avg"], w["exp_avg_sq"])):
        new = []
        for f, t in enumerate(ts):
            if group:
                fresh = t.new_zeros((int(clone.sum()) + n * int(split.sum()),) + tuple(t.shape[1:]))
                new.append(torch.cat([t[survive], fresh]))
                continue
            children = centres if f == 0 else t[split].repeat_interleave(n, 0)
            if f == 3:
                children = children - float(row[5])
            new.append(torch.cat([t[survive], t[clone], children]))
        outs.append(new)
    return outs


def rows(P, degree, dev, rounds, rate):
    from lara_amd import _native, splatdensify as D
    from lara_amd._native import host_array
    w = workload(P, degree, dev)
    row = D.plan(THRESHOLD, 1.0, 1.0, 0.005)
    row[1], row[2] = LOG_DENSE, LOGIT_MIN
    stats = D.DensifyStats(P, dev)
    stats.grad_sum, stats.seen, stats.max_radius = w["grad_sum"], w["seen"], w["max_radius"]
    scratch = D.DensifyStats(P, dev)
    action, offset, counts = D.decide(w["params"], stats, row)
    p2, m2, v2, source, child, five = D.apply(w["params"], w["exp_avg"], w["exp_avg_sq"], action, offset, counts, row, noise=w["noise"])
    ws = torch.empty(_native.query("lara_splatdensify_workspace_bytes", P), dtype=torch.uint8, device=dev)
    plan_c, ins, outs = host_array("d", [float(x) for x in row]), host_array("p", w["params"] + w["exp_avg"] + w["exp_avg_sq"]), host_array("p", p2 + m2 + v2)
    survivors, P_out = five["kept"] + five["cloned"], five["P_out"]
    variants = {
        "accumulate_ms": lambda: scratch.accumulate(w["grad"], w["radii"]),
        "decide_ms": lambda: _native.call_on("lara_splatdensify_decide", dev, plan_c, P, w["params"][2], w["params"][3], stats.grad_sum,
                                             stats.seen, stats.max_radius, action, offset, counts, ws),
        "apply_ms": lambda: _native.call_on("lara_splatdensify_apply", dev, plan_c, degree, P, P_out, survivors, action, offset, w["noise"], ins,
                                            outs, source, child),
        "densify_ms": lambda: D.densify(w["params"], w["exp_avg"], w["exp_avg_sq"], stats, row, noise=w["noise"]),
        "torch_ms": lambda: torch_round(w, row),
    }
    times, calls = {k: [] for k in variants}, {}
    for _ in range(rounds):
        for k, fn in variants.items():                   # alternating: every variant once per round
            ms, calls[k] = B.windowed(fn)
            times[k].append(ms)
    words_in = sum(t.shape[1:].numel() for t in w["params"])
    nbytes = 4 * words_in * (3 * P_out + 3 * survivors + (P_out - survivors)) + 10 * P_out + 5 * P
    out = {"P": P, "sh_degree": degree, "counts": five, "rounds": rounds, "calls_in_window": calls, **{k: B.spread(ts) for k, ts in times.items()},
           "apply_bytes": nbytes, "apply_GBps": nbytes / (B.spread(times["apply_ms"])["median"] * 1e-3) / 1e9}
    out["apply_fraction_of_copy_rate"] = out["apply_GBps"] * 1e9 / rate
    out["torch_over_densify"] = out["torch_ms"]["median"] / out["densify_ms"]["median"]
    t2 = torch_round(w, row)
    out["torch_round_rows_equal"] = all(a.shape == b.shape for a, b in zip(t2[0] + t2[1] + t2[2], p2 + m2 + v2))
    return out


def kernel_resources():
    """{kernel: {"VGPRs", "SGPRs", "scratch_bytes_per_lane", "LDS_bytes_per_block", "occupancy_waves_per_SIMD"}} of the unit, from the compiler."""
    csrc = os.path.join(ROOT, "lara_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    run = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-ffp-contract=off",
                          "-Rpass-analysis=kernel-resource-usage", "-c", "splatdensify.hip", "-o", os.devnull], cwd=csrc, capture_output=True, text=True)
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
    return {k: v for k, v in out.items() if k.startswith(("sd_", "mm_scan"))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="65 536 surfels, short windows")
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
            raise SystemExit("splatdensify_bench: needs an MI355X")
        dev = torch.device("cuda:0")
        if a.quick:
            B.WINDOW_S = 0.005
        P = (1 << 16) if a.quick else (1 << 19)
        rate = copy_rate(dev, (1 << 26) if a.quick else (1 << 30))
        run = {"copy_rate_GBps": rate / 1e9, "window_s": B.WINDOW_S, "views_of_the_accumulated_call": VIEWS,
               "rows": [rows(P, d, dev, a.rounds, rate) for d in (1, 3)],
               "not_measured": "a densification round inside refine at 512 x 512 (its share of a step), the capped (max_surfels) round, "
                               "other mixes of actions, counters of the memory system; the torch round allocates as it goes, as the "
                               "3DGS code does, and `densify` allocates its outputs too"}

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
