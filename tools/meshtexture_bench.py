"""Times `lara_amd.meshtexture` on one MI355X: HIP events after warm-up, on the UV sphere of about 557 k triangles of the neighbouring
benches (tools/meshbvh_bench.py, tools/meshwind_bench.py) simplified at 4 voxels of 2 / 256, baked at S = 8 from 16 views of 512 x 512
that `meshray` renders of the full sphere under an analytic colour field.  Nothing baked a texture in this package before, so no time
is gated and no row has a baseline.

  * per stage: the texel kernel, the hierarchy build, `meshray.visibility` on the anchors, the bake kernel (both blends, with and
    without the mask), `bake` as a whole, `render_textured` of one 512 x 512 view and its sample kernel alone, the files;
  * the traffic each kernel must move and the rate that gives, beside what bounds it;
  * the compiler's register, LDS and scratch report of the three kernels (one device-only compile of csrc/meshtexture.hip;
    `--no-compiler-report` skips it);
  * the quality: RMSE of the rendered textured mesh against the field at the hit points, beside the vertex colours'.

Every figure is the mean of --steps runs in ONE process run: no spread is measured.  Nothing is read from outside the repository.
    python tools/meshtexture_bench.py [--steps 10] [--warmup 2] [--quick] [--out profiles/meshtexture_bench.json]"""
import argparse
import json
import math
import os
import re
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.meshmetrics_bench import sphere_pair, timed  # noqa: E402

WAVE = 20.0


def field(p):
    return 0.5 + 0.5 * torch.sin(WAVE * p.double() + torch.tensor([0.0, 1.0, 2.0], dtype=torch.float64, device=p.device))


def orbit(n, res, radius=3.0):
    ixt, c2w = [], []
    for i in range(n):
        a = 0.3 + 2 * math.pi * i / n
        eye = torch.tensor([radius * math.cos(a), radius * math.sin(a), radius * 0.4 * (-1) ** i], dtype=torch.float64)
        z = -eye / eye.norm()
        x = torch.linalg.cross(z, torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64))
        x = x / x.norm()
        M = torch.eye(4, dtype=torch.float64)
        M[:3, 0], M[:3, 1], M[:3, 2], M[:3, 3] = x, torch.linalg.cross(z, x), z, eye
        c2w.append(M)
        f = (1.25 if i % 2 == 0 else 1.4) * res
        ixt.append(torch.tensor([[f, 0, res / 2], [0, f, res / 2], [0, 0, 1]], dtype=torch.float64))
    return torch.stack(ixt).float(), torch.stack(c2w).float()


def compiler_report():
    """{kernel: {VGPRs, SGPRs, scratch bytes per lane, LDS bytes, waves per SIMD}} from hipcc's resource remarks, or a reason."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "lara_amd", "csrc", "meshtexture.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only",
               "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(tmp, "unit.o")]
        try:
            text = subprocess.run(cmd, capture_output=True, text=True, timeout=300).stderr
        except (OSError, subprocess.TimeoutExpired) as e:
            return {"unavailable": str(e)}
    out, name = {}, None
    keys = {"VGPRs": "vgprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
            "Occupancy [waves/SIMD]": "waves_per_simd", "LDS Size [bytes/block]": "lds_bytes"}
    for line in text.splitlines():
        m = re.search(r"Function Name: \S*?(mt_\w+_kernel)", line)
        if m:
            name = m.group(1)
            out[name] = {}
        for k, short in keys.items():
            m = re.search(r"remark:\s+" + re.escape(k) + r": (\d+)", line)
            if m and name:
                out[name][short] = int(m.group(1))
    return out or {"unavailable": "no remarks"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="a small sphere, 4 views of 128 x 128, one step")
    ap.add_argument("--no-compiler-report", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("meshtexture_bench: needs an MI355X")
    from lara_amd import meshbvh, meshray, meshsimplify, meshtexture as MT
    dev = torch.device("cuda:0")
    n_lat, n_lon = (64, 128) if a.quick else (374, 746)
    n_views, res, S = (4, 128, 8) if a.quick else (16, 512, 8)
    steps, warmup = (1, 1) if a.quick else (a.steps, a.warmup)
    V0, F0, _ = sphere_pair(n_lat, n_lon, dev)
    full = meshbvh.TriangleBVH(V0, F0)
    ixt, c2w = orbit(n_views, res)
    # the source views: the full sphere through meshray, coloured by the field at the hit points
    o, d = meshray.pixel_rays(ixt, c2w, res, res, dev)
    t, face = meshray.raycast(full, o.view(-1, 3), d.view(-1, 3))
    hit = (o.view(-1, 3).double() + t.double()[:, None] * d.view(-1, 3).double())
    images = torch.where((face >= 0)[:, None], field(hit), torch.full_like(hit, 0.25)).float().view(n_views, res, res, 3).contiguous()
    voxel = 4 * 2 / 256
    V, F, C, _ = meshsimplify.simplify_vertex_clustering(V0, F0, field(V0).float(), voxel)
    T = int(F.shape[0])
    L = MT.atlas(T, S)
    n_tex = L[2] * L[3]
    resd = {"Nv_full": int(V0.shape[0]), "T_full": int(F0.shape[0]), "simplify_voxel": voxel, "Nv": int(V.shape[0]), "T": T, "patch": S,
            "atlas": [L[2], L[3]], "texels": n_tex, "views": n_views, "source": [res, res], "steps": steps, "warmup": warmup, "one_run": True}
    k, w2c, eyes = MT._cameras(ixt, c2w, dev)
    bvh = meshbvh.TriangleBVH(V, F)
    fc, pt, an = MT.texels(L, V, F)
    mask = meshray.visibility(bvh, an.view(-1, 3), eyes, faces=fc.view(-1)).view(fc.shape)
    ms = resd["ms"] = {}
    ms["texels_kernel"] = timed(lambda: MT.texels(L, V, F), steps, warmup)
    ms["bvh_build"] = timed(lambda: meshbvh.TriangleBVH(V, F), steps, warmup)
    ms["visibility"] = timed(lambda: meshray.visibility(bvh, an.view(-1, 3), eyes, faces=fc.view(-1)), steps, warmup)
    for blend in ("weighted", "best"):
        ms[f"bake_kernel_{blend}"] = timed(lambda: MT.bake_texels(L, V, F, fc, pt, an, images, k, w2c, eyes, mask, blend=blend), steps, warmup)
    ms["bake_kernel_weighted_no_mask"] = timed(lambda: MT.bake_texels(L, V, F, fc, pt, an, images, k, w2c, eyes, None), steps, warmup)
    ms["bake_whole"] = timed(lambda: MT.bake(V, F, images, ixt, c2w, patch=S, vertex_colors=C), steps, warmup)
    tex = MT.bake(V, F, images, ixt, c2w, patch=S, vertex_colors=C, bvh=bvh)
    resd["coverage"] = tex.coverage
    held_ixt, held_c2w = orbit(7, res, radius=2.6)
    held_ixt, held_c2w = held_ixt[3:4], held_c2w[3:4]
    ms["render_textured_one_view"] = timed(lambda: MT.render_textured(bvh, tex, held_ixt, held_c2w, res, res), steps, warmup)
    ho, hd = meshray.pixel_rays(held_ixt, held_c2w, res, res, dev)
    ht, hf, hb = meshray.raycast(bvh, ho.view(-1, 3), hd.view(-1, 3), return_bary=True)
    ms["sample_kernel"] = timed(lambda: tex.sample(hf, hb), steps, warmup)
    # traffic: what each kernel has to read and write at least once
    texel_bytes = n_tex * (4 + 12 + 12)
    bake_bytes = n_tex * (4 + 12 + 12 + 8 + 4 + 4 + 4)
    resd["GBps"] = {"texels_kernel": texel_bytes / ms["texels_kernel"] / 1e6, "bake_kernel_weighted": bake_bytes / ms["bake_kernel_weighted"] / 1e6,
                    "sample_kernel": hf.shape[0] * (4 + 12 + 12) / ms["sample_kernel"] / 1e6}
    accepted = tex.view.sum().item() / max(1, int((fc >= 0).sum()))
    resd["mean_views_accepted_per_owned_texel"] = accepted
    # what binds: stated from the figures above only -- no hardware counters are collected here
    resd["what_binds"] = {
        "bake_whole": "meshray.visibility on the anchors (every texel x every eye): %.0f %% of the time; the three kernels of this module "
                      "together are below 1 %%" % (100 * ms["visibility"] / ms["bake_whole"]),
        "texels_kernel": "writes 28 bytes per texel and gathers 9 floats from a vertex table that fits in L2; at this atlas it lasts tens "
                         "of microseconds, where launch ramp and tail count as much as the memory rate shown",
        "bake_kernel": "one thread per texel at 4 waves per SIMD (99 VGPRs); per texel and unmasked view three dot products, two "
                       "divisions and a square root in double come before 12 gathered source floats; the mask saves the work of hidden "
                       "views (compare the no-mask row); its compulsory traffic runs below the HBM rate, so it is not bandwidth-bound",
        "sample_kernel": "28 bytes per sample and four scattered 4-byte reads of an atlas that fits in L2; tens of microseconds per "
                         "512 x 512 view, beside the 1.2 ms of the ray cast that feeds it"}
    # quality on the held-out view
    hitm = hf >= 0
    Fl = F.long()
    tri = V[Fl[hf[hitm].long()]].double()
    P = (hb[hitm].double()[:, :, None] * tri).sum(1)
    truth = field(P)
    got = tex.sample(hf, hb)[hitm].double()
    vcol = (hb[hitm].double()[:, :, None] * C[Fl[hf[hitm].long()]].double()).sum(1)
    rm = lambda x: float(((x - truth) ** 2).mean().sqrt())
    resd["rmse_textured"], resd["rmse_vertex_colours"] = rm(got), rm(vcol)
    resd["rmse_ratio"] = resd["rmse_textured"] / resd["rmse_vertex_colours"]
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        MT.write_textured_obj(os.path.join(tmp, "mesh.obj"), V, F, tex)
        ms["write_textured_obj_host"] = (time.perf_counter() - t0) * 1e3
        resd["file_bytes"] = {e: os.path.getsize(os.path.join(tmp, "mesh." + e)) for e in ("obj", "mtl", "png")}
    if not a.no_compiler_report:
        resd["compiler_report_gfx950"] = compiler_report()

    def rounded(x):
        if isinstance(x, float):
            return float(f"{x:.6g}")
        if isinstance(x, dict):
            return {k: rounded(v) for k, v in x.items()}
        return x
    line = json.dumps(rounded(resd))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
