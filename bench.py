#!/usr/bin/env python
"""bench.py -- novel-view frames/sec @512x512 (4-view in, 2DGS fwd+bwd) on MI355X.

One *step* (default `--step pipeline`) = one pass of the WHOLE data-dependent LaRa training step on the hot path (every row
of SURVEY.md section 8a, composed as lightning/network.py:455-532 composes them, `lara_amd.pipeline.LaRaPipeline`), on
every rank for its B = 4 scenes:
    1. the volume transformer's forward (`encoder_train.VolTransformer`, rows A1-A3) on the image-feature volume;
    2. `Decoder.forward_coarse` (plain torch, outside section 8a) -> the scenes' P = 524 288 Gaussians each, centres, masks;
    3. per scene 8 coarse views (4 input + 4 novel, dataLoader/gobjverse.py:46-47) at 512x512 through ONE multi-view
       rasteriser call + ONE fused post-processing launch (`Renderer.render_views`);
    4. LaRa's fine stage (network.py:502-525): `_check_mask` (in training a mask keeping > 50 % is thinned to about half at
       random), the point sampler on the 4 input views, `Decoder.forward_fine`, 8 fine views over the masked subset;
    5. the loss of lightning/loss.py minus MS-SSIM (package absent) on the reference's output dictionary;
    6. ONE backward through all of it -- every view's rasteriser backward, the sampler, the decoders, then the transformer's
       backward, whose encoder is one autograd node per block, so that under DistributedDataParallel (N > 1,
       train_lightning.py:68-81) each 25 MB bucket's RCCL all-reduce starts while the earlier blocks' backward still runs.
       That all-reduce is the path's only exchange step; the raster is per view and NOT sharded (BASELINE.json north_star)
       -> per-scene data parallel, weak scaling;
    7. the parameter update: `clip_grad_norm_(0.5)` (train_lightning.py:75) + AdamW over the reference's two parameter groups
       (system.py:78-106), every step.  `--lr` defaults to 0: all of the update's kernels run and every parameter's version
       counter advances -- the HIP modules then re-derive their bf16 / transposed operands in the next step's forward, as they
       must in training -- while the values stay, so that all K timed steps see the same synthetic workload.  (Rounds 1-3
       timed steps 1-6 only and so kept those operand caches warm; `--no-optimizer` reproduces that.)
A *frame* is one rasteriser forward + backward; a step holds 64 of them.  `value` = frames of all
ranks / max-over-ranks wall time of the timed steps, with the collated batch (cameras, images, rays) and the image-feature
volume already resident in HBM.  Data is synthetic (no dataset / checkpoint in this environment): random-init network of the
reference's architecture = SURVEY.md section 8d's "init" regime (mean opacity 0.10, every pixel walks ~1.5 k surfels).
`--step train` is round 2's definition (encoder and raster on INDEPENDENT synthetic tensors, no decoder / sampler /
forward_fine / loss), carried on the default line as `independent_tensors_step`; `--step raster` times the raster alone.

`python bench.py --gpus N` with N > 1 launches its own N ranks (torch.distributed.run, one per GPU, backend nccl =
RCCL) when it is not already running under a launcher; under `python -m torch.distributed.run ... bench.py --gpus N`
it reads RANK / LOCAL_RANK / WORLD_SIZE from the environment.

The scenes of a step are independent after the decoder, so scene i runs on HIP stream i % `--streams` (default 2).

A plain run (`python bench.py --gpus 1 --steps K --warmup W`) sets up, runs the W warm-up steps, times the K steps, writes
the last timed step's outputs when `--dump-outputs DIR` is given, and prints the line: `metric`, `value`, `unit`,
`higher_is_better`, `dtype`, `ms_per_step` (wall time of one timed step) and `config`.  Everything else is measured only
with `--full`.

Extra objects on the JSON line with `--full`: "memory_per_rank" (any N); on rank 0 with N = 1 "stages" (where the step's
time goes: forward stages + backward on one stream, the library's kernels grouped by stage), "roofline" (dominant kernel
on the seeded synthetic scenes of SURVEY 8d, HIP-event timed, algorithmic bytes of section 8d; `bound` says what binds it; `valu_useful_frac` = useful FMA lane-ops /
issued lane-slots), "cpu_baseline" (the CPU oracle of the raster AND the fixture-pinned fp32 restatement of the
reference's encoder, both on this box's host cores; `parity_vs_oracle` with the committed fp64 arbitration),
"independent_tensors_step", "raster_only", "single_stream", "forward_only", "mesh_eval" (configs[4]: 48 views @1024x1024 +
block-sparse TSDF fusion + marching cubes), "attention", "encoder", "encoder_train", "rays", "render_img", "point_feats",
"coarse_decoder", "fine_decoder", "fine_stage".
"""
import argparse
import contextlib
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6300 achievable
MEASURED_COPY_GBS = 5400.0   # what a device-to-device copy sustains on this part (`roofline.measured_copy_GBs`, 5.3-5.4 TB/s in every run)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scenes", type=int, default=4, help="scenes per rank per step (config 3: 4)")
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--grid", type=int, default=64, help="surfels = grid^3 * 2 (64 -> 524288)")
    ap.add_argument("--regime", default="init", choices=["init", "trained"])
    ap.add_argument("--step", default="pipeline", choices=["pipeline", "train", "raster"],
                    help="pipeline: the whole data-dependent LaRa step (lara_amd.pipeline: encoder -> coarse decoder -> coarse views -> "
                         "sampler -> forward_fine -> fine views -> loss -> one backward; DDP all-reduce when N > 1); train: round 2's "
                         "definition (encoder and raster on independent tensors, no decoder / sampler / forward_fine); raster: the raster alone")
    ap.add_argument("--fine-mask", default="reference", choices=["reference", "plain"],
                    help="pipeline step: `reference` applies Network._check_mask as a training step does (a mask keeping > 50 %% of the "
                         "Gaussians is thinned to about half at random, network.py:381-388); `plain` keeps every Gaussian above the "
                         "opacity threshold (what an eval step renders)")
    ap.add_argument("--dense-map-grads", action="store_true",
                    help="A/B only: a pass whose maps take no gradient hands the rasteriser seven planes of zeros (the behaviour up to "
                         "round 5) instead of None = the colour-only composite_bwd")
    ap.add_argument("--fine-rebins", action="store_true",
                    help="pipeline step: the fine pass scatters and sorts its own lists (rounds 1-5) instead of filtering the coarse pass's "
                         "(`rasterize_gaussians_views(..., subset_of=...)`, round 6); same results bit for bit")
    ap.add_argument("--no-fine", action="store_true", help="coarse views only (LaRa before train.start_fine)")
    ap.add_argument("--encoder-layers", type=int, default=12, help="transformer depth (configs/base.yaml:16: 12)")
    ap.add_argument("--raster-api", default="views", choices=["views", "loop"],
                    help="views: one multi-view call per scene and pass (lara_amd.rasterize_gaussians_views / Renderer.render_views, "
                         "opt-in, SURVEY.md section 8f-2); loop: one GaussianRasterizer call per view, as the reference's loop issues them")
    ap.add_argument("--streams", type=int, default=2,
                    help="HIP streams the independent scenes of a step are spread over (1 = the reference's sequential loop)")
    ap.add_argument("--ms-ssim", action="store_true",
                    help="add the reference's 0.5 (1 - MS_SSIM) term (loss.py:41-45) to the timed step's loss = its whole loss: "
                         "lara_amd.loss.ms_ssim_fused (HIP kernels, csrc/msssim.hip; the package the reference imports is absent: held to "
                         "the restatement).  Default: the step is timed WITHOUT it (the workload string says so; the definition of "
                         "rounds 1-4) and `step_with_ms_ssim` reports the step with it in the same run")
    ap.add_argument("--lr", type=float, default=0.0,
                    help="learning rate of the AdamW update inside the timed step (--step pipeline).  Default 0: every kernel of the "
                         "update runs and the parameters' version counters advance (the bf16 operand caches of the HIP modules are "
                         "rebuilt every step, as in training) while the values, and with them the synthetic workload, stay put")
    ap.add_argument("--accumulate", type=int, default=1,
                    help="--step pipeline: micro-batches per optimiser step.  2 = the reference's cadence (train_lightning.py:73 "
                         "accumulate_grad_batches=2: loss / 2, DDP `no_sync()` on the first micro-batch, all-reduce + clip + AdamW on the "
                         "second); 1 (default, the headline) reduces and updates on EVERY timed step -- the dearer definition")
    ap.add_argument("--no-optimizer", action="store_true", help="--step pipeline: forward + loss + backward only (rounds 1-3's step)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also measure everything else: the per-rank memory report, the step's stage breakdown, "
                         "the other step definitions, the raster legs, the roofline (with its own rocprofv3 passes), the side objects "
                         "and the CPU baselines (the --no-* options below trim that set).  Without it a run is the headline only: "
                         "set-up, warm-up, the timed steps, --dump-outputs, the JSON line")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-side-legs", action="store_true", help="skip the side objects (attention, encoder, rays, ...)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed (rank 0: the step's output maps, loss "
                         "terms and gradients) as DIR/<name>.npy, float32 (float64 where the tensor is), under 64 MB in all: an "
                         "array larger than its share is replaced by a fixed, seeded sample of its elements (flattened)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


def self_spawn(args):
    """`python bench.py --gpus N` (N > 1) outside a launcher: start N ranks, one per GPU, and relay rank 0's line."""
    import socket
    import subprocess
    backend = os.environ.get("LARA_BENCH_BACKEND", "nccl")
    if backend == "nccl" and os.environ.get("LARA_BENCH_PLUMBING", "0") != "1":
        have = torch.cuda.device_count() if torch.cuda.is_available() else 0
        if have < args.gpus:
            raise SystemExit(f"bench.py --gpus {args.gpus}: only {have} GPU(s) visible; RCCL wants one rank per device "
                             "(LARA_BENCH_BACKEND=gloo lets ranks share a device for plumbing tests)")
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: RCCL's intra-node transport needs it on this driver
    env.setdefault("OMP_NUM_THREADS", "8")
    raise SystemExit(subprocess.call(cmd, env=env))


def build_batch(args, device, rank):
    from lara_amd import cameras, synthetic, GaussianRasterizationSettings
    from lara_amd import dp
    scenes = []
    for seed in dp.scene_seeds(rank, args.scenes):
        sc = synthetic.make_scene(grid=args.grid, K=2, regime=args.regime, seed=seed, device=device)
        scenes.append({k: v.requires_grad_(True) for k, v in sc.items()})
    cams = cameras.make_cameras(cameras.turntable_c2w(args.views), args.res, args.res, 0.75, 0.75,
                                1.906 - 0.8, 1.906 + 0.8, device=device)
    # background: 1 for the input views, {0, 0.5, 1} for the novel ones (gobjverse.py:103-106)
    bgs = [1.0] * (args.views // 2) + [(0.0, 0.5, 1.0)[j % 3] for j in range(args.views - args.views // 2)]
    settings = []
    for cam, b in zip(cams, bgs):
        settings.append(GaussianRasterizationSettings(
            image_height=args.res, image_width=args.res, tanfovx=math.tan(cam.FoVx * 0.5),
            tanfovy=math.tan(cam.FoVy * 0.5), bg=torch.full((3,), b, device=device), scale_modifier=1.0,
            viewmatrix=cam.world_view_transform.contiguous(), projmatrix=cam.full_proj_transform.contiguous(),
            sh_degree=1, campos=cam.camera_center.contiguous(), prefiltered=False, debug=False))
    g = torch.Generator(device="cpu").manual_seed(7 + rank)
    gc = (torch.randn(3, args.res, args.res, generator=g) / (args.res * args.res)).to(device)
    ga = (torch.randn(7, args.res, args.res, generator=g) / (args.res * args.res) * 0.1).to(device)
    return scenes, settings, gc, ga


_streams = []
FINE_OPACITY = 0.005   # network.py:465: the fine stage keeps Gaussians with opacity > 0.005


def fine_subsets(scenes):
    """Per scene: row indices of the fine stage's subset (`masks = sigmoid(opacity) > 0.005`, network.py:464-465),
    computed once per batch like the reference does, as index tensors (a boolean mask index would synchronise the
    host on every use)."""
    with torch.no_grad():
        return [(torch.sigmoid(sc["opacity"].detach()).squeeze(-1) > FINE_OPACITY).nonzero().squeeze(-1) for sc in scenes]


def step(scenes, settings, gc, ga, n_streams=1, fine_idx=None, after=None, api="loop", capture=None):
    """All forwards of the batch, then one backward through every view (as loss.backward() does).
    Per scene: the coarse views (network.py:487-497) and, with `fine_idx`, the fine views over the masked subset with
    refined SH coefficients (network.py:508-525; the refinement itself -- `forward_fine` -- is a side leg, here the
    subset's coefficients are offset by a constant).  Activations and subset gathers are applied per view, as the
    reference's `render_img` / loop do.  Scenes are independent (the unit the north star data-parallelises over), so
    scene i is enqueued on HIP stream i % n_streams; autograd replays each view's backward on its forward's stream.
    `after(outs, grads)` names the roots of a second backward call that runs after the raster's (the encoder's output
    and its gradient).
    api = "views": the views of a scene and pass go through ONE multi-view call (one autograd node; activations and
    subset gathers once per scene, as `lara_amd.renderer.Renderer.render_views` does) instead of one call per view.
    `capture` (a dict): receives the rendered maps and the scenes' gradients (`--dump-outputs`)."""
    from lara_amd import GaussianRasterizer, rasterize_gaussians_views
    from lara_amd import rasterizer as _rz
    outs, grads = [], []
    cur = torch.cuda.current_stream()
    while len(_streams) < n_streams and n_streams > 1:
        _streams.append(torch.cuda.Stream())

    def render(rs, centers, shs, opacity, scales, rotations):
        # the reference's activations, applied per view (renderer_2dgs.py:181-189)
        means2D = torch.zeros_like(centers, requires_grad=True)
        color, radii, allmap = GaussianRasterizer(rs)(
            means3D=centers, means2D=means2D, shs=shs, opacities=torch.sigmoid(opacity), scales=torch.exp(scales),
            rotations=torch.nn.functional.normalize(rotations), cov3D_precomp=None)
        outs.extend((color, allmap) if ga is not None else (color,))
        grads.extend((gc, ga) if ga is not None else (gc,))

    nv = len(settings)
    gcs, gas = gc.expand(nv, *gc.shape), (ga.expand(nv, *ga.shape) if ga is not None else None)      # (ga None: no gradient on the maps)

    def render_views(centers, shs, opacity, scales, rotations):
        color, radii, allmap = rasterize_gaussians_views(
            settings, centers, torch.zeros_like(centers), torch.sigmoid(opacity), shs=shs, scales=torch.exp(scales),
            rotations=torch.nn.functional.normalize(rotations))
        outs.extend((color, allmap) if gas is not None else (color,))
        grads.extend((gcs, gas) if gas is not None else (gcs,))

    for i, sc in enumerate(scenes):
        side = _streams[i % n_streams] if n_streams > 1 else None
        if side is not None:
            side.wait_stream(cur)
        with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
            if api == "views":
                render_views(sc["centers"], sc["shs"], sc["opacity"], sc["scales"], sc["rotations"])
            else:
                for rs in settings:
                    render(rs, sc["centers"], sc["shs"], sc["opacity"], sc["scales"], sc["rotations"])
            if fine_idx is not None:
                idx = fine_idx[i]
                if api != "views":
                    centers_f = sc["centers"][idx]                # network.py:514
                    shs_f = sc["shs"][idx] + 0.01                 # network.py:518 (+ forward_fine's residual)
                if api == "views":
                    from lara_amd.fine import take_rows      # (the indices of a mask are unique: no sort in the backward)
                    render_views(take_rows(sc["centers"], idx), take_rows(sc["shs"], idx) + 0.01, take_rows(sc["opacity"], idx),
                                 take_rows(sc["scales"], idx), take_rows(sc["rotations"], idx))
                else:
                    for rs in settings:                           # network.py:524: subset gathers per view
                        render(rs, centers_f, shs_f, sc["opacity"][idx], sc["scales"][idx], sc["rotations"][idx])
    for side in _streams[:n_streams if n_streams > 1 else 0]:
        cur.wait_stream(side)
    torch.autograd.backward(outs, grads)
    for side in _streams[:n_streams if n_streams > 1 else 0]:
        cur.wait_stream(side)
    if after is not None:
        # the encoder's backward consumes what the raster's backward produces (through the decoder, in LaRa): it is
        # a second backward call, enqueued behind the scene streams' work, so that the two do not overlap on the device
        more_outs, more_grads = [], []
        after(more_outs, more_grads)
        torch.autograd.backward(more_outs, more_grads)
    if capture is not None:
        capture["raster_maps"] = [o.detach() for o in outs]
        capture["grad_surfels"] = [v.grad for sc in scenes for _, v in sorted(sc.items())]
    for sc in scenes:
        for v in sc.values():
            v.grad = None


def forward_only_leg(scenes, settings, args):
    """BASELINE.json configs[1] (inference): forward renders only, same scenes / views / streams."""
    from lara_amd import GaussianRasterizer
    cur = torch.cuda.current_stream()

    def fwd(n_streams=None):
        n_streams = args.streams if n_streams is None else n_streams
        with torch.no_grad():
            for i, sc in enumerate(scenes):
                side = _streams[i % n_streams] if n_streams > 1 and _streams else None
                if side is not None:
                    side.wait_stream(cur)
                with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
                    opac, scales = torch.sigmoid(sc["opacity"]), torch.exp(sc["scales"])
                    rots = torch.nn.functional.normalize(sc["rotations"])
                    for rs in settings:
                        GaussianRasterizer(rs)(means3D=sc["centers"], means2D=None, shs=sc["shs"], opacities=opac,
                                               scales=scales, rotations=rots, cov3D_precomp=None)
            for side in _streams[:n_streams if n_streams > 1 else 0]:
                cur.wait_stream(side)

    def fwd_views():   # the same renders through one multi-view call per scene
        from lara_amd import rasterize_gaussians_views
        with torch.no_grad():
            for i, sc in enumerate(scenes):
                side = _streams[i % args.streams] if args.streams > 1 and _streams else None
                if side is not None:
                    side.wait_stream(cur)
                with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
                    rasterize_gaussians_views(settings, sc["centers"], None, torch.sigmoid(sc["opacity"]), shs=sc["shs"],
                                              scales=torch.exp(sc["scales"]), rotations=torch.nn.functional.normalize(sc["rotations"]))
            for side in _streams[:args.streams if args.streams > 1 else 0]:
                cur.wait_stream(side)

    def rate(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        return round(len(scenes) * len(settings) * args.steps / (time.perf_counter() - t0), 1)

    return {"value": rate(fwd), "unit": "frames/s", "views_api": rate(fwd_views), "per_view_one_stream": rate(lambda: fwd(1)),
            "workload": "forward renders only (configs[1]: inference; forward-only calls of the library under no_grad), same scenes and "
                        "views; `value`: one operator call per view (the reference's loop) with the scenes dealt to the step's streams, "
                        "`per_view_one_stream`: the same on one stream (what evaluation.py:129 unchanged issues), `views_api`: one "
                        "multi-view call per scene"}


def mesh_eval_leg(args, device):
    """BASELINE.json configs[4] (eval_all.py / tools/meshExtractor.py:50-110): the mesh path's 48 views of one object at
    1024x1024, forward only, each batch of 8 fused into the TSDF volume on the device (the reference copies depth,
    alpha and colour of every view to the host for Open3D).  Trained-like scene (an opaque shell: there is a surface)."""
    from lara_amd import cameras, synthetic, GaussianRasterizationSettings, rasterize_gaussians_views
    from lara_amd.tsdf import TSDFVolume
    res, n_views, chunk, grid = 1024, 48, 8, 256
    sc = synthetic.make_scene(grid=args.grid, K=2, regime="trained", seed=123, device=device)
    cams = cameras.make_cameras(cameras.turntable_c2w(n_views), res, res, 0.75, 0.75, 1.906 - 0.8, 1.906 + 0.8, device=device)
    settings = [GaussianRasterizationSettings(
        image_height=res, image_width=res, tanfovx=math.tan(c.FoVx * 0.5), tanfovy=math.tan(c.FoVy * 0.5),
        bg=torch.ones(3, device=device), scale_modifier=1.0, viewmatrix=c.world_view_transform.contiguous(),
        projmatrix=c.full_proj_transform.contiguous(), sh_degree=1, campos=c.camera_center.contiguous(), prefiltered=False,
        debug=False) for c in cams]
    K = torch.tensor([[res / (2 * math.tan(c.FoVx / 2.0)), res / (2 * math.tan(c.FoVy / 2.0)), res / 2, res / 2] for c in cams],
                     device=device)
    ext = torch.stack([c.world_view_transform.T for c in cams]).contiguous()
    with torch.no_grad():
        opac, scales = torch.sigmoid(sc["opacity"]), torch.exp(sc["scales"])
        rots = torch.nn.functional.normalize(sc["rotations"])

    def run(fuse, fuse_events=None):
        vol = TSDFVolume((-1.0, -1.0, -1.0), 2.0 / grid, 0.08, grid, device=device) if fuse else None
        with torch.no_grad():
            for i in range(0, n_views, chunk):
                color, _, allmap = rasterize_gaussians_views(settings[i:i + chunk], sc["centers"], None, opac, shs=sc["shs"],
                                                             scales=scales, rotations=rots)
                if fuse:   # expected depth = ch0 / ch1 where the ray hit something (renderer_2dgs.py:226-233), else 0
                    if fuse_events is not None:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                    acc = allmap[:, 1]
                    depth = torch.where(acc < 0.08, torch.zeros_like(acc), allmap[:, 0] / acc.clamp_min(1e-8))
                    rgb8 = (color.clamp(0, 1).permute(0, 2, 3, 1) * 255).to(torch.uint8).float()
                    vol.integrate(depth, rgb8, K[i:i + chunk], ext[i:i + chunk], 10.0)
                    if fuse_events is not None:
                        e1.record()
                        fuse_events.append((e0, e1))
        return vol

    def timed(fuse):
        run(fuse)
        torch.cuda.synchronize()
        ev = [] if fuse else None
        t0 = time.perf_counter()
        for _ in range(2):
            vol = run(fuse, ev)
        torch.cuda.synchronize()
        # the fuse's share is what ITS kernels took on the device (HIP events around them), not the difference of two
        # separately timed runs (round 5 shipped a negative number that way)
        return (time.perf_counter() - t0) / 2, vol, (sum(a.elapsed_time(b) for a, b in ev) / 2e3 if fuse else 0.0)

    t_r, _, _ = timed(False)
    t_all, vol, t_fuse = timed(True)
    assert t_fuse > 0.0 and t_all > 0.0 and t_r > 0.0, (t_r, t_all, t_fuse)
    occupied = int((vol.weight > 0).sum())
    vol.extract_triangle_mesh()                 # warm-up (loads the case tables)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    verts, tris, cols = vol.extract_triangle_mesh()
    torch.cuda.synchronize()
    t_mesh = time.perf_counter() - t0
    return {"workload": f"one object: {n_views} views @{res}x{res} forward (multi-view calls of {chunk}), each batch fused into a "
                        f"{grid}^3 TSDF volume on the device (voxel 2/{grid}, trunc 0.08, alpha threshold 0.08; 16^3-voxel blocks touched "
                        f"by a view's depth samples, as Open3D's ScalableTSDFVolume), then marching cubes on the device "
                        f"(tools/meshExtractor.py:67-110)",
            "render_frames_per_s": round(n_views / t_r, 1), "ms_per_object_render": round(1e3 * t_r, 2),
            "ms_per_object_render_and_fuse": round(1e3 * t_all, 2), "tsdf_ms_per_object": round(1e3 * t_fuse, 2),
            "mesh_extract_ms": round(1e3 * t_mesh, 2), "mesh_vertices": int(verts.shape[0]), "mesh_triangles": int(tris.shape[0]),
            "voxels_observed": occupied, "blocks_allocated": int(vol.allocated.sum()), "blocks_total": int(vol.allocated.numel())}


def measure_roofline(scenes, settings, gc, ga, args):
    """Per-kernel HIP-event times over one step; returns (roofline dict, per-kernel table, D)."""
    from lara_amd import rasterizer
    # An event pair around a launch also measures the host: the start event runs at once and the device then waits for the
    # kernel to be enqueued.  One profiled step first (its first launches pay one-off host work: up to tens of ms were seen
    # on one launch), then the measured one; a launch that still sits beyond 3x its kernel's median is a host stall, not a
    # kernel time, and is left out of the average (`host_stalls` counts them; rocprofv3's averages, which only see the
    # device, are the cross-check: profiles/<tag>_kernel_stats.csv).
    rasterizer.profile_enable(True)
    step(scenes, settings, gc, ga)
    torch.cuda.synchronize()
    rasterizer.profile_collect()
    step(scenes, settings, gc, ga)
    torch.cuda.synchronize()
    rec = rasterizer.profile_collect()
    # the same step without a gradient on the seven maps (LaRa's fine pass: lightning/loss.py reads its image only): the
    # compositing backward's colour-only form
    step(scenes, settings, gc, None)
    torch.cuda.synchronize()
    rec_color = [ms for name, ms in rasterizer.profile_collect() if name == "composite_bwd_color"]
    rasterizer.profile_enable(False)
    by_name = {}
    for name, ms in rec:
        by_name.setdefault(name, []).append(ms)
    agg, stalls = {}, 0
    for name, v in by_name.items():
        med = sorted(v)[len(v) // 2]
        kept = [x for x in v if x <= 3.0 * med]
        stalls += len(v) - len(kept)
        agg[name] = [len(kept), sum(kept)]
    # D (pairs per frame) of one representative view
    from lara_amd import synthetic
    act = synthetic.activate({k: v.detach() for k, v in scenes[0].items()})
    r = rasterizer.forward_with_state(settings[0], act["means3D"], act["opacities"], shs=act["shs"],
                                      scales=act["scales"], rotations=act["rotations"])
    torch.cuda.synchronize()
    D = int(r["views"]["header"][0].item())
    P = scenes[0]["centers"].shape[0]
    HW = args.res * args.res
    # ALGORITHMIC bytes per launch: SURVEY.md section 8d's per-unit figures (forward 175 P + 120 D + 60 HW, backward
    # 248 P + 220 D + 100 HW per frame) split over the kernels that move them
    alg = {
        "preprocess_fwd": 88 * P + 87 * P,
        "tile_scan": 12 * (HW // 256),
        "scatter": 12 * D,
        "tile_sort": 24 * D + 8 * D,
        "composite_fwd": 76 * D + 60 * HW,
        "composite_bwd": 76 * D + 100 * HW + 144 * D,
        "preprocess_bwd": (88 + 72) * P + 88 * P,
    }
    table = {k: {"launches": n, "avg_us": 1e3 * t / n, "alg_bytes": alg.get(k, 0),
                 "alg_GBs": (alg.get(k, 0) / (1e-3 * t / n) / 1e9) if t > 0 else 0.0}
             for k, (n, t) in agg.items()}
    dom = max(table, key=lambda k: table[k]["avg_us"] * table[k]["launches"])
    t = table[dom]
    # Counter-derived figures need rocprofv3 passes of their own: `live_counters` runs three short ones as child processes (this
    # run's numbers); where that is not possible (no rocprofv3, a pass failed, LARA_BENCH_NO_LIVE_PMC=1) the summaries committed
    # under profiles/ (tools/gpu_profile.sh, tools/gpu_traffic.sh) are READ instead and the `*_source` fields say so.
    traffic, traffic_src, valu, valu_src, insts, insts_src = None, None, None, None, None, None
    live = None if os.environ.get("LARA_BENCH_NO_LIVE_PMC") == "1" else live_counters(dom, args)
    if live is not None:
        src = (f"measured in this run: rocprofv3 --kernel-trace --pmc, three child passes of the serialised raster step (one scene, "
               f"{live['launches']} launches of {dom} averaged)")
        # calibrated (profiles/r04a_traffic_calibration.json): gfx950's FETCH_SIZE tallies 128-byte requests at 64 bytes; unit KB
        traffic, traffic_src = int((2.0 * live["FETCH_SIZE"] + live["WRITE_SIZE"]) * 1024), src + "; bytes = 2 x FETCH_SIZE + WRITE_SIZE"
        valu, valu_src = round(4.0 * live["SQ_ACTIVE_INST_VALU"] / (1024.0 * live["GRBM_GUI_ACTIVE"] / 8.0), 4), src
        insts, insts_src = live["SQ_INSTS_VALU"], src
    elif args.grid == 64 and args.res == 512:
        # (same regime, and the per-view launches: `<tag>_views_pmc_summary.csv` holds the 8-view launches of a multi-view call)
        same = (lambda f: "trained" in os.path.basename(f)) if args.regime == "trained" else (lambda f: "trained" not in os.path.basename(f))
        tagged = lambda f: same(f) and "_views_" not in os.path.basename(f)
        traffic, traffic_src = _newest_profile("traffic_r*.json", lambda f: json.load(open(f))["bytes_per_launch"][dom]["total"], tagged)
        valu, valu_src = _newest_profile("r*pmc_summary.csv", lambda f: _valu_issue_frac(f, dom), tagged)
        insts, insts_src = _newest_profile("r*pmc_summary.csv", lambda f: _pmc_value(f, dom, "SQ_INSTS_VALU"), tagged)
    # what a plain device-to-device copy reaches on this box (read + write bytes / time): the achievable
    # HBM rate to hold beside the vendor peak (SURVEY.md section 8d asks for both)
    buf = torch.empty(2, 1 << 28, dtype=torch.uint8, device=scenes[0]["centers"].device)
    buf[1].copy_(buf[0])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        buf[1].copy_(buf[0])
    e1.record()
    torch.cuda.synchronize()
    copy_GBs = 5 * 2 * (1 << 28) / (e0.elapsed_time(e1) * 1e-3) / 1e9
    del buf
    # the whole frame against the byte model of SURVEY.md section 8d
    frame_bytes = (175 + 248) * P + (120 + 220) * D + 160 * HW
    frame_us = sum(v["avg_us"] for v in table.values())
    # `bound`: the composite kernels are VALU-issue bound in the init regime (SURVEY.md section 8d predicted an ALU
    # floor 4-7x above the HBM floor; PMC: profiles/*_pmc_summary.csv); `frac` stays the HBM-roofline fraction the
    # north star asks for, `valu_issue_frac` is the share of SIMD issue cycles spent on vector ALU instructions
    composite = dom.startswith("composite")
    roof = {"kernel": dom, "bound": "valu" if composite else "hbm", "achieved": round(t["alg_GBs"], 2), "peak": HBM_PEAK_GBS,
            "unit": "GB/s", "frac": round(t["alg_GBs"] / HBM_PEAK_GBS, 5),
            "traffic": traffic, "traffic_source": traffic_src,
            # the same fraction on the COUNTER bytes (calibrated: 2 x FETCH_SIZE + WRITE_SIZE) instead of the algorithmic model
            "traffic_frac": (round(traffic / (t["avg_us"] * 1e-6) / 1e9 / HBM_PEAK_GBS, 5) if traffic else None),
            "valu_issue_frac": valu, "valu_issue_source": valu_src,
            # useful FMA lane-operations / issued VALU lane-slots: filled in by the cpu_baseline leg, whose oracle counts the
            # (pixel, splat) pairs the frame really blends (`blended_pairs`); issued = SQ_INSTS_VALU x 64 lanes (committed PMC)
            "valu_useful_frac": None, "valu_insts_per_launch": insts, "valu_insts_source": insts_src,
            "avg_launch_us": round(t["avg_us"], 2), "host_stalls_left_out": stalls, "alg_bytes_per_launch": t["alg_bytes"],
            "pairs_per_frame_D": D, "measured_copy_GBs": round(copy_GBs, 1),
            "color_only_backward": (None if not rec_color else {
                "avg_launch_us": round(1e3 * sorted(rec_color)[len(rec_color) // 2], 2),
                "what": "composite_bwd when the seven maps take no gradient (dL_dallmap = NULL: every fine pass of the headline step): "
                        "median launch of the same frames; 16 sums per (entry, block) instead of 22, no depth / distortion / normal chain"}),
            "whole_frame": {"alg_bytes": frame_bytes, "kernel_us": round(frame_us, 1),
                            "achieved": round(frame_bytes / frame_us / 1e3, 1),
                            "frac": round(frame_bytes / frame_us / 1e3 / HBM_PEAK_GBS, 5)}}
    return roof, table, D


def _newest_profile(pattern, reader, accept=lambda f: True):
    """(value, 'profiles/<file> (committed rocprofv3 summary, not measured in this run)') from the newest match."""
    import glob
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", pattern)), reverse=True):
        if not accept(f):
            continue
        try:
            v = reader(f)
            if v is not None:
                return v, f"profiles/{os.path.basename(f)} (committed rocprofv3 --pmc summary; not measured in this run)"
        except Exception:
            continue
    return None, None


def live_counters(kernel, args, timeout_s=90):
    """The dominant kernel's SQ and HBM counters MEASURED IN THIS RUN: three short rocprofv3 passes (counters in their own passes,
    `--kernel-trace --pmc` only, as MI355X_MICROARCH.md prescribes: FETCH_SIZE and WRITE_SIZE do not fit one pass) of this script's
    serialised raster step (one scene, one operator call per view, one stream), run as child processes from /tmp.  Returns
    {counter: mean per launch of `kernel`} or None (no rocprofv3 on the box, a pass timed out or produced nothing -- the
    committed summaries under profiles/ are read instead and say so)."""
    import csv, glob, shutil, subprocess, tempfile
    exe = shutil.which("rocprofv3")
    if exe is None:
        return None
    out = {}
    base = [sys.executable, os.path.abspath(__file__), "--steps", "1", "--warmup", "0", "--scenes", "1", "--views", str(args.views), "--res", str(args.res),
            "--grid", str(args.grid), "--regime", args.regime, "--step", "raster", "--raster-api", "loop", "--streams", "1", "--no-fine",
            "--no-cpu-baseline", "--no-roofline"]
    env = dict(os.environ, TMPDIR="/tmp")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    for counters in (["SQ_WAVES", "SQ_INSTS_VALU", "SQ_ACTIVE_INST_VALU", "GRBM_GUI_ACTIVE"], ["FETCH_SIZE"], ["WRITE_SIZE"]):
        d = tempfile.mkdtemp(prefix="lara_pmc_", dir="/tmp")
        try:
            r = subprocess.run([exe, "--kernel-trace", "--output-format", "csv", "--pmc", *counters, "-d", d, "-o", "pmc", "--", *base],
                               cwd="/tmp", env=env, capture_output=True, text=True, timeout=timeout_s)
            files = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
            if r.returncode != 0 or not files:
                return None
            acc = {}
            for f in files:
                for row in csv.DictReader(open(f)):
                    if (kernel + "_kernel") in row["Kernel_Name"]:
                        acc.setdefault(row["Counter_Name"], []).append(float(row["Counter_Value"]))
            for c in counters:
                if c not in acc:
                    return None
                out[c] = sum(acc[c]) / len(acc[c])
                out["launches"] = len(acc[c])
        except Exception:
            return None
        finally:
            shutil.rmtree(d, ignore_errors=True)
    return out


def _valu_issue_frac(csv_path, kernel):
    """SQ_ACTIVE_INST_VALU counts quad-cycles (4 shader cycles) summed over the chip's 1024 SIMDs; GRBM_GUI_ACTIVE is
    the launch's duration in shader cycles summed over the 8 XCDs (rocprofv3 adds the per-XCD instances)."""
    import csv
    for r in csv.DictReader(open(csv_path)):
        if r["kernel"].split("<")[0] == kernel and r.get("SQ_ACTIVE_INST_VALU") and r.get("GRBM_GUI_ACTIVE"):
            return round(4.0 * float(r["SQ_ACTIVE_INST_VALU"]) / (1024.0 * float(r["GRBM_GUI_ACTIVE"]) / 8.0), 4)
    return None


def _pmc_value(csv_path, kernel, counter):
    import csv
    for r in csv.DictReader(open(csv_path)):
        if r["kernel"].split("<")[0] == kernel and r.get(counter):
            return float(r[counter])
    return None


# FMA-equivalent lane operations one blended (pixel, splat) pair needs (~60 flop forward, ~150 flop
# backward per evaluation = 30 / 75 fused multiply-adds)
USEFUL_FMA_PER_PAIR = {"composite_fwd": 30, "composite_bwd": 75}


def attention_leg(device, scenes):
    """Group cross-attention step of one transformer layer for this rank's scenes (forward, bf16
    MFMA): time and FLOP rate against the 2.5 PFLOP/s dense bf16 peak.  Reported beside the raster;
    not part of `value`."""
    from torch import nn
    from lara_amd import rasterizer
    from lara_amd.attention import GroupCrossAttention
    torch.manual_seed(0)
    mod = GroupCrossAttention.from_modules(
        nn.LayerNorm(256), nn.MultiheadAttention(256, 16, kdim=800, vdim=800, bias=False, batch_first=True)).to(device)
    G = 4096 * scenes
    x = torch.randn(G, 8, 256, device=device)
    cond = torch.randn(G, 4, 800, device=device)
    with torch.no_grad():
        for _ in range(2):
            mod(x, cond)
        torch.cuda.synchronize()
        rasterizer.profile_enable(True)
        for _ in range(5):
            mod(x, cond)
        torch.cuda.synchronize()
    rec = rasterizer.profile_collect()
    rasterizer.profile_enable(False)
    us = 1e3 * sum(ms for _, ms in rec) / 5
    flops = G * (2 * 8 * 256 * 256 * 2 + 2 * 4 * 800 * 512 + 2 * 2 * 8 * 4 * 16 * 16)
    # What this formulation must move through HBM whatever its kernels do: the fp32 residual stream in and out, the bf16 conditioning
    # rows, the K|V rows written by their projection and read back by the attention kernel.  (Fusing that projection into the per-group
    # kernel -- VERDICT r5 #5 -- would take the 67 MB round trip away and the projection's weight reuse with it: a wave owns 16 conditioning
    # rows and would stream the 0.8 MB weight matrix for them.)  At the copy rate this part sustains the step cannot be faster than
    # `hbm_floor_us`, i.e. its ceiling against the matrix peak is `ceiling_frac`, not 1.
    hbm_bytes = G * (2 * 8 * 256 * 4 + 4 * 800 * 2 + 2 * 4 * 512 * 2)
    floor_us = hbm_bytes / (MEASURED_COPY_GBS * 1e3)
    return {"workload": f"GroupAttBlock attention step (LN, q/k/v/out projections, QK^T, softmax, AV), "
                        f"{scenes} scenes = {G} groups, forward, bf16 MFMA / fp32 accumulate",
            "us_per_layer": round(us, 1), "achieved": round(flops / us / 1e6, 1), "peak": 2500.0,
            "unit": "TFLOP/s", "frac": round(flops / us / 1e6 / 2500.0, 4), "bound": "mfma",
            "hbm_bytes": hbm_bytes, "hbm_floor_us": round(floor_us, 1), "copy_GBs_assumed": MEASURED_COPY_GBS,
            "ceiling_frac": round(flops / floor_us / 1e6 / 2500.0, 4), "frac_of_ceiling": round(floor_us / us, 4)}


def encoder_leg(device, scenes):
    """The whole volume transformer (12 GroupAttBlocks on a 32^3 x 256 volume + the x2 deconvolution,
    network.py:105-164) for this rank's scenes, forward, random-init weights of the reference's shapes:
    time and FLOP rate against the 2.5 PFLOP/s dense bf16 peak.  Reported beside the raster."""
    from lara_amd import rasterizer
    from lara_amd.encoder import VolTransformer
    torch.manual_seed(0)
    vt = VolTransformer(256, 800, [16], 32, 64, 80, 12, 16).to(device)
    with torch.no_grad():
        for n, p in list(vt.named_parameters()) + list(vt.named_buffers()):
            if p.dtype == torch.bfloat16:
                p.copy_((torch.randn(p.shape, device=device) * (p.shape[-1] ** -0.5)).to(torch.bfloat16))
            elif n.endswith("_w"):
                p.fill_(1.0)
        vt.pos_embed.normal_(0, 1 / 16)
        feats = torch.randn(scenes, 4, 800, 16, 16, 16, device=device)
        vt(feats)
        torch.cuda.synchronize()
        rasterizer.profile_enable(True)  # per-kernel HIP events need plain launches
        for _ in range(2):
            vt(feats)
        torch.cuda.synchronize()
        rec = rasterizer.profile_collect()
        rasterizer.profile_enable(False)
        vt(feats, use_graph=True)  # captures the HIP graph
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(3):
            vt(feats, use_graph=True)
        e1.record()
        torch.cuda.synchronize()
        wall_graph = e0.elapsed_time(e1) / 3
    M, G = scenes * 32 ** 3, scenes * 4096
    ms = sum(t for _, t in rec) / 2
    conv_us = 1e3 * sum(t for k, t in rec if k == "gb_conv3d") / 24
    per_layer = 2 * M * 256 * 256 * 2 + 2 * G * 4 * 800 * 512 + 2 * 2 * 8 * 4 * 16 * 16 * G + 2 * M * 256 * 512 * 2 + 2 * M * 27 * 256 * 256
    flops = 12 * per_layer + 2 * M * 256 * 640
    return {"workload": f"VolTransformer forward (12 x [attention, MLP, LayerNorms, Conv3d 3x3x3] + deconv), {scenes} scenes "
                        f"x 32^3 voxels, bf16 MFMA / fp32 accumulate, random-init weights",
            "ms_per_forward": round(ms, 2), "ms_wall_hip_graph": round(wall_graph, 2),
            "achieved": round(flops / ms / 1e9, 1), "peak": 2500.0, "unit": "TFLOP/s",
            "frac": round(flops / ms / 1e9 / 2500.0, 4), "bound": "mfma",
            "conv3d_us": round(conv_us, 1), "conv3d_TFLOPs": round(2 * M * 27 * 256 * 256 / conv_us / 1e6, 1)}


def encoder_train_leg(device, scenes):
    """The trainable drop-in (lara_amd.encoder_train.VolTransformer: fp32 master parameters with the
    reference's state_dict, HIP forward AND backward) on this rank's scenes: one forward + backward per step,
    gradients for every parameter and for the image features.  Reported beside the raster."""
    from lara_amd.encoder_train import VolTransformer
    torch.manual_seed(0)
    vt = VolTransformer(256, 800, [16], 32, 64, 80, 12, 16).to(device)  # the reference's own initialisation
    feats = torch.randn(scenes, 4, 800, 16, 16, 16, device=device, requires_grad=True)
    dout = torch.randn(scenes, 64, 64, 64, 80, device=device)

    def one():
        vt(feats).backward(dout)
        vt.zero_grad(set_to_none=True)
        feats.grad = None

    torch.cuda.reset_peak_memory_stats(device)
    one()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(3):
        one()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 3
    M, G = scenes * 32 ** 3, scenes * 4096
    per_layer = 2 * M * 256 * 256 * 2 + 2 * G * 4 * 800 * 512 + 2 * 2 * 8 * 4 * 16 * 16 * G + 2 * M * 256 * 512 * 2 + 2 * M * 27 * 256 * 256
    flops = 3 * (12 * per_layer + 2 * M * 256 * 640)   # backward = 2 x forward (dX and dW for every product)
    return {"workload": f"VolTransformer forward + backward, {scenes} scenes x 32^3 voxels, 12 layers, bf16 MFMA / fp32 "
                        f"accumulate, fp32 master parameters, all parameter and image-feature gradients",
            "ms_per_step": round(ms, 2), "achieved": round(flops / ms / 1e9, 1), "peak": 2500.0, "unit": "TFLOP/s",
            "frac": round(flops / ms / 1e9 / 2500.0, 4), "bound": "mfma",
            "peak_memory_GiB": round(torch.cuda.max_memory_allocated(device) / 2 ** 30, 1)}


def render_img_leg(device, args):
    """One scene's 8 views through the whole of `Renderer.render_img` (renderer_2dgs.py:167-268), forward +
    backward with a gradient on every returned map: (a) the reference's sequence on the drop-in rasteriser --
    activations per view and ~15 torch kernels of post-processing per view (restated in torch here, as the
    reference's class does it); (b) `lara_amd.renderer.Renderer` -- activations once per scene, one fused HIP
    kernel per direction.  Single stream, as the reference's Python loop issues it."""
    import torch.nn.functional as F
    from lara_amd import batch, cameras, synthetic
    from lara_amd.renderer import Renderer
    sc = synthetic.make_scene(grid=args.grid, K=2, regime=args.regime, seed=123, device=device)
    c2w = cameras.turntable_c2w(args.views).to(device)
    cams = cameras.make_cameras(c2w, args.res, args.res, 0.75, 0.75, 1.906 - 0.8, 1.906 + 0.8, device=device)
    ixt = batch.fov_to_ixt(torch.tensor([0.75, 0.75], device=device), (args.res, args.res))
    rays = batch.build_rays(c2w, ixt.reshape(1, 3, 3).expand(args.views, 3, 3).contiguous(), args.res, args.res)
    keys = ("image", "depth", "acc_map", "rend_normal", "depth_normal", "rend_dist")
    r = Renderer(sh_degree=1, white_background=True)

    def ref_style(cam, ray, p):
        rast = r.set_rasterizer(cam, device=device)
        sp = torch.zeros_like(p["centers"], requires_grad=True) + 0
        col, _, allmap = rast(means3D=p["centers"], means2D=sp, shs=p["shs"], opacities=torch.sigmoid(p["opacity"]),
                              scales=torch.exp(p["scales"]), rotations=F.normalize(p["rotations"]), cov3D_precomp=None)
        image = col.clamp(0, 1)
        alpha = allmap[1:2]
        normal = (allmap[2:5].permute(1, 2, 0) @ (cam.world_view_transform[:3, :3].T)).permute(2, 0, 1)
        median = torch.nan_to_num(allmap[5:6], 0, 0)
        expected = torch.nan_to_num(allmap[0:1] / alpha, 0, 0)
        surf = expected * (1 - 0.0) + 0.0 * median
        pts = (ray[..., :3].reshape(-1, 3) + surf.reshape(-1, 1) * ray[..., 3:].reshape(-1, 3)).reshape(*surf.shape[1:], 3)
        out = torch.zeros_like(pts)
        dx = pts[2:, 1:-1] - pts[:-2, 1:-1]
        dy = pts[1:-1, 2:] - pts[1:-1, :-2]
        out[1:-1, 1:-1, :] = F.normalize(torch.cross(dx, dy, dim=-1), dim=-1)
        dn = out.permute(2, 0, 1) * alpha.detach()
        return {"image": image.permute(1, 2, 0), "depth": surf.permute(1, 2, 0), "acc_map": alpha.squeeze(0),
                "rend_normal": normal.permute(1, 2, 0), "depth_normal": dn.permute(1, 2, 0), "rend_dist": allmap[6]}

    def one(mode):
        # as network.py:473-497 calls it: batched tensors [B, P, ...], a FRESH `x[i]` view object per view
        pb = {k: v.detach()[None].requires_grad_(True) for k, v in sc.items()}
        loss = 0
        if mode == "views":     # the whole loop as ONE call (Renderer.render_views: one rasteriser node for the 8 views)
            p = {k: v[0] for k, v in pb.items()}
            for o in r.render_views(cams, rays, p["centers"], p["shs"], p["opacity"], p["scales"], p["rotations"], device):
                for k in keys:
                    loss = loss + o[k].sum() * 1e-6
            loss.backward()
            return
        for cam, ray in zip(cams, rays):
            p = {k: v[0] for k, v in pb.items()}
            o = (r.render_img(cam, ray, p["centers"], p["shs"], p["opacity"], p["scales"], p["rotations"], device)
                 if mode == "fused" else ref_style(cam, ray, p))
            for k in keys:
                loss = loss + o[k].sum() * 1e-6
        loss.backward()

    res = {}
    for mode in ("reference_style", "fused", "views"):
        one(mode)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(2):
            one(mode)
        torch.cuda.synchronize()
        res[mode] = round(2 * args.views / (time.perf_counter() - t0), 1)
    return {"workload": f"Renderer.render_img fwd+bwd, 1 scene x {args.views} views @{args.res}x{args.res}, gradients on all six "
                        f"returned maps, one stream", "unit": "frames/s", "reference_style_torch_postprocessing": res["reference_style"],
            "fused_renderer": res["fused"], "fused_renderer_render_views": res["views"]}


def point_feats_leg(device, args):
    """The fine stage's point sampler (network.py:390-411): 262 144 points (half of a scene's Gaussians pass the
    opacity mask) into the 4 input views @res, forward + backward: the reference's torch sequence (projection,
    cat + permute, grid_sample, and their autograd) against the fused HIP kernels."""
    import torch.nn.functional as F
    from lara_amd import cameras
    from lara_amd.fine import sample_point_feats
    g = torch.Generator().manual_seed(3)
    V, h, w, n = 4, args.res, args.res, 262144
    w2c = torch.linalg.inv(cameras.turntable_c2w(V).double()).float().to(device)
    focal = 0.5 * w / math.tan(0.5 * 0.75)
    ixt = torch.tensor([[focal, 0, w / 2], [0, focal, h / 2], [0, 0, 1.0]], dtype=torch.float32).expand(V, 3, 3).contiguous().to(device)
    pts0 = ((torch.rand(n, 3, generator=g) * 2 - 1) * 0.5).to(device)
    img_ref = torch.rand(V, 3, h, w, generator=g).to(device)
    maps0 = [torch.rand(V, h, w, 3, generator=g).to(device), torch.rand(V, h, w, generator=g).to(device),
             (1.5 + torch.rand(V, h, w, 1, generator=g)).to(device)]
    gout = torch.randn(V, 8, n, generator=g).to(device)

    def torch_path(points, image, acc, depth):
        pc = points.reshape(1, -1, 3) @ w2c[:, :3, :3].permute(0, 2, 1) + w2c[:, :3, 3][:, None]
        q = pc @ ixt.permute(0, 2, 1)
        xy, z = q[..., :2] / q[..., -1:], q[..., -1:]
        grid = (xy + 0.5) / torch.tensor([w, h], device=device) * 2 - 1.0
        stack = torch.cat((img_ref, torch.einsum('bhwc->bchw', torch.cat((image, acc.unsqueeze(-1), depth), dim=-1))), dim=1)
        feats = F.grid_sample(stack, grid.unsqueeze(1), align_corners=False).view(V, -1, n)
        return torch.cat((feats[:, :-1], (feats[:, -1:] - z.view(V, -1, n)).abs()), dim=1)

    def one(fused):
        p = pts0.clone().requires_grad_(True)
        m = [t.clone().requires_grad_(True) for t in maps0]
        out = sample_point_feats(p, w2c, ixt, img_ref, *m) if fused else torch_path(p, *m)
        out.backward(gout)

    res = {}
    for fused in (False, True):
        one(fused)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            one(fused)
        e1.record()
        torch.cuda.synchronize()
        res[fused] = e0.elapsed_time(e1) / 5 * 1e3
    return {"workload": f"get_point_feats fwd+bwd, {n} points x {V} views @{h}x{w} (incl. cloning the inputs)", "unit": "us",
            "torch_sequence_us": round(res[False], 1), "fused_us": round(res[True], 1)}


def _leg(name):
    """Progress line on stderr: a leg that dies (device fault, time-out) is then named in the log."""
    print(f"[bench] {name}", file=sys.stderr, flush=True)


def coarse_decoder_leg(device, scenes):
    """`Decoder.forward_coarse` (network.py:259-278) on the batch's scenes x 64^3 voxel rows, forward + backward with gradients
    to the volume features and the six parameters: the torch sequence under bf16 autocast arithmetic (`pipeline.decode_coarse`:
    three bf16 GEMMs with chip-filling weight gradients, split, activations) and the fused HIP kernels (`lara_amd.coarse`)."""
    from lara_amd import coarse, rasterizer
    from lara_amd.pipeline import CoarseFineDecoder, decode_coarse
    torch.manual_seed(0)
    dec = CoarseFineDecoder().to(device)
    M = 64 ** 3
    x0 = torch.randn(scenes, M, 80, device=device)
    gouts = None

    def one(mode):
        nonlocal gouts
        x = x0.clone().requires_grad_(True)
        res = coarse.forward_coarse(dec, x, -2.1792, -5.26) if mode == "fused" else decode_coarse(dec, x, -2.1792, -5.26, True)
        if gouts is None:
            gouts = [torch.randn_like(r) for r in res]
        torch.autograd.backward(res, gouts)
        for p in dec.parameters():
            p.grad = None

    res = {}
    for mode in ("torch", "fused"):
        one(mode)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(3):
            one(mode)
        e1.record()
        torch.cuda.synchronize()
        res[mode] = e0.elapsed_time(e1) / 3 * 1e3
    rasterizer.profile_enable(True)
    one("fused")
    torch.cuda.synchronize()
    k = {name: round(ms * 1e3, 1) for name, ms in rasterizer.profile_collect()}
    rasterizer.profile_enable(False)
    rows = scenes * M
    fwd_bytes, bwd_bytes = rows * (320 + 88 * 2), rows * (320 + 88 * 2 + 12 * 2 + 320 + 896)
    out = {"workload": f"Decoder.forward_coarse fwd+bwd, {rows} voxel rows ({scenes} scenes), K = 2, gradients to the features and "
                       "the parameters (incl. cloning the input)", "unit": "us", "torch_sequence_bf16_us": round(res["torch"], 1),
           "fused_us": round(res["fused"], 1), "kernels_us": k, "bound": "hbm"}
    if "coarse_decoder_fwd" in k:
        out["fwd_GBs"] = round(fwd_bytes / (k["coarse_decoder_fwd"] * 1e-6) / 1e9, 1)
    if "coarse_decoder_bwd" in k:
        out["bwd_GBs"] = round(bwd_bytes / (k["coarse_decoder_bwd"] * 1e-6) / 1e9, 1)
    return out


def fine_decoder_leg(device):
    """`Decoder.forward_fine` (network.py:280-284) on one scene's 524 288 Gaussians (the init regime keeps 99.9 % of
    them), forward + backward with gradients to both inputs and all ten parameters: the reference's torch sequence
    (LayerNorm, nn.MultiheadAttention with one query and four keys, Linear-ReLU-Linear) under bf16 autocast as the
    reference trains it, the same in fp32, and the fused HIP kernels (fp32)."""
    from torch import nn
    from lara_amd import rasterizer
    from lara_amd.fine import forward_fine

    class Dec(nn.Module):       # the reference's declarations, network.py:234-240
        def __init__(self):
            super().__init__()
            self.norm = nn.LayerNorm(80)
            self.cross_att = nn.MultiheadAttention(embed_dim=80, num_heads=8, kdim=8, vdim=8, dropout=0.0, bias=False, batch_first=True)
            self.mlp_fine = nn.Sequential(nn.Linear(80, 64), nn.ReLU(), nn.Linear(64, 12))

        def forward_fine(self, volume_feat, point_feats):
            volume_feat = self.norm(volume_feat.unsqueeze(1))
            x = self.cross_att(volume_feat, point_feats, point_feats, need_weights=False)[0]
            return self.mlp_fine(x).float()

    torch.manual_seed(0)
    dec = Dec().to(device)
    n = 524288
    vol0 = torch.randn(n, 80, device=device)
    pf0 = torch.randn(4, 8, n, device=device)
    gout = torch.randn(n, 1, 12, device=device)

    def one(mode):
        vol, pfp = vol0.clone().requires_grad_(True), pf0.clone().requires_grad_(True)
        pf = torch.einsum('lcb->blc', pfp)
        if mode == "fused":
            sh = forward_fine(dec, vol, pf)
        else:
            # torch's scaled-dot-product kernels reject 524 288 x 8 (batch x heads) problems in one launch on this
            # build (hipErrorInvalidValue), so the reference sequence is fed 16 chunks of 32 768 points
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=(mode == "torch_bf16")):
                sh = torch.cat([dec.forward_fine(v, q) for v, q in zip(vol.split(32768), pf.split(32768))])
        sh.backward(gout)
        for p in dec.parameters():
            p.grad = None

    res = {}
    for mode in ("torch_bf16", "torch_fp32", "fused"):
        one(mode)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(3):
            one(mode)
        e1.record()
        torch.cuda.synchronize()
        res[mode] = e0.elapsed_time(e1) / 3 * 1e3
    rasterizer.profile_enable(True)
    one("fused")
    torch.cuda.synchronize()
    k = {}
    for name, ms in rasterizer.profile_collect():
        k[name] = round(ms * 1e3, 1)
    rasterizer.profile_enable(False)
    flop = n * 2 * (64 * 80 + 64 * 64 + 12 * 64 + 600)
    return {"workload": f"Decoder.forward_fine fwd+bwd, {n} points (one scene), gradients to inputs and parameters (incl. cloning the inputs)",
            "unit": "us", "torch_sequence_bf16_autocast_us": round(res["torch_bf16"], 1), "torch_sequence_fp32_us": round(res["torch_fp32"], 1),
            "fused_us": round(res["fused"], 1), "kernels_us": k,
            "fwd_kernel_TFLOPs_f32": round(flop / (k.get("fine_decoder_fwd", 1e9) * 1e-6) / 1e12, 1) if "fine_decoder_fwd" in k else None}


def fine_stage_leg(device, args):
    """One scene through LaRa's whole render section after `start_fine` (network.py:486-527): 8 coarse views ->
    `get_point_feats` on the 4 input views -> `Decoder.forward_fine` -> 8 fine views over the opacity > 0.005 subset,
    forward + backward with gradients on image / depth / normal maps of all 16 frames:
      (a) reference style -- the reference's sequence of torch operators around the drop-in rasteriser (one call per
          view, torch post-processing, torch sampler, torch modules of the fine decoder, boolean-mask gathers per view);
      (b) every opt-in of this repository -- `Renderer.render_views`, `fine.sample_point_feats`, `fine.forward_fine`,
          `fine.take_rows`.
    What a LaRa training step spends per scene on rows R0-R11 + section 8f-2/8f-4, as frames/s (16 frames per scene)."""
    import torch.nn.functional as F
    from torch import nn
    from lara_amd import batch, cameras, synthetic
    from lara_amd.fine import forward_fine, sample_point_feats, take_rows
    from lara_amd.renderer import Renderer

    class Dec(nn.Module):       # the reference's declarations, network.py:234-240
        def __init__(self):
            super().__init__()
            self.norm = nn.LayerNorm(80)
            self.cross_att = nn.MultiheadAttention(embed_dim=80, num_heads=8, kdim=8, vdim=8, dropout=0.0, bias=False, batch_first=True)
            self.mlp_fine = nn.Sequential(nn.Linear(80, 64), nn.ReLU(), nn.Linear(64, 12))

        def forward_fine(self, volume_feat, point_feats):
            volume_feat = self.norm(volume_feat.unsqueeze(1))
            x = self.cross_att(volume_feat, point_feats, point_feats, need_weights=False)[0]
            return self.mlp_fine(x).float()

    torch.manual_seed(1)
    dec = Dec().to(device)
    V, res, nsel = args.views, args.res, 4
    sc = synthetic.make_scene(grid=args.grid, K=2, regime=args.regime, seed=321, device=device)
    P = sc["centers"].shape[0]
    c2w = cameras.turntable_c2w(V).to(device)
    cams = cameras.make_cameras(c2w, res, res, 0.75, 0.75, 1.906 - 0.8, 1.906 + 0.8, device=device)
    ixt = batch.fov_to_ixt(torch.tensor([0.75, 0.75], device=device), (res, res)).reshape(1, 3, 3).expand(V, 3, 3).contiguous()
    rays = batch.build_rays(c2w, ixt, res, res)
    w2c = torch.linalg.inv(c2w.double()).float()
    img_ref = torch.rand(nsel, 3, res, res, device=device)
    vol_feat0 = torch.randn(P, 80, device=device) * 0.5
    keys = ("image", "depth", "rend_normal")
    r = Renderer(sh_degree=1, white_background=True)
    mask = torch.sigmoid(sc["opacity"].detach()).squeeze(-1) > FINE_OPACITY
    idx = mask.nonzero().squeeze(-1)

    def ref_view(cam, ray, centers, shs, opacity, scales, rotations):     # renderer_2dgs.py:181-268 as torch operators
        rast = r.set_rasterizer(cam, device=device)
        sp = torch.zeros_like(centers, requires_grad=True) + 0
        col, _, allmap = rast(means3D=centers, means2D=sp, shs=shs, opacities=torch.sigmoid(opacity), scales=torch.exp(scales),
                              rotations=F.normalize(rotations), cov3D_precomp=None)
        image = col.clamp(0, 1)
        alpha = allmap[1:2]
        normal = (allmap[2:5].permute(1, 2, 0) @ (cam.world_view_transform[:3, :3].T)).permute(2, 0, 1)
        expected = torch.nan_to_num(allmap[0:1] / alpha, 0, 0)
        return {"image": image.permute(1, 2, 0), "depth": expected.permute(1, 2, 0), "acc_map": alpha.squeeze(0),
                "rend_normal": normal.permute(1, 2, 0)}

    def ref_sampler(points, image, acc, depth):                            # network.py:390-411
        pc = points.reshape(1, -1, 3) @ w2c[:nsel, :3, :3].permute(0, 2, 1) + w2c[:nsel, :3, 3][:, None]
        q = pc @ ixt[:nsel].permute(0, 2, 1)
        xy, z = q[..., :2] / q[..., -1:], q[..., -1:]
        grid = (xy + 0.5) / torch.tensor([res, res], device=device) * 2 - 1.0
        stack = torch.cat((img_ref, torch.einsum('bhwc->bchw', torch.cat((image, acc.unsqueeze(-1), depth), dim=-1))), dim=1)
        n = points.shape[0]
        feats = F.grid_sample(stack, grid.unsqueeze(1), align_corners=False).view(nsel, -1, n)
        return torch.cat((feats[:, :-1], (feats[:, -1:] - z.view(nsel, -1, n)).abs()), dim=1)

    def one(opt_in):
        p = {k: v.detach().clone().requires_grad_(True) for k, v in sc.items()}
        vol_feat = vol_feat0.clone().requires_grad_(True)
        loss = 0
        if opt_in:
            coarse = r.render_views(cams, rays, p["centers"], p["shs"], p["opacity"], p["scales"], p["rotations"], device)
        else:
            coarse = [ref_view(cam, ray, p["centers"], p["shs"], p["opacity"], p["scales"], p["rotations"]) for cam, ray in zip(cams, rays)]
        for o in coarse:
            for k in keys:
                loss = loss + o[k].sum() * 1e-6
        ren = {k: torch.stack([o[k] for o in coarse[:nsel]]) for k in ("image", "acc_map", "depth")}
        if opt_in:
            centers_f = take_rows(p["centers"], idx)
            pf = sample_point_feats(centers_f, w2c[:nsel], ixt[:nsel], img_ref, ren["image"], ren["acc_map"], ren["depth"])
            sh_res = forward_fine(dec, take_rows(vol_feat, idx), torch.einsum('lcb->blc', pf))
            shs_f = sh_res.view(-1, 4, 3) + take_rows(p["shs"], idx)
            fine = r.render_views(cams, rays, centers_f, shs_f, take_rows(p["opacity"], idx), take_rows(p["scales"], idx),
                                  take_rows(p["rotations"], idx), device)
        else:
            centers_f = p["centers"][mask]
            pf = torch.einsum('lcb->blc', ref_sampler(centers_f, ren["image"], ren["acc_map"], ren["depth"]))
            vf = vol_feat[mask]
            with torch.autocast("cuda", dtype=torch.bfloat16):     # the reference trains under bf16-mixed
                sh_res = torch.cat([dec.forward_fine(a, b) for a, b in zip(vf.split(32768), pf.split(32768))])
            shs_f = sh_res.view(-1, 4, 3) + p["shs"][mask]
            fine = [ref_view(cam, ray, centers_f, shs_f, p["opacity"][mask], p["scales"][mask], p["rotations"][mask])
                    for cam, ray in zip(cams, rays)]
        for o in fine:
            for k in keys:
                loss = loss + o[k].sum() * 1e-6
        loss.backward()
        for q in dec.parameters():
            q.grad = None

    res_ = {}
    for opt_in in (False, True):
        one(opt_in)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(2):
            one(opt_in)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / 2
        res_[opt_in] = (round(2 * V / dt, 1), round(1e3 * dt, 2))
    return {"workload": f"one scene through the render section after start_fine: {V} coarse views, point sampler on {nsel} views, "
                        f"forward_fine on {int(idx.numel())} points, {V} fine views, forward + backward; one stream",
            "unit": "frames/s", "reference_style_torch_operators": res_[False][0], "ms_per_scene_reference_style": res_[False][1],
            "all_opt_ins": res_[True][0], "ms_per_scene_all_opt_ins": res_[True][1]}


def rays_leg(device, scenes, views, res):
    """Device-side generation of the step's tar_rays + tar_rays_down (dataLoader/utils.py:21-34):
    a pure store stream, priced against the HBM peak."""
    from lara_amd import cameras
    from lara_amd.batch import build_rays, fov_to_ixt
    c2w = cameras.turntable_c2w(views).float().to(device)
    ixt = fov_to_ixt(torch.full((views, 2), 0.75), (res, res)).to(device)
    from lara_amd import rasterizer
    for _ in range(2):
        build_rays(c2w, ixt, res, res)
    torch.cuda.synchronize()
    rasterizer.profile_enable(True)
    for _ in range(scenes * 5):
        build_rays(c2w, ixt, res, res)
        build_rays(c2w, ixt, res, res, 1.0 / 16)
    torch.cuda.synchronize()
    rec = rasterizer.profile_collect()
    rasterizer.profile_enable(False)
    us = 1e3 * sum(t for k, t in rec if k == "build_rays") / 5  # kernel time (HIP events on the launch stream)
    nbytes = scenes * views * 24 * (res * res + (res // 16) ** 2)
    return {"workload": f"tar_rays + tar_rays_down of {scenes} scenes x {views} views @{res}x{res}, written on the device",
            "us_per_step": round(us, 1), "achieved": round(nbytes / us / 1e3, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(nbytes / us / 1e3 / HBM_PEAK_GBS, 4), "bound": "hbm"}


def cpu_baseline(args):
    """The CPU oracle (fp32 restatement, OpenMP over tiles) on a bounded sample of the same
    workload: the 8 views of scene 0, forward + backward each (about 10-30 s of CPU work)."""
    import numpy as np
    import oracle
    from lara_amd import cameras, synthetic
    sc = synthetic.make_scene(grid=args.grid, K=2, regime=args.regime, seed=0)
    act = {k: v.numpy() for k, v in synthetic.activate(sc).items()}
    res = args.res   # the sample is a subset of the workload's frames, never a smaller frame
    cams = cameras.make_cameras(cameras.turntable_c2w(args.views), res, res, 0.75, 0.75,
                                1.906 - 0.8, 1.906 + 0.8)
    oracle.build()
    g = np.random.default_rng(0)
    dc = g.normal(size=(3, res, res)).astype(np.float32)
    da = (0.1 * g.normal(size=(7, res, res))).astype(np.float32)   # (the gradient mix of tests/test_raster_parity_gpu.py)
    t0 = time.perf_counter()
    D = 0
    first = None
    for cam in cams:
        view = oracle.View(res, res, math.tan(0.375), math.tan(0.375), np.ones(3, np.float32), 1.0,
                           cam.world_view_transform.numpy(), cam.full_proj_transform.numpy(), 1,
                           cam.camera_center.numpy())
        r = oracle.forward(view, act["means3D"], act["opacities"], shs=act["shs"], scales=act["scales"],
                           rotations=act["rotations"])
        gr = oracle.backward(r, dc, da)
        D = r.num_rendered
        if first is None:
            first = (r, gr)
    dt = time.perf_counter() - t0
    cores = int(os.environ.get("OMP_NUM_THREADS", os.cpu_count() or 1))
    out = {"value": round(len(cams) / dt, 4), "unit": "frames/s", "cores": cores, "kind": "port",
           "sample": f"{len(cams)} frames (fwd+bwd, the {len(cams)} views of scene 0, {res}x{res}, "
                     f"P={act['means3D'].shape[0]}, D~{D}) with the OpenMP fp32 oracle; {dt:.2f} s"}
    # the checker's other job: the HIP frame of view 0 against the oracle's, at full size (BASELINE's "PSNR vs ref";
    # the oracle stands in for the absent reference rasteriser)
    from lara_amd import GaussianRasterizationSettings, GaussianRasterizer
    dev = torch.device("cuda", torch.cuda.current_device())
    cam = cams[0]
    rs = GaussianRasterizationSettings(
        image_height=res, image_width=res, tanfovx=math.tan(0.375), tanfovy=math.tan(0.375), bg=torch.ones(3, device=dev),
        scale_modifier=1.0, viewmatrix=cam.world_view_transform.to(dev), projmatrix=cam.full_proj_transform.to(dev),
        sh_degree=1, campos=cam.camera_center.to(dev), prefiltered=False, debug=False)
    t = {k: torch.from_numpy(v).to(dev).requires_grad_(True) for k, v in act.items()}
    m2d = torch.zeros_like(t["means3D"], requires_grad=True)
    color, radii, allmap = GaussianRasterizer(rs)(means3D=t["means3D"], means2D=m2d, shs=t["shs"], opacities=t["opacities"],
                                                  scales=t["scales"], rotations=t["rotations"], cov3D_precomp=None)
    ((color * torch.from_numpy(dc).to(dev)).sum() + (allmap * torch.from_numpy(da).to(dev)).sum()).backward()
    r, gr = first
    mse = float(((color.detach().cpu().numpy() - r.color) ** 2).mean())
    gerr, l2err = {}, {}
    for k in ("means3D", "opacities", "scales", "rotations", "shs"):
        d = t[k].grad.cpu().numpy().reshape(gr[k].shape).astype(np.float64) - gr[k]
        gerr[k] = float(np.abs(d).max() / (np.abs(gr[k]).max() + 1e-20))
        l2err[k] = float(np.sqrt((d ** 2).sum() / ((gr[k].astype(np.float64) ** 2).sum() + 1e-300)))
    # yardstick: the fp32 oracle's own gradient after every input moved by one ulp (tools/grad_probe.py)
    rng = np.random.default_rng(1)
    pert = {k: (v * (1 + (rng.integers(0, 2, v.shape) * 2 - 1) * 2.0 ** -23)).astype(np.float32) for k, v in act.items()}
    view0 = oracle.View(res, res, math.tan(0.375), math.tan(0.375), np.ones(3, np.float32), 1.0, cam.world_view_transform.numpy(),
                        cam.full_proj_transform.numpy(), 1, cam.camera_center.numpy())
    rp = oracle.forward(view0, pert["means3D"], pert["opacities"], shs=pert["shs"], scales=pert["scales"], rotations=pert["rotations"])
    gp = oracle.backward(rp, dc, da)
    self_l2 = {k: float(np.sqrt(((gp[k].astype(np.float64) - gr[k]) ** 2).sum() / ((gr[k].astype(np.float64) ** 2).sum() + 1e-300)))
               for k in l2err}
    out["blended_pairs_view0"] = int(r.blended_pairs)
    arb = None
    try:
        arb_file = sorted(__import__("glob").glob(os.path.join(ROOT, "profiles", "r*_grad_arbitration.json")))[-1]
        a = json.load(open(arb_file))
        arb = {"source": f"profiles/{os.path.basename(arb_file)} (tools/grad_arbiter.py, {a['fp64_seconds']} s of fp64 autograd: committed, not run here)",
               "what": a["what"], "surfels": a["surfels_chosen"], "tiles": a["tiles"],
               "max_err_rel_to_max_fp64": {k: {"hip": v["hip"]["max_err_rel_to_max"], "fp32_oracle": v["fp32_oracle"]["max_err_rel_to_max"]}
                                           for k, v in a["per_tensor"].items()},
               "rel_l2_vs_fp64": {k: {"hip": v["hip"]["rel_l2"], "fp32_oracle": v["fp32_oracle"]["rel_l2"]} for k, v in a["per_tensor"].items()},
               "closer_to_fp64": {k: v["closer_to_fp64"] for k, v in a["per_tensor"].items()}}
    except Exception:
        pass
    out["parity_vs_oracle"] = {"view": 0, "fp64_arbitration": arb, "psnr_color_dB": round(10 * math.log10(1.0 / max(mse, 1e-30)), 1),
                               "oracle_1ulp_self": {"psnr_color_dB": round(10 * math.log10(1.0 / max(float(((rp.color - r.color) ** 2).mean()), 1e-30)), 1),
                                                    "grad_rel_l2": {k: float(f"{v:.2e}") for k, v in self_l2.items()}},
                               "radii_identical": bool(np.array_equal(radii.cpu().numpy(), r.radii)),
                               "max_grad_err_rel_to_max": {k: float(f"{v:.2e}") for k, v in gerr.items()},
                               "grad_err_rel_l2": {k: float(f"{v:.2e}") for k, v in l2err.items()}}
    return out


def cpu_encoder_baseline(scenes=1):
    """The reference's CPU encoder path (BASELINE.json configs[0], north_star: "next to the reference's CPU encoder
    path timed on the same box's host cores in the same run"): `VolTransformer.forward` (network.py:138-164) +
    `Decoder.forward_coarse` (network.py:259-278) for ONE scene at LaRa's sizes (32^3 x 256 volume, 12 layers, 4 views
    x 16^3 x 800 image-feature tokens -> 524 288 Gaussians), fp32 torch.  The reference modules themselves cannot travel
    to this box (/root/reference is absent here); what runs is oracle/voltrans_ref.py, the plain-torch restatement that
    tests/test_voltrans.py pins to the reference's own output (3e-5).  kind = "port".
    A stated baseline should be the best the host can do: the thread count is chosen from
    {8, 32, all} on a 2-layer probe (oversubscribed matmuls get slower: 256 threads took 55.6 s where 8 take 7), then the
    full 12-layer pass runs once as warm-up and once timed at that count."""
    from oracle.voltrans_ref import build_decoder_coarse, build_modules, restated_decoder_coarse, restated_voltrans
    cores = os.cpu_count() or 1
    prev = torch.get_num_threads()
    try:
        feats = torch.randn(scenes, 4, 800, 16, 16, 16)
        probe_mod = build_modules(0, 32, 2)
        probe = {}
        for n in sorted({min(8, cores), min(32, cores), cores}):
            torch.set_num_threads(n)
            with torch.no_grad():
                restated_voltrans(probe_mod, feats)             # warm-up at this thread count
                t0 = time.perf_counter()
                restated_voltrans(probe_mod, feats)
                probe[n] = time.perf_counter() - t0
        best = min(probe, key=probe.get)
        torch.set_num_threads(best)
        m = build_modules(0, 32, 12)
        dec = build_decoder_coarse(1)
        with torch.no_grad():
            restated_voltrans(m, feats)                          # warm-up
            t0 = time.perf_counter()
            vol = restated_voltrans(m, feats)
            t1 = time.perf_counter()
            offset, sh, scaling, rotation, opacity = restated_decoder_coarse(dec, vol, -2.1792, math.log(0.5 * (2 / 64) / 3))
            t2 = time.perf_counter()
        assert tuple(vol.shape) == (scenes, 64, 64, 64, 80) and tuple(opacity.shape) == (scenes, 524288, 1)
    finally:
        torch.set_num_threads(prev)
    return {"value": round(scenes / (t2 - t0), 4), "unit": "scenes/s", "cores": best, "host_cores": cores, "kind": "port",
            "voltransformer_s": round(t1 - t0, 3), "decoder_coarse_s": round(t2 - t1, 3),
            "thread_probe_2_layers_s": {str(k): round(v, 3) for k, v in probe.items()},
            "sample": f"{scenes} scene (VolTransformer 12 x GroupAttBlock on 32^3 x 256 + ConvTranspose3d, then the coarse decoder "
                      f"MLP -> 524288 Gaussians), fp32 torch, {best} threads (best of {sorted(probe)} on a 2-layer probe); one warm-up pass, "
                      f"then one timed pass"}


def reference_optimizer(module, lr):
    """`system.configure_optimizers` (lightning/system.py:78-106): AdamW over two groups -- every LayerNorm parameter and every bias
    without weight decay, the rest with `train.weight_decay` -- with configs/base.yaml's betas; fused multi-tensor update."""
    no_decay = []
    for m in module.modules():
        if isinstance(m, torch.nn.LayerNorm):
            no_decay.extend(m.parameters())
        elif isinstance(getattr(m, "bias", None), torch.nn.Parameter):
            no_decay.append(m.bias)
    ids = set(map(id, no_decay))
    decay = [p for p in module.parameters() if id(p) not in ids and p.requires_grad]
    seen, nd = set(), []
    for p in no_decay:
        if p.requires_grad and id(p) not in seen:
            seen.add(id(p))
            nd.append(p)
    groups = [{"params": decay, "weight_decay": 0.05}, {"params": nd, "weight_decay": 0.0}]
    try:
        return torch.optim.AdamW(groups, lr=lr, betas=(0.9, 0.95), fused=True)
    except (RuntimeError, TypeError):      # (CPU plumbing runs)
        return torch.optim.AdamW(groups, lr=lr, betas=(0.9, 0.95))


def make_pipeline_step(args, device, rank, world, plumbing):
    """The headline step: `lara_amd.pipeline.LaRaPipeline` (network.py:455-532) + `lara_loss` (loss.py minus MS-SSIM) +
    one backward through everything, the encoder's backward last (autograd's order), DDP over ALL trainable
    parameters (VolTransformer + decoder) when N > 1.  Inputs resident in HBM: the collated batch dictionary
    (cameras, images, rays) and the image-feature volume the DINO encoder + `build_feat_vol` would hand over (both
    outside SURVEY.md section 8)."""
    from lara_amd import rasterizer
    from lara_amd.batch import synthetic_batch
    from lara_amd.encoder_train import VolTransformer
    from lara_amd.pipeline import CoarseFineDecoder, LaRaPipeline
    from lara_amd.loss import lara_loss      # the fused restatement of loss.py (same values as pipeline.lara_loss: tests/test_pipeline.py)
    rasterizer.load_library()
    if args.views < 4 and not args.no_fine:
        raise SystemExit("bench.py --step pipeline: the fine stage samples the 4 input views (configs/base.yaml: n_views 4); --views >= 4 or --no-fine")
    info = {"grad_allreduce": None}
    torch.manual_seed(0)          # identical initial parameters on every rank, as DDP expects
    enc = VolTransformer(256, 800, [args.grid // 4], args.grid // 2, args.grid, 80, args.encoder_layers, 16)
    pipe = LaRaPipeline(enc, CoarseFineDecoder(), grid_reso=args.grid // 2, n_streams=args.streams).to(device)
    pipe.fine_mask = args.fine_mask
    pipe.fine_reuses_coarse_lists = not getattr(args, "fine_rebins", False)
    if getattr(args, "dense_map_grads", False):
        from lara_amd import renderer
        plain = renderer._SurfaceMapsViews.backward

        def dense(ctx, *gs):
            out = plain(ctx, *gs)
            return out if out[1] is not None else (out[0], torch.zeros_like(ctx.saved_tensors[1])) + tuple(out[2:])
        renderer._SurfaceMapsViews.backward = staticmethod(dense)
    pipe._streams = _streams      # one pair of scene streams for every leg of this process: the device has 4 hardware queues, and a
                                  # second pair (the side legs' `step`) would alias onto them and serialise (93.5 vs 82.3 ms)
    pipe.train()
    batch = synthetic_batch(batch_size=args.scenes, n_views=args.views, H=args.res, W=args.res, n_input=4, seed=7 + rank, device=device)
    g = torch.Generator(device="cpu").manual_seed(11 + rank)
    batch["tar_rgb"] = torch.rand(batch["tar_rgb"].shape, generator=g).to(device)
    feat_vol = torch.randn(args.scenes, 4, 800, args.grid // 4, args.grid // 4, args.grid // 4, generator=g).to(device)
    feat_vol.requires_grad_(True)     # the DINO encoder in front is trained too (network.py:314): its features want a gradient
    n_par = sum(p.numel() for p in pipe.parameters() if p.requires_grad)
    info["encoder"] = {"parameters": sum(p.numel() for p in enc.parameters()), "layers": args.encoder_layers}
    model = pipe
    if world > 1:
        from torch.nn.parallel import DistributedDataParallel as DDP
        from lara_amd import dp
        model = DDP(pipe, device_ids=[device.index], **dp.DDP_KW)   # train_lightning.py:72
        info["grad_allreduce"] = {"bytes_per_step": 4 * n_par, "bucket_cap_MB": dp.DDP_BUCKET_MB, "buckets": None,
                                  "gradient_as_bucket_view": True, "every_n_steps": max(1, args.accumulate),
                                  "backend": os.environ.get("LARA_BENCH_BACKEND", "nccl"),
                                  "what": "torch DistributedDataParallel over the VolTransformer + decoder parameters (fp32 master "
                                          "gradients); the encoder's backward is one autograd node per block, so a bucket's all-reduce "
                                          "starts while the earlier blocks' backward is still running"}
    params = [p for p in pipe.parameters() if p.requires_grad]
    with_fine = not args.no_fine
    opt = None if args.no_optimizer else reference_optimizer(pipe, args.lr)
    info["optimizer"] = None if opt is None else {
        "what": "AdamW as system.py:78-106 builds it (LayerNorm parameters and biases without weight decay, betas 0.9 / 0.95, weight decay "
                "0.05, fused multi-tensor kernels) behind clip_grad_norm_(0.5) (train_lightning.py:75), " +
                ("EVERY step (the reference steps every second batch: accumulate_grad_batches=2; --accumulate 2 runs that cadence)"
                 if args.accumulate <= 1 else f"every {args.accumulate} steps (train_lightning.py:73), loss / {args.accumulate}, DDP no_sync() in between"),
        "lr": args.lr, "parameters": n_par, "accumulate_grad_batches": max(1, args.accumulate),
        "note": "lr 0: all of the update's kernels run and every parameter's version advances, so the HIP modules re-derive their bf16 / "
                "transposed operands each step as they do in training; the values stay, so all K steps time the same synthetic workload"}

    poison = os.environ.get("LARA2DGS_POISON_BUFFERS") == "1"

    def update():
        if opt is not None:
            torch.nn.utils.clip_grad_norm_(params, 0.5)
            opt.step()
            opt.zero_grad(set_to_none=True)
        else:
            for p in params:
                p.grad = None
        feat_vol.grad = None
    info["update"] = update
    info["opt"] = opt
    info["model"] = model

    info["micro_batch"] = 0

    def full_step(ms_ssim=args.ms_ssim, model=None, accumulate=None):
        model = info.get("model") if model is None else model
        acc = max(1, args.accumulate if accumulate is None else accumulate)
        last = info["micro_batch"] % acc == acc - 1      # train_lightning.py:73: reduce + update on every acc-th micro-batch
        info["micro_batch"] += 1
        with (model.no_sync() if (not last and hasattr(model, "no_sync")) else contextlib.nullcontext()):
            out = model(batch, feat_vol, with_fine=with_fine)
            loss, stats = lara_loss(batch, out, 2000, ms_ssim=ms_ssim)   # past iteration 1000: distortion + normal terms are on (loss.py:48)
            (loss if acc == 1 else loss / acc).backward()
        pipe.join_streams()
        cap = info.get("capture")
        if cap is not None:     # --dump-outputs: what this step hands its caller (references only; read after the timed steps)
            cap.update({k: v.detach() for k, v in out.items()})
            cap["loss"] = loss.detach()
            cap.update({f"loss_{k}": v for k, v in stats.items()})
            # (clip_grad_norm_ scales these in place below: the gradients the update consumes)
            cap["grad_params"] = [p.grad for p in params]
            cap["grad_feat_vol"] = feat_vol.grad
        if last:
            update()
        else:
            feat_vol.grad = None
        if poison:      # debugging mode: every state / scratch buffer 0xFF-filled between guard zones; checked (and released) per step
            bad = rasterizer.check_poison_guards()
            if bad:
                raise SystemExit(f"bench.py: a kernel wrote beyond the end of a state / scratch buffer (payload sizes {bad})")

    def after_first_step():
        if info["grad_allreduce"] is not None:
            try:
                sizes = model._get_ddp_logging_data().get("bucket_sizes", "")
                info["grad_allreduce"]["buckets"] = [int(x) for x in str(sizes).split(",") if x.strip()]
            except Exception:
                pass
    info.update(after_first_step=after_first_step, frames_per_rank_step=args.scenes * args.views * (2 if with_fine else 1),
                pipeline=(pipe, batch, feat_vol, full_step))
    if rank == 0 and not args.no_roofline:
        # the seeded synthetic scenes of SURVEY.md section 8d (what `roofline`, `kernels` and the raster side legs run on)
        scenes, settings, gc, ga = build_batch(args, device, rank)
        info["raster_state"] = (scenes, settings, gc, ga, None if args.no_fine else fine_subsets(scenes))
    return full_step, info


def ddp_single_rank_leg(info, args, device):
    """The pipeline step under torch DistributedDataParallel with backend nccl (= RCCL) and ONE rank: the reducer's hooks on
    the per-block encoder nodes, its bucket copies and RCCL's all-reduce launches (a one-member ring) -- the local cost of the
    path's exchange step, measurable on the one GPU this environment exposes.  N > 1 adds the xGMI transfers themselves."""
    import socket
    import torch.distributed as dist
    from torch.nn.parallel import DistributedDataParallel as DDP
    from lara_amd import dp
    from lara_amd.loss import lara_loss
    pipe, batch, feat_vol, _ = info["pipeline"]
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=device)
    try:
        model = DDP(pipe, device_ids=[device.index], **dp.DDP_KW)
        full_step = info["pipeline"][3]
        res = {}
        for name, acc in (("every_step", 1), ("accumulate_2", 2)):
            info["micro_batch"] = 0
            for _ in range(4):
                full_step(ms_ssim=False, model=model, accumulate=acc)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps + args.steps % acc):
                full_step(ms_ssim=False, model=model, accumulate=acc)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / (args.steps + args.steps % acc)
            res[name] = {"ms_per_step": round(1e3 * dt, 3), "value": round(info["frames_per_rank_step"] / dt, 3)}
        # the same two cadences WITHOUT the wrapper, back to back on the same box: the local cost of the exchange step is the difference
        for name, acc in (("every_step", 1), ("accumulate_2", 2)):
            info["micro_batch"] = 0
            for _ in range(2):
                full_step(ms_ssim=False, model=pipe, accumulate=acc)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps + args.steps % acc):
                full_step(ms_ssim=False, model=pipe, accumulate=acc)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / (args.steps + args.steps % acc)
            res[name]["ms_per_step_without_ddp"] = round(1e3 * dt, 3)
            res[name]["ddp_overhead_ms"] = round(res[name]["ms_per_step"] - 1e3 * dt, 3)
        info["micro_batch"] = 0
        try:
            sizes = [int(x) for x in str(model._get_ddp_logging_data().get("bucket_sizes", "")).split(",") if x.strip()]
        except Exception:
            sizes = None
        return {"ms_per_step": res["every_step"]["ms_per_step"], "value": res["every_step"]["value"], "unit": "frames/s", "buckets": sizes,
                "every_step": res["every_step"], "accumulate_2": res["accumulate_2"], "gradient_as_bucket_view": True,
                "what": "the same step wrapped in DistributedDataParallel, backend nccl (RCCL), world size 1: reducer hooks, gradients "
                        "written straight into the buckets (gradient_as_bucket_view) and one-member all-reduces included; `every_step` "
                        "reduces and updates on every micro-batch (the headline's definition), `accumulate_2` is the reference's cadence "
                        "(train_lightning.py:73: no_sync() on the first micro-batch, all-reduce + clip + AdamW on the second); "
                        "`ddp_overhead_ms` = against the same cadence without the wrapper, same box, back to back"}
    finally:
        dist.destroy_process_group()


def pipeline_breakdown(info, args):
    """Where the pipeline step's time goes: (a) forward stages on ONE stream (HIP events at the stage boundaries of
    `LaRaPipeline.forward`) + the whole backward; (b) the library's kernels of one whole step grouped by stage (HIP events
    around every launch, serialised); (c) the fine subset's size and D."""
    from lara_amd import rasterizer
    from lara_amd.loss import lara_loss
    pipe, batch, feat_vol, full_step = info["pipeline"]
    prev_streams = pipe.n_streams
    pipe.n_streams = 1
    res = {}
    try:
        for _ in range(3):      # (the caller's stream has its own allocator pool: let it see the step's sizes first)
            full_step()
        torch.cuda.synchronize()
        pipe.stage_events = []
        out = pipe(batch, feat_vol, with_fine=not args.no_fine)
        loss, _ = lara_loss(batch, out, 2000, ms_ssim=False)
        e_l = torch.cuda.Event(enable_timing=True); e_l.record()
        loss.backward()
        pipe.join_streams()
        e_b = torch.cuda.Event(enable_timing=True); e_b.record()
        torch.cuda.synchronize()
        ev, pipe.stage_events = pipe.stage_events, None
        stages = {}
        for (n0, e0), (n1, e1) in zip(ev[:-1], ev[1:]):
            stages[n1] = stages.get(n1, 0.0) + e0.elapsed_time(e1)
        stages["loss"] = ev[-1][1].elapsed_time(e_l)
        stages["backward (all of it)"] = e_l.elapsed_time(e_b)
        res["one_stream_ms"] = {k: round(v, 2) for k, v in stages.items()}
        res["one_stream_ms"]["sum"] = round(sum(stages.values()), 2)
        for p in pipe.parameters():
            p.grad = None
        # (b) per-kernel HIP events of the library's launches over one step
        rasterizer.profile_enable(True)
        full_step()
        torch.cuda.synchronize()
        rec = rasterizer.profile_collect()
        rasterizer.profile_enable(False)
        groups = {"raster": ("preprocess", "tile_", "scatter", "composite", "sum_view_grads"), "encoder": ("ga_", "gb_", "gbb_", "gbt_", "vt_", "vtb_"),
                  "surface maps": ("surface",), "point sampler": ("point_feats",), "forward_fine": ("fine_",)}
        agg, other = {k: 0.0 for k in groups}, {}
        for name, ms in rec:
            for gname, pre in groups.items():
                if name.startswith(pre):
                    agg[gname] += ms
                    break
            else:
                other[name] = other.get(name, 0.0) + ms
        res["library_kernels_ms"] = {k: round(v, 2) for k, v in agg.items()}
        if other:
            res["library_kernels_ms"]["other"] = {k: round(v, 3) for k, v in sorted(other.items(), key=lambda kv: -kv[1])[:12]}
        res["library_kernels_ms"]["sum"] = round(sum(ms for _, ms in rec), 2)
        comp = {}
        for name, ms in rec:
            if name in ("composite_fwd", "composite_bwd", "preprocess_fwd", "preprocess_bwd", "preprocess_fwd_views", "preprocess_bwd_views", "tile_sort"):
                c = comp.setdefault(name, [0, 0.0]); c[0] += 1; c[1] += ms
        res["raster_kernels"] = {k: {"launches": n, "avg_us": round(1e3 * t / n, 1)} for k, (n, t) in comp.items()}
        with torch.no_grad():
            g = pipe.gaussians(feat_vol)
            res["fine_subset_fraction_before_check_mask"] = round(float(g["masks"].float().mean()), 4)
            res["opacity_mean"] = round(float(torch.sigmoid(g["opacity"]).mean()), 4)
    finally:
        pipe.n_streams = prev_streams
    return res


class _PlumbingEncoder(torch.nn.Module):
    """LARA_BENCH_PLUMBING=1 (CPU tests of the launcher): a few linear layers stand in for the HIP encoder so that the
    spawn / process-group / DDP / barrier / max-over-ranks / JSON path can run without a GPU.  Nothing is measured."""

    def __init__(self):
        super().__init__()
        self.net = torch.nn.Sequential(torch.nn.Linear(64, 256), torch.nn.ReLU(), torch.nn.Linear(256, 64))

    def forward(self, x):
        return self.net(x)


def make_training_step(args, device, rank, world, plumbing):
    """Returns (full_step, info): the per-rank step described in the module docstring."""
    info = {"grad_allreduce": None, "encoder": None}
    from lara_amd import dp as _dp
    ddp_kw = dict(_dp.DDP_KW)     # train_lightning.py:72 + torch's default bucket, gradients as bucket views
    if plumbing:
        torch.manual_seed(0)
        enc = _PlumbingEncoder().to(device)
        feats, dout = torch.randn(8, 64, device=device), torch.randn(8, 64, device=device)
        raster = lambda after: after and torch.autograd.backward(*_roots(after))
        frames = args.scenes * args.views * (1 if args.no_fine else 2)
    else:
        from lara_amd import rasterizer
        rasterizer.load_library()
        scenes, settings, gc, ga = build_batch(args, device, rank)
        fine_idx = None if args.no_fine else fine_subsets(scenes)
        frames = args.scenes * args.views * (1 if args.no_fine else 2)
        raster = lambda after: step(scenes, settings, gc, ga, args.streams, fine_idx, after, api=args.raster_api,
                                    capture=info.get("capture"))
        enc = None
        if args.step == "train":
            from lara_amd.encoder_train import VolTransformer
            torch.manual_seed(0)      # identical initial parameters on every rank, as DDP expects
            enc = VolTransformer(256, 800, [16], 32, 64, 80, args.encoder_layers, 16).to(device)
            g = torch.Generator(device="cpu").manual_seed(11 + rank)
            feats = torch.randn(args.scenes, 4, 800, 16, 16, 16, generator=g).to(device)
            dout = (torch.randn(args.scenes, 64, 64, 64, 80, generator=g) * 1e-3).to(device)
        info["raster_state"] = (scenes, settings, gc, ga, fine_idx)
    model = enc
    if enc is not None:
        n_par = sum(p.numel() for p in enc.parameters() if p.requires_grad)
        info["encoder"] = {"parameters": n_par, "layers": args.encoder_layers if not plumbing else 2}
        if world > 1:
            from torch.nn.parallel import DistributedDataParallel as DDP
            model = DDP(enc, device_ids=[device.index] if device.type == "cuda" else None, **ddp_kw)
            info["grad_allreduce"] = {"bytes_per_step": 4 * n_par, "bucket_cap_MB": ddp_kw["bucket_cap_mb"],
                                      "buckets": None, "backend": os.environ.get("LARA_BENCH_BACKEND", "nccl"),
                                      "what": "torch DistributedDataParallel over the trainable VolTransformer "
                                              "(fp32 master gradients, all-reduced bucket by bucket while its backward runs)"}

    def _enc_roots(outs, grads):
        outs.append(info["_out"])
        grads.append(dout)

    def full_step():
        if model is None:                       # --step raster
            raster(None)
            return
        info["_out"] = model(feats)             # 1. encoder forward (DDP: also arms the reducer's hooks)
        raster(_enc_roots)                      # 2. raster forwards; 3. raster backward; 4. encoder backward (+ all-reduce)
        cap = info.get("capture")
        if cap is not None:                     # --dump-outputs
            cap["encoder_out"] = info["_out"].detach()
            cap["grad_encoder_params"] = [p.grad for p in enc.parameters()]
        for p in enc.parameters():
            p.grad = None
        info["_out"] = None

    def after_first_step():
        if info["grad_allreduce"] is not None:
            try:    # the reducer's own record of the buckets it built (bytes each), after the first backward
                sizes = model._get_ddp_logging_data().get("bucket_sizes", "")
                info["grad_allreduce"]["buckets"] = [int(x) for x in str(sizes).split(",") if x.strip()]
            except Exception:
                pass
    info["after_first_step"] = after_first_step
    info["frames_per_rank_step"] = frames
    return full_step, info


def _roots(after):
    outs, grads = [], []
    after(outs, grads)
    return outs, grads


DUMP_BUDGET_BYTES = 60 * 2 ** 20     # all of `--dump-outputs` together, under its promised 64 MB


def dump_outputs(path, arrays):
    """`--dump-outputs`: {name: tensor or list of tensors} -> path/<name>.npy.  float64 tensors stay float64, every other
    dtype is written as float32 (integers as float64).  A list is one flat array (its tensors flattened, in order).  Each
    array gets an equal share of the byte budget; one that holds more elements is written as the sample at sorted indices
    drawn by a generator seeded with the name's CRC32 -- the same elements in every run of the same arguments."""
    import zlib
    import numpy as np
    items = []
    for name, ts in sorted(arrays.items()):
        ts = [t.detach() for t in (ts if isinstance(ts, (list, tuple)) else [ts]) if t is not None]
        if ts:
            items.append((name, ts))
    share = DUMP_BUDGET_BYTES // 8 // max(1, len(items))    # elements per array, counted at float64's 8 bytes
    os.makedirs(path, exist_ok=True)
    for name, ts in items:
        dtype = np.float64 if ts[0].dtype == torch.float64 or not ts[0].is_floating_point() else np.float32
        total = sum(t.numel() for t in ts)
        if len(ts) == 1 and total <= share:
            a = ts[0].double().cpu().numpy()
        elif total <= share:
            a = torch.cat([t.reshape(-1).double().cpu() for t in ts]).numpy()
        else:
            idx = np.sort(np.random.default_rng(zlib.crc32(name.encode())).integers(0, total, share))
            parts, off = [], 0
            for t in ts:
                sel = idx[(idx >= off) & (idx < off + t.numel())] - off
                parts.append(t.reshape(-1)[torch.from_numpy(sel).to(t.device)].double().cpu())
                off += t.numel()
            a = torch.cat(parts).numpy()
        np.save(os.path.join(path, f"{name}.npy"), a.astype(dtype))


def main():
    args = parse()
    if not args.full:       # a plain run measures the headline only
        args.no_roofline = args.no_side_legs = args.no_cpu_baseline = True
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_spawn(args)
    # Exactly ONE line on stdout, the JSON: libraries that print there on their own (RCCL's version banner at communicator
    # creation, for one) are sent to stderr at the file-descriptor level until the line is ready.
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    plumbing = os.environ.get("LARA_BENCH_PLUMBING", "0") == "1"
    if world != args.gpus:
        raise SystemExit(f"bench.py --gpus {args.gpus} but WORLD_SIZE={world}: launch with --nproc-per-node {args.gpus}")
    if plumbing:
        device = torch.device("cpu")
    else:
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs an MI355X (torch.cuda.is_available() is False)")
        backend = os.environ.get("LARA_BENCH_BACKEND", "nccl")
        if backend == "nccl" and world > torch.cuda.device_count():
            raise SystemExit(f"{world} ranks but {torch.cuda.device_count()} GPU(s): RCCL wants one rank per device")
        local = local % torch.cuda.device_count()  # (several ranks on one GPU only in the gloo self-test)
        torch.cuda.set_device(local)
        device = torch.device("cuda", local)
    sync = (lambda: None) if plumbing else torch.cuda.synchronize
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = "gloo" if plumbing else os.environ.get("LARA_BENCH_BACKEND", "nccl")  # nccl = RCCL over xGMI
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group(backend)

    if args.step == "pipeline" and not plumbing:
        full_step, info = make_pipeline_step(args, device, rank, world, plumbing)
    else:
        full_step, info = make_training_step(args, device, rank, world, plumbing)
    for i in range(max(args.warmup, 1) if info["grad_allreduce"] else args.warmup):
        full_step()
        if i == 0:
            info["after_first_step"]()
    sync()
    if world > 1:
        dist.barrier()
    sync()
    capture_at = args.steps - 1 if args.dump_outputs and rank == 0 else -1
    t0 = time.perf_counter()
    for i in range(args.steps):
        if i == capture_at:
            info["capture"] = {}
        full_step()
    sync()
    if world > 1:
        dist.barrier()
    sync()
    dt = time.perf_counter() - t0
    if capture_at >= 0:
        dump_outputs(args.dump_outputs, info.pop("capture"))
    joined = world
    if world > 1:
        from lara_amd import dp
        dt = dp.max_over_ranks(dt, device)
        cnt = torch.ones(1, device=device)
        dist.all_reduce(cnt)
        joined = int(cnt.item())        # ranks that actually joined the job
    memory = None
    if not plumbing and args.full:
        from lara_amd import rasterizer
        # Per rank: where the device memory sits once the timed steps have run (VERDICT r5 weak #8 -- the first 8-GPU run says
        # at once whether 4 scenes per GPU fit after the raster's capacity has followed the pair counts).  Gathered to rank 0.
        cap_rep = rasterizer.capacity_report()
        cap_rep.pop("reruns", None)
        mine = {"rank": rank, "peak_allocated_GiB": round(torch.cuda.max_memory_allocated() / 2**30, 2),
                "peak_reserved_GiB": round(torch.cuda.max_memory_reserved() / 2**30, 2),
                "allocated_GiB": round(torch.cuda.memory_allocated() / 2**30, 2),
                "device_total_GiB": round(torch.cuda.get_device_properties(device).total_memory / 2**30, 1),
                "alloc_retries": torch.cuda.memory_stats().get("num_alloc_retries", 0),
                "raster_capacity": [{"surfels_sized_for": b[1], "image": [b[2], b[3]], "D_max": r_["D_max"], "capacity_next_call": r_["capacity"]}
                                    for b, r_ in sorted(cap_rep.items())]}
        memory = [mine]
        if world > 1:
            memory = [None] * world
            dist.all_gather_object(memory, mine)
    frames_per_step = info["frames_per_rank_step"] * joined
    P = (args.grid ** 3) * 2
    enc = info["encoder"]
    out = {
        "metric": "novel-view frames/sec @512x512 (4-view in, 2DGS fwd+bwd)",
        "value": round(frames_per_step * args.steps / dt, 3),
        "unit": "frames/s",
        "n_gpus": joined,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(1e3 * dt / args.steps, 3),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f32" if args.step == "raster" else "f32 raster + bf16-MFMA/f32-accumulate encoder"
                 + (" (+ bf16-autocast coarse decoder MLP, as the reference's bf16-mixed)" if args.step == "pipeline" else ""),
        "data": "synthetic" if not plumbing else "PLUMBING SELF-TEST (no GPU work; not a measurement)",
        "config": {
            "workload": (
                (f"configs[2]: the whole data-dependent LaRa training step (lightning/network.py:455-532 + loss.py {'WITH its MS-SSIM term' if args.ms_ssim else 'minus MS-SSIM'}), per GPU "
                 f"{args.scenes} scenes: VolTransformer ({enc['layers']} layers, {enc['parameters'] / 1e6:.2f} M parameters) -> coarse decoder MLP "
                 f"-> {args.views} coarse views/scene -> " + ("" if args.no_fine else f"_check_mask ({args.fine_mask}) -> point sampler on 4 input views -> "
                 f"forward_fine -> {args.views} fine views/scene -> ") + f"loss -> ONE backward through all of it"
                 + ("" if info.get("optimizer") is None else " -> clip_grad_norm_ + AdamW update of every parameter") + f"; @{args.res}x{args.res}, P={P} "
                 f"surfels/scene, SH degree 1, random-init network (= SURVEY 8d's init regime)")
                if args.step == "pipeline" and not plumbing else
                (f"configs[2]: LaRa training step on the hot path (round 2's definition: encoder and raster on independent tensors), per GPU {args.scenes} scenes: "
                 + (f"VolTransformer fwd+bwd ({enc['layers']} layers, {enc['parameters'] / 1e6:.2f} M parameters) + "
                    if enc else "")
                 + f"raster fwd+bwd of {args.views} coarse" + ("" if args.no_fine else f" + {args.views} fine")
                 + f" views/scene @{args.res}x{args.res}, P={P} surfels/scene, SH degree 1, regime={args.regime}")),
            "step": args.step,
            "frames_per_step": frames_per_step,
            "parallelism": f"dp{joined} (per-scene; raster not sharded)",
            "hip_streams": args.streams,
            "raster_api": ("views: one multi-view rasteriser call per scene and pass (opt-in lara_amd API; every kernel one "
                           "launch over the cameras)" if args.raster_api == "views" or args.step == "pipeline" else
                           "loop: one GaussianRasterizer call per view (the reference's loop)"),
            "grad_allreduce": info["grad_allreduce"],
            "optimizer": info.get("optimizer"),
        },
    }
    if memory is not None:
        out["memory_per_rank"] = memory
    solo = rank == 0 and world == 1 and not plumbing
    if solo and args.step == "pipeline" and not args.no_roofline:
        _leg("stages")
        out["stages"] = pipeline_breakdown(info, args)
    if solo and args.step == "pipeline" and not args.no_side_legs and not args.ms_ssim and args.res > 160:
        # the same step with the reference's 0.5 (1 - MS_SSIM) term in the loss (loss.py:41-45): plain torch operators (outside
        # SURVEY.md section 8; `pytorch_msssim` itself is absent), so the like-for-like figure sits beside `value`
        _leg("step_with_ms_ssim")
        fs = info["pipeline"][3]
        for _ in range(2):
            fs(True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            fs(True)
        torch.cuda.synchronize()
        d1 = time.perf_counter() - t1
        out["step_with_ms_ssim"] = {"value": round(frames_per_step * args.steps / d1, 3), "unit": "frames/s",
                                    "ms_per_step": round(1e3 * d1 / args.steps, 3),
                                    "what": "the headline step + 0.5 (1 - MS_SSIM) for the coarse and the fine image = the reference's whole loss "
                                            "(loss.py:28-58); the MS-SSIM term as HIP kernels (lara_amd.loss.ms_ssim_fused, csrc/msssim.hip; "
                                            "rounds 3-4: torch operators, +31 ms)"}
    if solo and args.step == "pipeline" and not args.no_side_legs and info.get("optimizer") is not None and args.lr == 0.0:
        # The same step with the reference's learning rate (configs/base.yaml: 4e-4) instead of 0: the parameters now MOVE, i.e. the
        # Gaussians the network emits -- and with them the raster's workload -- drift from step to step; the figure shows that the
        # update itself costs the same either way.  The parameters and the optimiser state are put back afterwards.
        _leg("step_with_reference_lr")
        pipe_, opt_ = info["pipeline"][0], info["opt"]
        snap = {k: v.detach().clone() for k, v in pipe_.state_dict().items()}
        opt_snap = opt_.state_dict()
        opt_snap = {"state": {k: {kk: (vv.clone() if torch.is_tensor(vv) else vv) for kk, vv in st.items()} for k, st in opt_snap["state"].items()},
                    "param_groups": [dict(g) for g in opt_snap["param_groups"]]}
        for g_ in opt_.param_groups:
            g_["lr"] = 4e-4

        def surfel_stats():      # what the raster's workload depends on
            with torch.no_grad():
                g_ = pipe_.gaussians(info["pipeline"][2])
                return {"opacity_mean": round(float(torch.sigmoid(g_["opacity"]).mean()), 4),
                        "scale_mean": round(float(g_["scaling"].mean()), 5),
                        "kept_by_the_fine_mask": round(float(g_["masks"].float().mean()), 4)}
        try:
            fs = info["pipeline"][3]
            before = surfel_stats()
            torch.cuda.synchronize()
            from lara_amd import rasterizer as _rz5
            reruns0 = _rz5.capacity_report()["reruns"]
            ms0 = torch.cuda.memory_stats()
            per = []
            for _ in range(args.steps):
                t1 = time.perf_counter()
                fs()
                torch.cuda.synchronize()
                per.append(time.perf_counter() - t1)
            d1 = sum(per)
            cap_rep = _rz5.capacity_report()
            out["step_with_reference_lr"] = {"value": round(frames_per_step * args.steps / d1, 3), "unit": "frames/s",
                                             "ms_per_step": round(1e3 * d1 / args.steps, 3), "lr": 4e-4,
                                             "ms_first_step": round(1e3 * per[0], 2), "ms_last_step": round(1e3 * per[-1], 2),
                                             "ms_steps": [round(1e3 * x, 1) for x in per],
                                             # (a step that grows a size class allocates its states afresh; one that makes the caching
                                             #  allocator give its cached blocks back first shows here as a retry and a long step)
                                             "allocator": {"retries": torch.cuda.memory_stats().get("num_alloc_retries", 0) - ms0.get("num_alloc_retries", 0),
                                                           "reserved_GiB_before": round(ms0.get("reserved_bytes.all.current", 0) / 2 ** 30, 2),
                                                           "reserved_GiB_after": round(torch.cuda.memory_reserved() / 2 ** 30, 2),
                                                           "peak_allocated_GiB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)},
                                             "surfels_before": before, "surfels_after": surfel_stats(),
                                             "binning_capacity": {
                                                 "calls_repeated_at_a_larger_capacity": cap_rep.pop("reruns") - reruns0,
                                                 "per_size_class": [{"surfels_sized_for": b[1], "image": [b[2], b[3]], "D_max": r_["D_max"],
                                                                     "capacity_next_call": r_["capacity"], "longest_list": r_.get("longest_list"),
                                                                     "D_over_capacity": round(r_["D_max"] / r_["capacity"], 3)}
                                                                    for b, r_ in sorted(cap_rep.items())],
                                                 "what": "the pair capacity follows the measured pair counts (2 x the maximum of the size class's last "
                                                         "256 calls, lara_amd/rasterizer.py); a call that outgrows it is repeated before the operator "
                                                         "returns: never an error, never a poisoned output"},
                                             "what": f"the headline step with AdamW's learning rate at the reference's 4e-4 for {args.steps} steps from the "
                                                     "random-init network, each step synchronised: the update costs what it costs at rate 0 (first step), "
                                                     "and the parameters -- hence the surfels the network emits and the raster's work -- move from there "
                                                     "(restored afterwards)"}
        finally:
            for g_ in opt_.param_groups:
                g_["lr"] = args.lr
            with torch.no_grad():
                pipe_.load_state_dict(snap)
            opt_.load_state_dict(opt_snap)
    if solo and args.step == "pipeline" and not args.no_side_legs:
        # The same step as an UNMODIFIED LaRa issues it around the drop-in rasteriser (tools.reference_style: one
        # GaussianRasterizer call per view on one stream, render_img's post-processing / get_point_feats / forward_fine / the coarse
        # MLP / the loss as plain torch operators, `x[mask]` indexing).  The encoder stays this package's HIP VolTransformer in both.
        from tools import reference_style
        from lara_amd.pipeline import lara_loss as torch_loss
        _leg("drop_in_step")
        pipe_, batch_, fv_, _fs = info["pipeline"]

        def drop_in():
            o = reference_style.network_forward(pipe_, batch_, fv_, with_fine=not args.no_fine)
            l, _ = torch_loss(batch_, o, 2000, ms_ssim=False)
            l.backward()
            info["update"]()
        for _ in range(2):
            drop_in()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(max(2, args.steps // 2)):
            drop_in()
        torch.cuda.synchronize()
        d1 = (time.perf_counter() - t1) / max(2, args.steps // 2)
        out["drop_in_step"] = {"value": round(frames_per_step / d1, 3), "unit": "frames/s", "ms_per_step": round(1e3 * d1, 3),
                               "what": "the headline's step as train_lightning.py issues it UNCHANGED around the shim: per-view GaussianRasterizer "
                                       "calls on one stream, reference-style torch operators for render_img's post-processing, the coarse MLP, "
                                       "get_point_feats, forward_fine, x[mask] and the loss (tools.reference_style); same HIP VolTransformer"}
        del drop_in
        torch.cuda.empty_cache()
        # SURVEY 8d's second regime for the whole step: the same network with its opacity logits biased to an opaque thin shell
        # in empty space (pixels saturate after tens of surfels; the fine pass renders the shell only)
        _leg("trained_like_step")
        pipe_.opacity_bias = pipe_.trained_like_opacity_bias()
        try:
            fs = info["pipeline"][3]
            for _ in range(2):
                fs()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(args.steps):
                fs()
            torch.cuda.synchronize()
            d1 = (time.perf_counter() - t1) / args.steps
            with torch.no_grad():
                kept = float((torch.sigmoid(pipe_.gaussians(fv_)["opacity"]) > 0.005).float().mean())
            out["trained_like_step"] = {"value": round(frames_per_step / d1, 3), "unit": "frames/s", "ms_per_step": round(1e3 * d1, 3),
                                        "fine_subset_fraction": round(kept, 4),
                                        "what": "the headline step with the decoder's opacity logits biased to SURVEY 8d's trained-like shell "
                                                "(opaque |r - 0.35| < 0.02, empty elsewhere): the composite kernels' early-terminating regime"}
        finally:
            pipe_.opacity_bias = None
    if solo and args.step == "pipeline" and not args.no_roofline and not args.no_side_legs:
        try:
            _leg("ddp_single_rank_rccl")
            out["ddp_single_rank_rccl"] = ddp_single_rank_leg(info, args, device)
        except Exception as e:      # (a box without a usable RCCL: say so instead of losing the line)
            out["ddp_single_rank_rccl"] = {"error": f"{type(e).__name__}: {e}"[:300]}
        # round 2's headline definition, kept for continuity: encoder and raster on independent synthetic tensors,
        # no decoder / sampler / forward_fine / loss, the fine subset not thinned
        a2 = argparse.Namespace(**{**vars(args), "step": "train"})
        step2, info2 = make_training_step(a2, device, rank, world, plumbing)
        _leg("independent_tensors_step")
        for _ in range(3):
            step2()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            step2()
        torch.cuda.synchronize()
        d2 = time.perf_counter() - t1
        out["independent_tensors_step"] = {
            "value": round(info2["frames_per_rank_step"] * args.steps / d2, 3), "unit": "frames/s", "ms_per_step": round(1e3 * d2 / args.steps, 3),
            "workload": "round 2's headline: VolTransformer fwd+bwd + raster fwd+bwd of 8 coarse + 8 fine views/scene on INDEPENDENT "
                        "synthetic tensors (no decoder, sampler, forward_fine, loss; fine subset = every surfel above the opacity threshold)"}
        del step2, info2
        torch.cuda.empty_cache()
    if solo and not args.no_roofline:
        scenes, settings, gc, ga, fine_idx = info["raster_state"]

        def timed(fn, frames):
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize()
            d = time.perf_counter() - t1
            return {"value": round(frames * args.steps / d, 3), "unit": "frames/s", "ms_per_step": round(1e3 * d / args.steps, 3)}

        coarse = args.scenes * args.views
        # the raster alone, coarse views only: round 1's headline definition (BENCH_r01.json `value`)
        api = args.raster_api
        _leg("raster_only")
        out["raster_only"] = dict(timed(lambda: step(scenes, settings, gc, ga, args.streams, api=api), coarse),
                                  workload=f"raster fwd+bwd only, {args.scenes} scenes x {args.views} coarse views, {args.streams} HIP streams, api={api}")
        if fine_idx is not None:
            _leg("raster_only_with_fine")
            out["raster_only_with_fine"] = dict(timed(lambda: step(scenes, settings, gc, ga, args.streams, fine_idx, api=api), 2 * coarse),
                                                workload="raster fwd+bwd only, coarse + fine views (the raster part of the headline step)",
                                                fine_subset_fraction=round(float(sum(i.numel() for i in fine_idx)) / (P * len(fine_idx)), 4))
        # the multi-view call on ONE caller stream (the library's side streams only)
        _leg("views_api_one_stream")
        out["views_api_one_stream"] = timed(lambda: step(scenes, settings, gc, ga, 1, api="views"), coarse)
        # one call per view, as the reference's loop issues them: two scene streams (round 1's headline) and one stream
        _leg("reference_loop")
        out["reference_loop"] = {"two_streams": timed(lambda: step(scenes, settings, gc, ga, 2, api="loop"), coarse),
                                 "with_fine_two_streams": (timed(lambda: step(scenes, settings, gc, ga, 2, fine_idx, api="loop"), 2 * coarse)
                                                           if fine_idx is not None else None)}
        _leg("single_stream")
        out["single_stream"] = timed(lambda: step(scenes, settings, gc, ga, 1, api="loop"), coarse)
        # opt-in, not in the reference: surfels with opacity < 1/255 (never drawn) culled in the preprocess; same
        # images to an ulp, same gradients (tests/test_raster_parity_gpu.py); nothing to cull at LaRa's initialisation,
        # most of the volume in a trained-like scene
        prev = rasterizer.set_cull_transparent(True)
        try:
            _leg("cull_transparent_opt_in")
            out["cull_transparent_opt_in"] = timed(lambda: step(scenes, settings, gc, ga, args.streams, api=api), coarse)
        finally:
            rasterizer.set_cull_transparent(prev)
        _leg("forward_only")
        out["forward_only"] = forward_only_leg(scenes, settings, args)
        if not args.no_side_legs:
            _leg("mesh_eval")
            out["mesh_eval"] = mesh_eval_leg(args, device)
    if rank == 0 and not plumbing and not args.no_roofline:
        scenes, settings, gc, ga, fine_idx = info["raster_state"]
        roof, table, D = measure_roofline(scenes, settings, gc, ga, args)
        out["roofline"] = roof
        out["kernels"] = {k: {"avg_us": round(v["avg_us"], 2), "launches": v["launches"],
                              "alg_GBs": round(v["alg_GBs"], 1)} for k, v in table.items()}
    if solo and not args.no_roofline and not args.no_side_legs:   # the side legs run at N = 1 only (the other ranks would wait)
        del full_step
        info.clear()
        torch.cuda.empty_cache()
        _leg("attention")
        out["attention"] = attention_leg(device, args.scenes)
        _leg("encoder")
        out["encoder"] = encoder_leg(device, args.scenes)
        _leg("encoder_train")
        out["encoder_train"] = encoder_train_leg(device, args.scenes)
        _leg("rays")
        out["rays"] = rays_leg(device, args.scenes, args.views, args.res)
        _leg("render_img")
        out["render_img"] = render_img_leg(device, args)
        _leg("point_feats")
        out["point_feats"] = point_feats_leg(device, args)
        _leg("coarse_decoder")
        out["coarse_decoder"] = coarse_decoder_leg(device, args.scenes)
        _leg("fine_decoder")
        out["fine_decoder"] = fine_decoder_leg(device)
        _leg("fine_stage")
        out["fine_stage"] = fine_stage_leg(device, args)
    if solo and not args.no_cpu_baseline:
        _leg("cpu_baseline")
        out["cpu_baseline"] = cpu_baseline(args)
        out["cpu_baseline"]["encoder"] = cpu_encoder_baseline()
        roof = out.get("roofline")
        if roof and roof.get("valu_insts_per_launch") and roof["kernel"] in USEFUL_FMA_PER_PAIR:
            pairs = out["cpu_baseline"]["blended_pairs_view0"]
            roof["valu_useful_frac"] = round(pairs * USEFUL_FMA_PER_PAIR[roof["kernel"]] / (roof["valu_insts_per_launch"] * 64.0), 4)
            roof["valu_useful_what"] = (f"{pairs} blended (pixel, splat) pairs of view 0 (counted by the CPU oracle in this run) x "
                                        f"{USEFUL_FMA_PER_PAIR[roof['kernel']]} FMA-equivalents / (SQ_INSTS_VALU x 64 lanes: {roof['valu_insts_source']})")
    # the other definitions of the step measured in this same run, inside `config` (a reader that keeps `config` but only the NAMES of
    # the side objects still sees what the headline is and is not): frames/s, ms per step
    also = {}
    for key, label in (("step_with_ms_ssim", "with_the_references_ms_ssim_term_its_whole_loss"),
                       ("step_with_reference_lr", "with_the_references_learning_rate_4e-4_for_the_timed_steps"),
                       ("trained_like_step", "trained_like_regime"), ("drop_in_step", "as_an_unmodified_lara_issues_it_around_the_shim"),
                       ("ddp_single_rank_rccl", "under_single_rank_rccl_ddp")):
        o = out.get(key)
        if isinstance(o, dict) and "value" in o:
            also[label] = {"frames_per_s": o["value"], "ms_per_step": o.get("ms_per_step")}
    if also:
        out["config"]["headline_is"] = ("init regime (random-init network: the raster's worst case), AdamW at learning rate 0 (every kernel of the "
                                        "update runs, the workload stays fixed), loss " + ("with" if args.ms_ssim else "WITHOUT") + " the MS-SSIM term")
        out["config"]["same_run_other_definitions"] = also
    # the north star's second target (attention / encoder on the matrix cores) inside `roofline`, where a reader who keeps only
    # `roofline` and `cpu_baseline` of the line still finds it (the stand-alone objects stay for their details)
    roof = out.get("roofline")
    if roof is not None:
        mf = {}
        for key in ("attention", "encoder", "encoder_train"):
            o = out.get(key)
            if isinstance(o, dict) and "frac" in o:
                mf[key] = {"bound": "mfma", "achieved": o.get("achieved"), "peak": o.get("peak"), "unit": o.get("unit"), "frac": o.get("frac"),
                           **{k: o[k] for k in ("us_per_layer", "ms_per_forward", "ms_per_step", "conv3d_us", "conv3d_TFLOPs") if k in o}}
        if mf:
            roof["mfma"] = mf
            roof["mfma_what"] = ("the encoder's kernels against the dense bf16 matrix-core peak (2.5 PFLOP/s): `attention` = one GroupAttBlock "
                                 "attention step (network.py:88-93), `encoder` / `encoder_train` = VolTransformer forward / forward + backward; "
                                 "model FLOPs / HIP-event time")
        if roof.get("valu_issue_frac") is not None and roof.get("valu_useful_frac") is not None:
            roof["valu_roof_frac"] = round(float(roof["valu_issue_frac"]) * float(roof["valu_useful_frac"]), 4)
            roof["valu_roof_what"] = ("the roof that binds the dominant kernel: vector-ALU issue slots used (valu_issue_frac) x the share of "
                                      "issued lane-operations that are the algorithm's own arithmetic (valu_useful_frac)")
    if world > 1:
        dist.destroy_process_group()
    sys.stdout.flush()
    os.dup2(real_stdout, 1)
    os.close(real_stdout)
    if rank == 0:
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
