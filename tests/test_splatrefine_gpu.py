"""`lara_amd.splatrefine` on the device: the kernel's words equal the host entry's on every case of the CPU tests (twice, on a side
stream, carved out of sentinel-filled buffers, the counter included); `SurfelAdam.step` advances the version counters, so a second
render of the same tensors is not the cached one; sparse steps leave surfels no camera sees untouched; `refine` brings a perturbed
cloud's image error below half, as the control with ``torch.optim.Adam`` does; tools/refine_surfels.py.  The figures the tests print, as measured at writing: profiles/splatrefine_parity.txt."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import splatrefine_cases as C
from tests import splatrefine_restate as S
from tests.test_splatrefine import CARVE_OFFSETS, carved, host_step, sentinels_kept, tensors

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
SIZE, VIEWS = 64, 4
FOV, NEAR, FAR = 0.75, 0.5, 2.5

_shared = {}


def _words(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------ kernel bits

@pytest.mark.parametrize("degree", C.DEGREES)
def test_the_kernel_equals_the_host_entry_bit_for_bit(hip_lib, degree):
    from lara_amd import splatrefine as R
    side = torch.cuda.Stream(DEV)
    for P, d, t, moments, sparse in C.all_cases():
        if d != degree:
            continue
        parts = C.case(P, d, moments, seed=P + d)
        row = R.plan(t, C.LRS)
        visible = C.mask(P, seed=d) if sparse else None
        want, skipped = host_step(parts, row, visible, zero_grads=sparse)
        want = [S.words(x.numpy()) for ts in want for x in ts]
        flat = [a[k] for a in parts for k in C.FIELDS]
        with torch.cuda.stream(side):
            for attempt in range(2):
                vis = None if visible is None else torch.from_numpy(visible).to(DEV)
                p, g, m, v = tensors(parts, DEV)
                counters = R.adam_step(p, g, m, v, row, visible=vis, zero_grads=sparse)
                views, wholes = carved(flat, CARVE_OFFSETS, DEV)
                counters2 = torch.full((1,), 1000, dtype=torch.int64, device=DEV)
                R.adam_step(views[0:5], views[5:10], views[10:15], views[15:20], row, visible=vis, zero_grads=sparse, counters=counters2)
                side.synchronize()
                assert int(counters) == skipped and int(counters2) == 1000 + skipped, (P, d, t, moments, sparse, attempt)
                for i, (a, b, w) in enumerate(zip(p + g + m + v, views, want)):
                    assert np.array_equal(_words(a), w), (P, d, t, moments, sparse, attempt, i)
                    assert np.array_equal(_words(b), w), (P, d, t, moments, sparse, attempt, i, "carved")
                assert sentinels_kept(wholes, CARVE_OFFSETS, P), (P, d, t, moments, sparse, attempt)
    empty = R.adam_step(*tensors(C.case(0, degree, False), DEV), R.plan(1), zero_grads=True)
    assert empty.is_cuda and int(empty) == 0


# ------------------------------------------------------------------------------------------------------------------ the scene

def _scene():
    """1 024 surfels of SH degree 1 on the device, four 64 x 64 turntable cameras with their rays, one renderer, the targets: once."""
    if not _shared:
        from lara_amd import cameras, splatio, synthetic
        from lara_amd.batch import build_rays, fov_to_ixt
        from lara_amd.renderer import Renderer
        sc = synthetic.make_scene(grid=8, K=2, regime="trained", sh_coeffs=4, device=DEV)
        cloud = splatio.SurfelCloud(*(sc[k].contiguous() for k in C.FIELDS))
        assert cloud.n_surfels == 1024 and cloud.sh_degree == 1
        c2w = cameras.turntable_c2w(VIEWS)
        cams = cameras.make_cameras(c2w, SIZE, SIZE, FOV, FOV, NEAR, FAR, device=DEV)
        rays = build_rays(c2w.float().to(DEV), fov_to_ixt(torch.tensor([[FOV, FOV]] * VIEWS), (SIZE, SIZE)).to(DEV), SIZE, SIZE)
        _shared.update(cloud=cloud, c2w=c2w, cams=cams, rays=rays, renderer=Renderer(sh_degree=1, white_background=True))
        _shared["targets"] = _image(cloud.render_args()).view(SIZE, VIEWS, SIZE, 3).permute(1, 0, 2, 3).contiguous()
        assert (_shared["targets"] != 1.0).float().mean() > 0.05                      # a picture, not the background
    return _shared


def _image(args, renderer=None):
    """The concatenated image [H, V W, 3] of five tensors, without a graph."""
    s = _shared
    with torch.no_grad():
        return (renderer or s["renderer"]).render_views(s["cams"], s["rays"], *args, DEV, concat=True)["image"].clone()


def _mse(args):
    s = _scene()
    img = _image(args).view(SIZE, VIEWS, SIZE, 3).permute(1, 0, 2, 3)
    return float(((img.double() - s["targets"].double()) ** 2).mean())


def _render_and_backward(opt, s):
    """One render of the optimiser's tensors, the loss against the targets, backward: (image, radii [V,P])."""
    from lara_amd import splatrefine as R
    raster_out = []
    out = s["renderer"].render_views(s["cams"], s["rays"], *opt.params(), DEV, concat=True, raster_out=raster_out)
    loss, _ = R._default_loss({"tar_rgb": s["targets"][None]}, {k: t[None] for k, t in out.items()}, 0)
    loss.backward()
    return out["image"].detach().clone(), raster_out[0][1]


def _perturbed(s, seed=11, sh0=0.3, opacity=0.7):
    """The scene's cloud with seeded noise on SH coefficient 0 and on the opacity logit only."""
    from lara_amd import splatio
    g = torch.Generator().manual_seed(seed)
    c = s["cloud"]
    shs, op = c.shs.clone(), c.opacity.clone()
    shs[:, 0, :] += (torch.randn(c.n_surfels, 3, generator=g) * sh0).to(DEV)
    op += (torch.randn(c.n_surfels, 1, generator=g) * opacity).to(DEV)
    return splatio.SurfelCloud(c.centers, shs, op, c.scales, c.rotations)


# ------------------------------------------------------------------------------------------------------------------ the version counter

def test_a_render_after_a_step_is_not_the_cached_one(hip_lib):
    """Only opacity, scales and rotations move here (the rates of centres and SH coefficients are 0), so the picture can change
    through the renderer's activations alone: with the cached sigmoid / exp / normalize reused it would be the picture before."""
    from lara_amd import splatrefine as R
    from lara_amd.renderer import Renderer
    s = _scene()
    opt = R.SurfelAdam(_perturbed(s), lrs={"centers": 0.0, "sh0": 0.0, "sh_rest": 0.0, "opacity": 0.05, "scales": 0.01, "rotations": 0.01})
    before = [_words(p) for p in opt.params()]
    first, _ = _render_and_backward(opt, s)
    again = _image(opt.params())
    assert torch.equal(first, again)                                                   # same tensors, same versions: the same picture
    versions = [p._version for p in opt.params()]
    opt.step()
    torch.cuda.synchronize()
    assert all(p._version > v for p, v in zip(opt.params(), versions))
    assert [bool((_words(p) != b).any()) for p, b in zip(opt.params(), before)] == [False, False, True, True, True]
    second = _image(opt.params())
    assert not torch.equal(second, first) and float((second - first).abs().max()) > 1e-4
    fresh = _image(opt.cloud().render_args(), Renderer(sh_degree=1, white_background=True))
    assert torch.equal(second, fresh)                                                  # and it is the picture of the current values
    assert torch.equal(_image(opt.cloud().render_args()), fresh)


# ------------------------------------------------------------------------------------------------------------------ sparse semantics

def test_sparse_steps_leave_unseen_surfels_as_they_are(hip_lib):
    """The cloud extended by 64 surfels on the turntable's axis at z = 6..7: behind each of the four cameras (they sit at z = 0.86
    and look down at the origin; a point of the axis is behind them from z = 4.3 on)."""
    from lara_amd import splatio, splatrefine as R
    s = _scene()
    start = _perturbed(s)
    g = torch.Generator().manual_seed(3)
    extra = splatio.SurfelCloud(torch.cat([torch.rand(64, 2, generator=g) * 0.2 - 0.1, torch.rand(64, 1, generator=g) + 6.0], 1).to(DEV),
                                (torch.randn(64, 4, 3, generator=g) * 0.5).to(DEV), torch.full((64, 1), 2.0, device=DEV),
                                torch.full((64, 2), -3.0, device=DEV), torch.randn(64, 4, generator=g).to(DEV))
    cloud = splatio.concatenate([start, extra])
    P = cloud.n_surfels
    opt = R.SurfelAdam(cloud, sparse=True)
    before = [_words(p) for p in opt.params()]
    masks = []
    for _ in range(5):
        _, radii = _render_and_backward(opt, s)
        visible = (radii > 0).any(0)
        masks.append(visible)
        opt.step(visible, zero_grads=True)
    masks = torch.stack(masks).cpu().numpy()
    assert not masks[:, P - 64:].any()                                                 # visible was 0 for them in every step
    assert masks[:, :P - 64].any(0).sum() > 100
    for now, was in zip(list(opt.params()) + opt.exp_avg + opt.exp_avg_sq, before + [None] * 10):
        w = _words(now)
        assert np.array_equal(w[P - 64:], was[P - 64:]) if was is not None else not w[P - 64:].any()
    seen_always = masks[:, :P - 64].all(0)
    assert all((_words(p)[:P - 64][seen_always] != b[:P - 64][seen_always]).any() for p, b in zip(opt.params(), before))
    assert int(opt.skipped) == 0

    # refine() itself, sparse: the same rows stay
    refined, history = R.refine(cloud, s["cams"], s["rays"], s["targets"], steps=5, sparse=True, renderer=s["renderer"])
    for t, was in zip(refined.render_args(), before):
        assert np.array_equal(_words(t)[P - 64:], was[P - 64:])
    assert any((_words(t)[:P - 64] != was[:P - 64]).any() for t, was in zip(refined.render_args(), before))
    assert history["loss"].shape == (5,) and history["loss"].is_cuda and int(history["skipped"]) == 0

    # a surfel seen in step 1, then masked out by hand
    for sparse in (True, False):
        opt = R.SurfelAdam(cloud, sparse=sparse)
        _, radii = _render_and_backward(opt, s)
        visible = (radii > 0).any(0)
        j = int(opt.params()[2].grad.abs().view(-1).argmax())                          # the surfel whose opacity the picture asks most about
        assert bool(visible[j])
        opt.step(visible, zero_grads=True)
        after_one = [_words(t)[j].copy() for t in list(opt.params()) + opt.exp_avg + opt.exp_avg_sq]
        assert after_one[2] != before[2][j] and after_one[7].any() and after_one[12].any()         # its opacity and the moments moved
        _render_and_backward(opt, s)
        hand = visible.clone()
        hand[j] = False
        opt.step(hand)
        after_two = [_words(t)[j] for t in list(opt.params()) + opt.exp_avg + opt.exp_avg_sq]
        kept = [np.array_equal(a, b) for a, b in zip(after_one, after_two)]
        assert all(kept) if sparse else not (kept[2] or kept[7] or kept[12]), (sparse, kept)


# ------------------------------------------------------------------------------------------------------------------ refinement works

REFINE_STEPS = 40
REFINE_LRS = {"centers": 0.0, "sh0": 0.02, "sh_rest": 0.02, "opacity": 0.05, "scales": 0.0, "rotations": 0.0}


def test_refine_halves_the_image_error_as_the_control_does(hip_lib):
    """Targets: the scene's 1 024 surfels at 4 views of 64 x 64.  Start: that cloud with seeded noise on SH coefficient 0 (sigma
    0.3) and on the opacity logit (sigma 0.7).  40 dense steps of `refine` with rates 0.02 (SH) and 0.05 (opacity), everything else
    held, and the control: the same loop with ``torch.optim.Adam`` on the same leaf tensors.  Both final image MSEs must be below
    half of the starting one (a condition on the set-up; the two loops are not compared element by element).  The starting MSE is
    held above 1e-4: eight orders above what fp32 rounding of an image in 0..1 can give (1e-12).  Measured at writing on an MI355X:
    start 3.79e-4, control 4.42e-6, refine 4.42e-6."""
    from lara_amd import splatrefine as R
    s = _scene()
    start = _perturbed(s)
    mse_start = _mse(start.render_args())
    assert mse_start > 1e-4

    # the control
    leaves = [t.detach().clone().requires_grad_(True) for t in start.render_args()]
    control = torch.optim.Adam([{"params": [leaves[1]], "lr": REFINE_LRS["sh0"]}, {"params": [leaves[2]], "lr": REFINE_LRS["opacity"]}],
                               betas=(0.9, 0.999), eps=1e-15)
    for _ in range(REFINE_STEPS):
        out = s["renderer"].render_views(s["cams"], s["rays"], *leaves, DEV, concat=True)
        loss, _ = R._default_loss({"tar_rgb": s["targets"][None]}, {k: t[None] for k, t in out.items()}, 0)
        control.zero_grad()
        for t in leaves:
            t.grad = None
        loss.backward()
        control.step()
    mse_control = _mse([t.detach() for t in leaves])

    refined, history = R.refine(start, s["cams"], s["rays"], s["targets"], steps=REFINE_STEPS, lrs=REFINE_LRS, sparse=False,
                                renderer=s["renderer"])
    mse_device = _mse(refined.render_args())
    losses = history["loss"].cpu().numpy()
    print(f"splatrefine parity, refine at 4 views of 64 x 64, 1 024 surfels, {REFINE_STEPS} dense steps: image MSE start {mse_start:.4e}, "
          f"control (torch.optim.Adam) {mse_control:.4e}, refine {mse_device:.4e}; first and last loss {losses[0]:.4e}, {losses[-1]:.4e}; "
          f"non-finite gradient words skipped {int(history['skipped'])}")
    assert mse_control < 0.5 * mse_start, (mse_control, mse_start)
    assert mse_device < 0.5 * mse_start, (mse_device, mse_start)
    assert int(history["skipped"]) == 0
    assert history["mse"].shape == (REFINE_STEPS,) and abs(float(history["mse"][0]) - mse_start) < 1e-3 * mse_start
    for a, b in zip(refined.render_args(), start.render_args()):                       # the fields with rate 0 kept their words
        assert np.array_equal(_words(a), _words(b)) == (a.shape[1:] not in ((4, 3), (1,)))


# ------------------------------------------------------------------------------------------------------------------ the tool

def test_refine_surfels_tool_writes_a_better_cloud(hip_lib, tmp_path):
    from lara_amd import splatio
    s = _scene()
    start = _perturbed(s)
    ply, views, out = str(tmp_path / "start.ply"), str(tmp_path / "views.npz"), str(tmp_path / "refined.ply")
    splatio.write_ply(ply, start)
    np.savez(views, images=(s["targets"].cpu().numpy() * 255.0 + 0.5).astype(np.uint8), c2w=s["c2w"].numpy(), fovx=FOV, fovy=FOV,
             znear=NEAR, zfar=FAR)
    # a fresh child process under its own time limit; nothing below runs when it fails
    run = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tools", "refine_surfels.py"), ply, views,
                          "--steps", "30", "--out", out, "--quick"], capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    refined, _ = splatio.read_ply(out)
    assert refined.n_surfels == start.n_surfels and refined.sh_degree == start.sh_degree
    with open(str(tmp_path / "refined.json")) as f:
        report = json.load(f)
    print(f"splatrefine tool, --quick: {report['steps']} steps, loss {report['loss_before']:.4e} -> {report['loss_after']:.4e}, PSNR "
          f"{report['psnr_before']:.2f} -> {report['psnr_after']:.2f} dB")
    assert report["steps"] == 10 and len(report["loss_per_step"]) == 10 and "no spread" in report["wall_note"]
    assert report["loss_after"] < report["loss_before"]
    assert report["non_finite_gradient_words_skipped"] == 0
