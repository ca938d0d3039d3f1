"""`lara_amd.splatio` where the surfels are made: a file written from device tensors and read back to the device renders, through
``Renderer.render_views``, to the same bits on every output map as the original tensors (coarse-style and fine-style tuples);
``select`` and ``ply_bytes`` on the device equal the same calls on the CPU copies; tools/render_surfels.py at its --quick size."""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import splatio_restate as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
SIZE = 64

_shared = {}


def _scene():
    """The 1 024 surfels (SH degree 1) on the device, two 64 x 64 cameras with their rays, one renderer: made once."""
    if not _shared:
        from lara_amd import cameras, synthetic
        from lara_amd.batch import build_rays, fov_to_ixt
        from lara_amd.renderer import Renderer
        sc = synthetic.make_scene(grid=8, K=2, regime="trained", sh_coeffs=4, device=DEV)
        c2w = cameras.turntable_c2w(2)
        cams = cameras.make_cameras(c2w, SIZE, SIZE, 0.75, 0.75, 0.5, 2.5, device=DEV)
        ixt = fov_to_ixt(torch.tensor([[0.75, 0.75]] * 2), (SIZE, SIZE)).to(DEV)
        _shared.update(args=tuple(sc[k] for k in ("centers", "shs", "opacity", "scales", "rotations")), cams=cams,
                       rays=build_rays(c2w.to(DEV), ixt, SIZE, SIZE), renderer=Renderer(sh_degree=1, white_background=True))
    return _shared


def _render(args, cams=None, rays=None):
    s = _scene()
    with torch.no_grad():
        out = s["renderer"].render_views(cams or s["cams"], s["rays"] if rays is None else rays, *args, DEV, concat=True)
    return {k: v.clone() for k, v in out.items()}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_same_maps(got, want):
    assert set(got) == set(want) == {"image", "depth", "acc_map", "rend_normal", "depth_normal", "rend_dist"}
    for k in want:
        assert got[k].shape == want[k].shape and torch.equal(_bits(got[k]), _bits(want[k])), k


@pytest.mark.parametrize("style", ["coarse", "fine"])
def test_a_loaded_file_renders_to_the_same_bits(hip_lib, tmp_path, style):
    from lara_amd import splatio
    centers, shs, opacity, scales, rotations = _scene()["args"]
    assert centers.shape == (1024, 3) and shs.shape == (1024, 4, 3)
    if style == "fine":          # network.py:515: centres and shs are the subset already, the rest is indexed by the mask
        mask = torch.rand(1024, generator=torch.Generator().manual_seed(1)).to(DEV) < 0.7
        assert 0 < int(mask.sum()) < 1024
        item = (centers[mask], shs[mask], opacity, scales, rotations, mask)
        args = (centers[mask], shs[mask], opacity[mask], scales[mask], rotations[mask])
    else:
        item = args = (centers, shs, opacity, scales, rotations)
    want = _render(args)
    assert bool((want["image"] != 1.0).any()) and float(want["acc_map"].max()) > 0.5          # a picture, not the background
    cloud = splatio.SurfelCloud.from_render_pkg(item)
    assert cloud.device == centers.device and cloud.sh_degree == 1
    path = str(tmp_path / "point_cloud.ply")
    splatio.write_ply(path, cloud)
    back, info = splatio.read_ply(path, device=DEV)
    assert back.device == centers.device and back.n_surfels == args[0].shape[0] == info["n_surfels"]
    for a, b in zip(back.render_args(), args):
        assert torch.equal(_bits(a), _bits(b))
    _assert_same_maps(_render(back.render_args()), want)


def test_select_and_ply_bytes_on_the_device_equal_the_cpu_copies(hip_lib):
    from lara_amd import splatio
    cloud = splatio.SurfelCloud(*_scene()["args"])
    host = cloud.to("cpu")
    assert cloud.device.type == "cuda" and host.device.type == "cpu"
    kept, idx = splatio.select(cloud, min_opacity=0.005)
    kept_h, idx_h = splatio.select(host, min_opacity=0.005)
    assert idx.is_cuda and idx.dtype == torch.int64 and torch.equal(idx.cpu(), idx_h) and 0 < idx.numel() < 1024
    for a, b in zip(kept.render_args(), kept_h.render_args()):
        assert a.is_cuda and torch.equal(_bits(a).cpu(), _bits(b))
    box = ([-0.4, -0.5, -0.1], [0.5, 0.2, 0.5])
    assert torch.equal(splatio.select(cloud, 0.005, box)[1].cpu(), splatio.select(host, 0.005, box)[1])
    for thickness in (None, 0.002):
        data = splatio.ply_bytes(cloud, thickness)
        assert data == splatio.ply_bytes(host, thickness)
        assert data == R.file_bytes({k: t.numpy() for k, t in zip(("centers", "shs", "opacity", "scales", "rotations"),
                                                                  host.render_args())}, thickness)
    assert splatio.ply_bytes(kept) == splatio.ply_bytes(kept_h)


def test_render_surfels_tool_runs_at_its_quick_size(hip_lib, tmp_path):
    from lara_amd import evaluate, meshtexture, splatio
    from lara_amd.batch import build_rays, fov_to_ixt
    args = _scene()["args"]
    ply, out = str(tmp_path / "scene.ply"), tmp_path / "frames"
    splatio.write_ply(ply, splatio.SurfelCloud(*args))
    # a fresh child process under its own time limit; nothing below runs when it fails
    run = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tools", "render_surfels.py"), ply,
                          "--dataset", "gobjeverse", "--out", str(out), "--quick"], capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    res = json.loads((out / "render_surfels.json").read_text())
    assert json.loads(run.stdout.strip().splitlines()[-1]) == res
    assert (res["n_surfels"], res["sh_degree"], res["frames"], res["size"]) == (1024, 1, 2, 32)
    assert res["mesh"] is None and res["dropped_third_scale"] is None and all(v >= 0 for v in res["wall_s"].values())
    assert sorted(os.listdir(out)) == ["normal_0000.png", "normal_0001.png", "render_surfels.json", "rgb_0000.png", "rgb_0001.png"]
    # the first RGB frame against the render of the ORIGINAL tensors from the same camera, rounded as evaluation.py:131 rounds
    cams = evaluate.video_cameras(2, "gobjeverse", (32, 32), device=DEV)
    c2w = torch.stack([c.view_world_transform for c in cams]).to(DEV)
    ixt = torch.stack([fov_to_ixt(torch.tensor((c.FoVx, c.FoVy)), (32, 32)) for c in cams]).to(DEV)
    img = _render(args, cams, build_rays(c2w, ixt, 32, 32))["image"]          # [32, 2 * 32, 3]
    want = torch.round(img[:, :32] * 255).clamp(0, 255).to(torch.uint8).cpu()
    got = torch.from_numpy(meshtexture.read_png(str(out / "rgb_0000.png")))
    assert got.shape == (32, 32, 4) and bool((got[..., 3] == 255).all())
    assert torch.equal(got[..., :3], want) and bool((want != 255).any())
