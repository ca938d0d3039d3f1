"""`lara_amd.splatxform` on the device: the kernel's words equal the host entry's on every case of the CPU tests (twice, on a side
stream, in place, at row offsets into sentinel-filled outputs); a cloud moved together with its cameras renders, through
``Renderer.render_views``, as the original within what one fp32 ulp on every input does to the same render (the control), while
unrotated SH coefficients or a rebuilt ``camera_center`` are tens of dB off; ``place``; ``align_to``; tools/render_surfels.py
``--transform``."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import splatxform_cases as C
from tests import splatxform_restate as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
SIZE = 64
MAPS = ("image", "depth", "acc_map", "rend_normal", "depth_normal", "rend_dist")

_shared = {}


def _cloud(c, device=DEV):
    from lara_amd import splatio
    return splatio.SurfelCloud(*(torch.from_numpy(c[k].copy()).to(device) for k in C.FIELDS))


def _words(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------ kernel bits

@pytest.mark.parametrize("degree", C.DEGREES)
def test_the_kernel_equals_the_host_entry_bit_for_bit(hip_lib, degree):
    from lara_amd import splatxform as X
    plan = X.similarity(C.SIMILARITY)
    n = (degree + 1) ** 2
    side = torch.cuda.Stream(DEV)
    for P in C.SIZES:
        c = C.cloud(P, degree, seed=P + degree)
        host = X.transform(_cloud(c, "cpu"), C.SIMILARITY)
        want = [_words(t) for t in host.render_args()]
        with torch.cuda.stream(side):
            for attempt in range(2):
                got = X.transform(_cloud(c), C.SIMILARITY)
                assert got.device.type == "cuda" and got.n_surfels == P and got.sh_degree == degree
                inplace = _cloud(c)
                assert X.transform(inplace, C.SIMILARITY, out=inplace) is inplace
                for k, a, b, w in zip(C.FIELDS, got.render_args(), inplace.render_args(), want):
                    assert a.shape == b.shape == w.shape
                    assert np.array_equal(_words(a), w), (P, k, attempt)
                    assert np.array_equal(_words(b), w), (P, k, attempt, "in place")
                for row0 in C.ROW_OFFSETS:
                    rows = row0 + P + 7
                    outs = [torch.from_numpy(np.full((rows,) + shape, C.SENTINEL, np.uint32).view(np.float32)).to(DEV)
                            for shape in ((3,), (n, 3), (1,), (2,), (4,))]
                    X._apply(plan, _cloud(c), outs, row0, rows)
                    for k, t, w in zip(C.FIELDS, outs, want):
                        g = _words(t)
                        assert np.array_equal(g[row0:row0 + P], w), (P, row0, k, attempt)
                        assert (g[:row0] == C.SENTINEL).all() and (g[row0 + P:] == C.SENTINEL).all(), (P, row0, k, attempt)
        side.synchronize()
    empty = X.transform(_cloud(C.cloud(0, degree)), C.RIGID)
    assert empty.n_surfels == 0 and empty.shs.shape == (0, n, 3) and empty.device.type == "cuda"


# ------------------------------------------------------------------------------------------------------------------ renders

def _scene():
    """The 1 024 surfels (16 SH coefficients) on the device, two 64 x 64 turntable cameras, one renderer of degree 3: made once."""
    if not _shared:
        from lara_amd import cameras, splatio, synthetic
        from lara_amd.renderer import Renderer
        sc = synthetic.make_scene(grid=8, K=2, regime="trained", sh_coeffs=16, device=DEV)
        c2w = cameras.turntable_c2w(2)
        cams = cameras.make_cameras(c2w, SIZE, SIZE, 0.75, 0.75, 0.5, 2.5, device=DEV)
        for i, cam in enumerate(cams):
            cam.view_world_transform = c2w[i].to(DEV)
        cloud = splatio.SurfelCloud(*(sc[k].contiguous() for k in C.FIELDS))
        assert cloud.n_surfels == 1024 and cloud.sh_degree == 3
        _shared.update(cloud=cloud, c2w=c2w, cams=cams, renderer=Renderer(sh_degree=3, white_background=True))
        _shared["original"] = _render(cloud, cams, c2w)
        _shared["control"] = _render(_one_ulp(cloud), cams, c2w)
    return _shared


def _render(cloud, cams, c2w):
    from lara_amd.batch import build_rays, fov_to_ixt
    ixt = fov_to_ixt(torch.tensor([[0.75, 0.75]] * len(cams)), (SIZE, SIZE)).to(DEV)
    rays = build_rays(torch.as_tensor(c2w).float().to(DEV), ixt, SIZE, SIZE)
    with torch.no_grad():
        out = _shared["renderer"].render_views(cams, rays, *cloud.render_args(), DEV, concat=True)
    return {k: out[k].double().cpu().numpy() for k in MAPS}


def _one_ulp(cloud):
    """Every input moved by one fp32 ulp in a seeded direction."""
    from lara_amd import splatio
    g = np.random.default_rng(2024)
    moved = []
    for t in cloud.render_args():
        a = t.cpu().numpy()
        moved.append(torch.from_numpy(np.nextafter(a, np.where(g.random(a.shape) < 0.5, -np.inf, np.inf).astype(np.float32))).to(DEV))
    return splatio.SurfelCloud(*moved)


def _psnr(got, want):
    mse = float(np.mean((got - want) ** 2))
    peak = float(np.abs(want).max())
    return float("inf") if mse == 0.0 else 10.0 * np.log10(peak * peak / mse)


def _figures(got, want, keys):
    """{map: (PSNR, max |diff|, share of values off by more than 1e-3)}."""
    out = {}
    for k in keys:
        d = np.abs(got[k] - want[k])
        out[k] = (_psnr(got[k], want[k]), float(d.max()), float((d > 1e-3).mean()))
    return out


def _expected(original, T):
    """What the moved render must show: the normals turned by R, the depth times s."""
    R, s, _, _ = S.split(T)
    want = dict(original)
    want["rend_normal"], want["depth_normal"] = original["rend_normal"] @ R.T, original["depth_normal"] @ R.T
    want["depth"] = original["depth"] * s
    return want, s


def _moved(name, **kw):
    from lara_amd import splatxform as X
    s = _scene()
    T = C.TRANSFORMS[name]
    cloud = kw.get("cloud") or X.transform(s["cloud"], T)
    cams = kw.get("cams") or X.transform_cameras(s["cams"], T)
    return _render(cloud, cams, X.transform_c2w(s["c2w"], T))


@pytest.mark.parametrize("name", ["rotation", "rigid", "similarity"])
def test_a_moved_cloud_renders_as_the_original(hip_lib, name):
    s = _scene()
    original = s["original"]
    assert (original["image"] != 1.0).any() and original["acc_map"].max() > 0.5          # a picture, not the background
    control = _figures(s["control"], original, MAPS)
    want, scale = _expected(original, C.TRANSFORMS[name])
    got = _moved(name)
    got["depth"] = got["depth"] / scale
    want["depth"] = original["depth"]
    keys = MAPS if name != "similarity" else MAPS[:-1]          # rend_dist rests on absolute near / far constants: s = 1 only
    figs = _figures(got, want, keys)
    for k in keys:
        print(f"splatxform parity, {name}, {k}: PSNR {figs[k][0]:.1f} dB (control {control[k][0]:.1f}), max |diff| {figs[k][1]:.3g} "
              f"(control {control[k][1]:.3g}), off by > 1e-3: {100 * figs[k][2]:.3f} %")
    for k in keys:
        assert figs[k][0] >= control[k][0] - 10.0, (k, figs[k], control[k])
        assert figs[k][1] <= 16.0 * control[k][1], (k, figs[k], control[k])
        assert figs[k][2] <= 0.005, (k, figs[k])


def test_unrotated_coefficients_and_a_rebuilt_centre_are_tens_of_db_off(hip_lib):
    from lara_amd import cameras, splatio, splatxform as X
    s = _scene()
    original = s["original"]["image"]
    for name in ("rotation", "rigid", "similarity"):
        T = C.TRANSFORMS[name]
        good = _psnr(_moved(name)["image"], original)
        moved = X.transform(s["cloud"], T)
        flat = splatio.SurfelCloud(moved.centers, s["cloud"].shs, moved.opacity, moved.scales, moved.rotations)
        tooth = _psnr(_moved(name, cloud=flat)["image"], original)
        print(f"splatxform tooth, {name}: {good:.1f} dB with the blocks, {tooth:.1f} dB with the coefficients left as they were")
        assert good - tooth > 40.0, (name, good, tooth)
    # the sic: camera_center rebuilt as -c2w'[:3, 3] instead of moved as a point
    T = C.TRANSFORMS["rigid"]
    cams = X.transform_cameras(s["cams"], T)
    poses = X.transform_c2w(s["c2w"], T)
    for cam, pose in zip(cams, poses):
        cam.camera_center = torch.nn.functional.pad(-pose[:3, 3].float(), (0, 1)).to(DEV)[:3]
    good, sic = _psnr(_moved("rigid")["image"], original), _psnr(_moved("rigid", cams=cams)["image"], original)
    print(f"splatxform sic, rigid: {good:.1f} dB with the centre moved as a point, {sic:.1f} dB with it rebuilt from the moved pose")
    assert good - sic > 40.0, (good, sic)
    assert cameras.make_cameras(s["c2w"], SIZE, SIZE, 0.75, 0.75, 0.5, 2.5)[0].camera_center.tolist() == (-s["c2w"][0, :3, 3]).tolist()


def test_place_renders_as_the_concatenated_transforms(hip_lib):
    from lara_amd import splatio, splatxform as X
    s = _scene()
    shift = np.eye(4)
    shift[0, 3] = 0.8
    placed = X.place([s["cloud"], s["cloud"]], [np.eye(4), shift])
    joined = splatio.concatenate([X.transform(s["cloud"], np.eye(4)), X.transform(s["cloud"], shift)])
    assert placed.n_surfels == 2048
    for a, b in zip(placed.render_args(), joined.render_args()):
        assert np.array_equal(_words(a), _words(b))
    got, want = _render(placed, s["cams"], s["c2w"]), _render(joined, s["cams"], s["c2w"])
    for k in MAPS:
        assert got[k].tobytes() == want[k].tobytes(), k
    assert np.abs(got["image"] - s["original"]["image"]).max() > 0.05          # the copy is in the picture


def test_align_to_follows_the_registration(hip_lib):
    from lara_amd import meshalign, splatio, splatxform as X
    from tests import meshalign_cases as M
    src, V, F, _ = M.registration_case(2, 10)
    src = np.ascontiguousarray(src, np.float32)
    c = C.cloud(len(src), 1, seed=3, special=False)
    c["centers"] = src
    cloud = _cloud(c)
    target = (torch.from_numpy(np.ascontiguousarray(V, np.float32)).to(DEV), torch.from_numpy(np.ascontiguousarray(F)).to(DEV))
    kept, idx = splatio.select(cloud, min_opacity=0.005)
    assert 0 < idx.numel() <= cloud.n_surfels
    want = meshalign.icp(kept.centers, target, max_dist=M.MAX_DIST)
    moved, result = X.align_to(cloud, target, max_dist=M.MAX_DIST)
    assert result["transformation"].tobytes() == want["transformation"].tobytes() and result["iterations"] == want["iterations"]
    again = X.transform(cloud, want["transformation"])
    for a, b in zip(moved.render_args(), again.render_args()):
        assert np.array_equal(_words(a), _words(b))
    assert np.abs(result["transformation"] - M.truth(10)).max() < 1e-2          # and it is the motion that was put in


def test_render_surfels_tool_moves_the_cloud(hip_lib, tmp_path):
    from lara_amd import splatio
    s = _scene()
    ply, ident = str(tmp_path / "scene.ply"), str(tmp_path / "identity.txt")
    splatio.write_ply(ply, s["cloud"])
    np.savetxt(ident, np.eye(4))
    outs = []
    for extra in ([], ["--transform", ident]):
        out = tmp_path / ("moved" if extra else "plain")
        # a fresh child process under its own time limit; nothing below runs when it fails
        run = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tools", "render_surfels.py"), ply,
                              "--dataset", "gobjeverse", "--out", str(out), "--quick"] + extra, capture_output=True, text=True, cwd=ROOT)
        assert run.returncode == 0, run.stderr[-2000:]
        outs.append(out)
    names = sorted(n for n in os.listdir(outs[0]) if n.endswith(".png"))
    assert names == ["normal_0000.png", "normal_0001.png", "rgb_0000.png", "rgb_0001.png"]
    for n in names:
        assert (outs[0] / n).read_bytes() == (outs[1] / n).read_bytes(), n
