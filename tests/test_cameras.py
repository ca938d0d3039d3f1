"""Row R11 of SURVEY.md section 8a: `lara_amd.cameras` against the REFERENCE's own `MiniCam` /
`getProjectionMatrix` (lightning/utils.py:5-48).

(1) fixture test: tests/golden/cameras_ref.npz is the output of the reference's classes
    (tests/golden/make_cameras_fixture.py); `make_cameras` must reproduce the four tensors the renderer hands to the
    rasteriser.  Tolerance: the reference inverts c2w with fp32 LAPACK, the mirror in fp64 then rounds ->
    |diff| <= 2e-6 (1 + |value|).
(2) contract test: tests/golden/shim_settings_ref.npz holds the settings record the reference's UNMODIFIED
    `lightning.renderer_2dgs.Renderer.set_rasterizer` built from a reference `MiniCam` with `diff_surfel_rasterization`
    resolving to this repository's shim (tests/golden/make_shim_settings_fixture.py); it is compared field by field --
    names, order, Python types, tensor shapes / dtypes, values -- with the one `lara_amd.renderer.Renderer` builds from
    a `lara_amd.cameras.Camera`.
"""
import math
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def fixture():
    return np.load(os.path.join(HERE, "golden", "cameras_ref.npz"))


def test_cameras_match_reference_minicam():
    from lara_amd import cameras
    f = fixture()
    c2w = torch.from_numpy(f["c2w"])
    for ci in (0, 1):
        W, H, fovx, fovy, zn, zf = f[f"case{ci}/params"]
        cams = cameras.make_cameras(c2w, int(W), int(H), float(fovx), float(fovy), float(zn), float(zf))
        assert len(cams) == c2w.shape[0]
        P = cameras.projection_matrix(float(zn), float(zf), float(fovx), float(fovy)).numpy()
        np.testing.assert_allclose(P, f[f"case{ci}/P"], rtol=1e-6, atol=1e-7)
        for i, cam in enumerate(cams):
            for name in ("world_view_transform", "projection_matrix", "full_proj_transform", "camera_center"):
                got, ref = getattr(cam, name).numpy(), f[f"case{ci}/{name}"][i]
                assert got.dtype == np.float32 and got.shape == ref.shape, name
                np.testing.assert_allclose(got, ref, rtol=2e-6, atol=2e-6, err_msg=f"case {ci} view {i} {name}")
            assert (cam.image_width, cam.image_height) == (int(W), int(H))
            assert math.isclose(cam.FoVx, fovx) and math.isclose(cam.FoVy, fovy)
        # the reference's (sic) camera centre is the NEGATED translation of c2w (utils.py:48)
        np.testing.assert_array_equal(cams[0].camera_center.numpy(), -f["c2w"][0, :3, 3])


def test_reference_renderer_builds_the_same_settings_through_the_shim():
    f = fixture()
    ref = np.load(os.path.join(HERE, "golden", "shim_settings_ref.npz"))
    import diff_surfel_rasterization as shim
    from lara_amd import cameras, rasterizer
    from lara_amd.renderer import Renderer as OurRenderer
    # what the reference module took from the shim (renderer_2dgs.py:7-10) is the operator itself
    assert [str(n) for n in ref["shim_names"]] == ["GaussianRasterizationSettings", "GaussianRasterizer"]
    for n in ref["shim_names"]:
        assert getattr(shim, str(n)) is getattr(rasterizer, str(n)), n
    c2w = torch.from_numpy(f["c2w"][int(ref["pose_index"])])
    W, H, fovx, fovy, zn, zf = ref["camera"]
    our_cam = cameras.make_cameras(c2w[None], int(W), int(H), float(fovx), float(fovy), float(zn), float(zf))[0]
    r = OurRenderer(sh_degree=1, white_background=True)
    r.set_bg_color(torch.from_numpy(ref["bg"]))                 # network.py:489-490
    rast = r.set_rasterizer(our_cam, device="cpu")              # renderer_2dgs.py:119-139
    assert isinstance(rast, rasterizer.GaussianRasterizer)
    b = rast.raster_settings
    assert type(b) is shim.GaussianRasterizationSettings
    assert b._fields == tuple(str(n) for n in ref["field_names"]) == (
        "image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix", "projmatrix",
        "sh_degree", "campos", "prefiltered", "debug")
    for name, tname in zip(b._fields, ref["field_types"]):
        x, y = ref[f"value/{name}"], getattr(b, name)
        if tname == "Tensor":
            assert isinstance(y, torch.Tensor) and tuple(y.shape) == x.shape and x.dtype == np.float32 and y.dtype == torch.float32, name
            np.testing.assert_allclose(y.numpy(), x, rtol=2e-6, atol=2e-6, err_msg=name)
        else:
            assert type(y).__name__ == str(tname), (name, type(y), tname)
            assert y == x.item() or math.isclose(y, x.item(), rel_tol=1e-6), name
    # the operator itself has no CPU path: the reference's render_img reaches it (renderer_2dgs.py:208-217) and it must fail loudly
    with pytest.raises(RuntimeError, match="no CPU path|HIP library not found"):
        p = 4
        centers = torch.zeros(p, 3)
        rast(means3D=centers, means2D=torch.zeros_like(centers, requires_grad=True), shs=torch.zeros(p, 4, 3),
             opacities=torch.sigmoid(torch.zeros(p, 1)), scales=torch.exp(torch.zeros(p, 2)),
             rotations=torch.nn.functional.normalize(torch.ones(p, 4)), cov3D_precomp=None)


def test_cameras_of_a_whole_batch_equal_the_per_scene_cameras():
    """`make_cameras_scenes` (one batched pass for the B x V cameras of a batch) against `make_cameras` per scene."""
    import torch
    from lara_amd import cameras
    c2w = torch.stack([cameras.turntable_c2w(8), cameras.turntable_c2w(8, 20.0)])
    scalars = [(1.1, 2.7, 0.75, 0.7), (0.9, 2.5, 0.6, 0.65)]
    sizes = [(512, 512), (256, 128)]
    got = cameras.make_cameras_scenes(c2w, sizes, scalars)
    for b in range(2):
        want = cameras.make_cameras(c2w[b], sizes[b][0], sizes[b][1], scalars[b][2], scalars[b][3], scalars[b][0], scalars[b][1])
        assert len(got[b]) == len(want) == 8
        for x, y in zip(got[b], want):
            for k in ("world_view_transform", "projection_matrix", "full_proj_transform", "camera_center"):
                assert torch.equal(getattr(x, k), getattr(y, k)), k
            assert (x.image_width, x.image_height, x.FoVx, x.FoVy, x.znear, x.zfar) == \
                   (y.image_width, y.image_height, y.FoVx, y.FoVy, y.znear, y.zfar)
