"""The image-feature volume (lara_amd.featvol; network.py:352-379 + :448-452) without a GPU: the plain-torch restatement in
tests/featvol_restate.py reproduces the reference's own run (tests/golden/featvol_ref.npz, tests/golden/make_featvol_fixture.py)
in fp32 and under bf16 autocast, forward and gradients -- that pins our reading of the reference, which the GPU tests then hold the
kernels to; FeatureVolume takes a reference-keyed state_dict; CPU tensors are refused."""
import numpy as np
import pytest
import torch

from tests.featvol_restate import load_fixture, restated


def _run(t, batch, bf16):
    x = t["img_feats"].clone().requires_grad_(True)
    p = {k: t[k].clone().requires_grad_(True) for k in ("ln_w", "ln_b", "mlp_w", "mlp_b", "view_embed")}
    V = batch["tar_rays_down"].shape[1]
    out = restated(batch, x, p["ln_w"], p["ln_b"], p["mlp_w"], p["mlp_b"], p["view_embed"], 3, batch["tar_rgb"].shape[2:4], V, bf16=bf16)
    (out * t["gout"].float()).sum().backward()
    return out.detach(), x.grad, {k: v.grad for k, v in p.items()}


@pytest.mark.parametrize("tag", ["fp32", "bf16"])
def test_restatement_reproduces_reference(tag):
    f, t, batch = load_fixture()
    assert f"mlp=torch.{'bfloat16' if tag == 'bf16' else 'float32'}" in list(f[f"{tag}_dtypes"])
    assert "norm=torch.float32" in list(f[f"{tag}_dtypes"]) and "feat_vol=torch.float32" in list(f[f"{tag}_dtypes"])
    out, dx, dp = _run(t, batch, tag == "bf16")
    tol = 1e-5 if tag == "fp32" else 1e-3
    ref = t[f"{tag}_feat_vol"]
    assert (out - ref).abs().max() <= tol * (1 + ref.abs().max())
    for name, got in (("d_img_feats", dx), ("d_ln_w", dp["ln_w"]), ("d_ln_b", dp["ln_b"]), ("d_mlp_w", dp["mlp_w"]),
                      ("d_mlp_b", dp["mlp_b"]), ("d_view_embed", dp["view_embed"])):
        r = t[f"{tag}_{name}"].float()
        err = (got - r).abs().max() / (r.abs().max() + 1e-12)
        assert err <= (1e-4 if tag == "fp32" else 2e-2), f"{tag} {name}: rel err {err:.2e}"


def test_fixture_covers_the_edges():
    f, t, batch = load_fixture()
    C = t["ln_w"].shape[0]
    s = t["fp32_feat_vol"][:, :, :C].abs().sum(2)
    assert (s == 0).any() and (s > 0).float().mean() > 0.5     # some points project outside the map, most inside
    h, w = batch["tar_rays_down"].shape[2:4]
    assert h != w


def test_state_dict_keys_are_the_references():
    from lara_amd.featvol import FeatureVolume
    fv = FeatureVolume(C=128, E=32, R=3)
    assert set(fv.state_dict()) == {"dir_norm.norm.weight", "dir_norm.norm.bias", "dir_norm.mlp.1.weight", "dir_norm.mlp.1.bias",
                                    "view_embed", "volume_grid"}
    _, t, _ = load_fixture()
    sd = {"dir_norm.norm.weight": t["ln_w"], "dir_norm.norm.bias": t["ln_b"], "dir_norm.mlp.1.weight": t["mlp_w"],
          "dir_norm.mlp.1.bias": t["mlp_b"], "view_embed": t["view_embed"], "volume_grid": fv.volume_grid.clone()}
    fv.load_state_dict(sd, strict=True)
    assert torch.equal(fv.dir_norm.mlp[1].weight.detach(), t["mlp_w"])
    # adopting the reference's own objects
    other = FeatureVolume(C=128, E=32, R=3, dir_norm=fv.dir_norm, view_embed=fv.view_embed)
    assert other.dir_norm is fv.dir_norm and other.view_embed is fv.view_embed
    assert FeatureVolume(C=128, E=0, R=3).view_embed is None


def test_cpu_tensors_have_no_path():
    from lara_amd.featvol import FeatureVolume
    _, t, batch = load_fixture()
    fv = FeatureVolume(C=128, E=32, R=3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fv(batch, t["img_feats"], 3)


def test_bad_shapes_are_refused():
    from lara_amd.featvol import FeatureVolume
    with pytest.raises(ValueError):
        FeatureVolume(C=128, E=32, R=3, dir_norm=FeatureVolume(C=64, E=32, R=3).dir_norm)


def test_invalid_arguments_return_error_codes(hip_lib):
    import ctypes
    from lara_amd._native import load_library
    from lara_amd.featvol import _Dims
    lib = load_library()
    d = _Dims()
    d.B, d.V, d.C, d.E, d.h, d.w, d.R, d.img_w, d.img_h, d.eps = 1, 4, 768, 32, 32, 32, 16, 512, 512, 1e-6
    assert lib.lara_featvol_workspace_bytes(ctypes.byref(d)) > 0
    dummy = ctypes.c_void_p(4096)        # (never dereferenced: the argument check comes first)
    assert lib.lara_featvol_forward(ctypes.byref(d), *([dummy] * 10), 2, dummy, dummy, None) == -1         # bad layout
    assert lib.lara_featvol_backward(ctypes.byref(d), *([dummy] * 10), 0, *([dummy] * 5), None, None, None) == -1   # no workspace
    for field, bad in (("C", 96), ("C", 2048), ("V", 9), ("E", 30), ("h", 300)):
        setattr(d, field, bad)
        assert lib.lara_featvol_workspace_bytes(ctypes.byref(d)) == -1, field
        assert lib.lara_featvol_forward(ctypes.byref(d), *([dummy] * 10), 0, dummy, dummy, None) == -1, field
        d.B, d.V, d.C, d.E, d.h = 1, 4, 768, 32, 32
