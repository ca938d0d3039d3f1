"""The image-feature volume on the MI355X (lara_amd.featvol, include/lara_featvol.h) against the reference's own run
(tests/golden/featvol_ref.npz) and against itself.

Tolerances.  The kernels mirror bf16 autocast (the reference trains bf16-mixed): against the autocast fixture the forward agrees to
|diff| <= 2e-2 * max|ref| (the Linear's fp32 sums are ordered differently, which can move a bf16 rounding of shift / scale, and
the bf16 sample positions with it: the `test_pointfeat.py` position budget, at bf16 resolution) and the gradients to 5e-2 of the
largest entry; against the fp32 fixture every error is at most twice autocast's own error (fixture bf16 vs fixture fp32) plus
1e-3 of the largest entry, as in `test_groupatt.py`.  Everything the kernels compute twice -- layouts, strides, runs -- is bitwise.

These are the COARSE bars: they are sized for bf16 noise at the reference's own shapes, and a dropped (point, tap) entry, a texel
list cut short or a border tap with the wrong weight would pass them.  The tight ones -- every fp32 element within its own
accumulation bound of a bf16-faithful fp64 reference, at the shapes where the kernels take another path -- are in
tests/test_featvol_faithful_gpu.py."""
import pytest
import torch

from tests.featvol_restate import load_fixture, restated

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRADS = ("d_img_feats", "d_ln_w", "d_ln_b", "d_mlp_w", "d_mlp_b", "d_view_embed")


def _module(t, C, E, R):
    from lara_amd.featvol import FeatureVolume
    fv = FeatureVolume(C=C, E=E, R=R).to(DEV)
    with torch.no_grad():
        fv.dir_norm.norm.weight.copy_(t["ln_w"]); fv.dir_norm.norm.bias.copy_(t["ln_b"])
        fv.dir_norm.mlp[1].weight.copy_(t["mlp_w"]); fv.dir_norm.mlp[1].bias.copy_(t["mlp_b"])
        if E:
            fv.view_embed.copy_(t["view_embed"])
    return fv


def _grads(fv, batch, x, gout, V):
    fv.zero_grad()
    x = x.detach().clone().requires_grad_(True)
    out = fv(batch, x, V)
    (out * gout).sum().backward()
    ps = (fv.dir_norm.norm.weight, fv.dir_norm.norm.bias, fv.dir_norm.mlp[1].weight, fv.dir_norm.mlp[1].bias, fv.view_embed)
    return out.detach(), dict(zip(GRADS, [x.grad] + [p.grad.clone() for p in ps]))


def _fixture():
    f, t, batch = load_fixture(DEV)
    return f, t, batch, _module(t, t["ln_w"].shape[0], t["view_embed"].shape[2], 3)


def test_forward_and_gradients_against_the_reference():
    f, t, batch, fv = _fixture()
    V = batch["tar_rays_down"].shape[1]
    out, gr = _grads(fv, batch, t["img_feats"], t["gout"].float(), V)
    rb, rf = t["bf16_feat_vol"], t["fp32_feat_vol"]
    assert (out - rb).abs().max() <= 2e-2 * rb.abs().max()
    assert (out - rf).abs().max() <= 2 * (rb - rf).abs().max() + 1e-3 * rf.abs().max()
    for k in GRADS:
        gb, gf = t[f"bf16_{k}"].float(), t[f"fp32_{k}"].float()
        err_b = (gr[k] - gb).abs().max() / gb.abs().max()
        assert err_b <= 5e-2, f"{k}: {err_b:.2e} against the autocast run"
        assert (gr[k] - gf).abs().max() <= 2 * (gb - gf).abs().max() + 1e-3 * gf.abs().max(), k


@pytest.mark.parametrize("V", [1, 3, 4])
def test_views_layouts_strides_and_runs_are_bitwise(V):
    from lara_amd.featvol import TOKENS, VOLUME
    from lara_amd._native import current_stream as _stream, load_library as enc_lib
    f, t, batch, fv = _fixture()
    B, Vf, h, w = batch["tar_rays_down"].shape[:4]
    C = t["ln_w"].shape[0]
    g = torch.Generator().manual_seed(V)
    rays = torch.randn(B, 4, h, w, 6, generator=g).to(DEV)
    rays[..., :3] = batch["tar_rays_down"][:, :1, ..., :3].expand(B, 4, h, w, 3)
    bt = {"tar_rays_down": rays, "tar_w2c": batch["tar_w2c"][:, [0, 1, 2, 0]], "tar_ixt": batch["tar_ixt"][:, [0, 1, 2, 0]],
          "tar_rgb": torch.zeros(B, 4, *batch["tar_rgb"].shape[2:], device=DEV)}
    tok = torch.randn(B * V, h * w, C, generator=g).to(DEV)
    x_cl = torch.einsum("blc->bcl", tok).reshape(B * V, C, h, w)       # channels-last view
    x_ct = x_cl.contiguous()
    assert x_cl.stride(1) == 1 and x_ct.stride(3) == 1
    gout = torch.randn(B, V, C + fv.E, 3, 3, 3, generator=g).to(DEV)
    o1, g1 = _grads(fv, bt, x_cl, gout, V)
    o2, g2 = _grads(fv, bt, x_cl, gout, V)
    o3, g3 = _grads(fv, bt, x_ct, gout, V)
    assert torch.equal(o1, o2) and torch.equal(o1, o3)
    for k in GRADS:
        assert torch.equal(g1[k], g2[k]), f"{k}: two runs differ"
        assert torch.equal(g1[k], g3[k]), f"{k}: channels-last and contiguous differ"
    assert g3["d_img_feats"].is_contiguous() and g1["d_img_feats"].stride() == x_cl.stride()
    # the encoder's operand: layout TOKENS == lara_batched_transpose(layout VOLUME), and the gradients through either layout
    prep = fv.prepare(bt, x_cl, V)
    prep.params(*fv._args(V))
    vol = prep.forward(VOLUME)
    toks = prep.forward(TOKENS)
    S, CE = 27, C + fv.E
    want = torch.empty(B * S, V, CE, dtype=torch.bfloat16, device=DEV)
    enc_lib().lara_batched_transpose(B, V * CE, S, vol.data_ptr(), want.data_ptr(), 1, _stream(torch.device(DEV)))
    assert torch.equal(toks, want) and torch.equal(vol, o1)
    g_tok = gout.reshape(B, V * CE, S).transpose(1, 2).contiguous().view(B * S, V, CE)
    ga, gb = prep.backward(gout, VOLUME), prep.backward(g_tok, TOKENS)
    for a, b in zip(ga, gb):
        assert torch.equal(a, b)


def test_full_size_against_the_restatement():
    """C = 768, R = 16, 4 views of a 32 x 32 map of 512^2 images (configs/base.yaml)."""
    from lara_amd.batch import synthetic_batch
    from lara_amd.featvol import FeatureVolume
    torch.manual_seed(0)
    B, V, C, R = 2, 4, 768, 16
    batch = synthetic_batch(batch_size=B, n_views=V, H=512, W=512, n_input=4, seed=3, device=DEV)
    fv = FeatureVolume(C=C, E=32, R=R).to(DEV)
    with torch.no_grad():
        fv.dir_norm.norm.weight.add_(0.2 * torch.randn(C, device=DEV))
        fv.dir_norm.mlp[1].bias.add_(0.1 * torch.randn(2 * C, device=DEV))
    tok = torch.randn(B * V, 32 * 32, C, device=DEV)
    x = torch.einsum("blc->bcl", tok).reshape(B * V, C, 32, 32)
    gout = torch.randn(B, V, C + 32, R, R, R, device=DEV)
    out, gr = _grads(fv, batch, x, gout, V)
    n, lin = fv.dir_norm.norm, fv.dir_norm.mlp[1]
    ps = [p.detach().clone().requires_grad_(True) for p in (n.weight, n.bias, lin.weight, lin.bias, fv.view_embed)]
    xr = x.detach().clone().requires_grad_(True)
    ref = restated(batch, xr, *ps, R, (512, 512), V, bf16=True)
    (ref * gout).sum().backward()
    assert (out - ref).abs().max() <= 2e-2 * ref.abs().max()
    assert (out - ref).abs().mean() <= 1e-3 * ref.abs().max()
    for k, p in zip(GRADS, [xr] + ps):
        err = (gr[k] - p.grad).abs().max() / p.grad.abs().max()
        assert err <= 5e-2, f"{k}: rel err {err:.2e}"


@pytest.mark.parametrize("training", [True, False])
def test_pipeline_from_image_features_equals_the_operator_then_the_pipeline(training):
    from lara_amd.featvol import FeatureVolume
    from tests.test_pipeline import _small_problem
    pipe, batch, _ = _small_problem(DEV)
    pipe.fine_mask = "plain"
    B = batch["tar_rgb"].shape[0]
    h, w = batch["tar_rays_down"].shape[2:4]
    fv = FeatureVolume(C=768, E=32, R=2).to(DEV)
    pipe.feat_volume = fv
    g = torch.Generator().manual_seed(5)
    x0 = torch.einsum("blc->bcl", torch.randn(B * 4, h * w, 768, generator=g).to(DEV)).reshape(B * 4, 768, h, w)
    params = list(pipe.parameters())

    def run(fused):
        x = x0.detach().clone().requires_grad_(True)
        for p in params:
            p.grad = None
        with torch.set_grad_enabled(training):
            out = pipe.forward_from_image_features(batch, x) if fused else pipe(batch, fv(batch, x, 4))
            if not training:
                return out, None, None
            from lara_amd.pipeline import lara_loss
            loss, _ = lara_loss(batch, out, ms_ssim=False)
            loss.backward()
        pipe.join_streams()
        return out, x.grad, [None if p.grad is None else p.grad.clone() for p in params]

    o1, dx1, gp1 = run(True)
    o2, dx2, gp2 = run(False)
    for k in o1:
        assert torch.equal(o1[k], o2[k]), k
    if training:
        assert torch.equal(dx1, dx2)
        names = [n for n, _ in pipe.named_parameters()]
        assert any(n.startswith("feat_volume.") for n in names)
        for n, a, b in zip(names, gp1, gp2):
            assert (a is None) == (b is None) and (a is None or torch.equal(a, b)), n
