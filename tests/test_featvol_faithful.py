"""The bf16-faithful fp64 reference of the image-feature volume (oracle/featvol_bf16.py) and the cases built on it
(tests/featvol_cases.py), without a GPU.  What tests/test_featvol_faithful_gpu.py then holds the kernels to rests on these:

  - with its roundings off the reference IS the fp32 restatement (tests/featvol_restate.py, which tests/test_featvol.py pins to
    the reference project's own run), values and autograd gradients;
  - with its roundings on its sample positions are, bit for bit, what torch's own bf16 operators feed grid_sample;
  - no case has a point whose position rounding could go the other way on the device (the position condition);
  - every case reaches what its row of the table claims, read off the reference's tap lists;
  - the yardstick N of the noise bar measures something: 0 < N < 5e-2 for every tensor it is used on.
"""
import pytest
import torch

from lara_amd.featvol import build_dense_grid
from oracle import featvol_bf16 as fb
from tests import featvol_cases as fc
from tests import featvol_restate
from tests.featvol_restate import load_fixture, restated

GRAD_KEYS = {"dx": "x", "d_ln_w": "ln_w", "d_ln_b": "ln_b", "d_mlp_w": "mlp_w", "d_mlp_b": "mlp_b", "d_view_embed": "embed"}


def _fixture_inputs():
    f, t, batch = load_fixture()
    H, W = batch["tar_rgb"].shape[2:4]
    B, V = batch["tar_rays_down"].shape[:2]
    ref = {"x": t["img_feats"].double(), "rays": batch["tar_rays_down"].double(), "w2c": batch["tar_w2c"].double(),
           "ixt": batch["tar_ixt"].double(), "embed": t["view_embed"][0, :V, :, 0, 0, 0].double(), "R": 3, "img_w": W, "img_h": H,
           "eps": 1e-6}
    ref.update({k: t[k].double() for k in ("ln_w", "ln_b", "mlp_w", "mlp_b")})
    return t, batch, ref, t["gout"].float().reshape(B, V, -1, 27), (H, W)


def _case_inputs(case):
    (B, V, C, E, h, w, R), (img_w, img_h), _ = fc.CASES[case]
    t, ref = fc.inputs(case, "B")
    batch = {"tar_rays_down": t["rays"], "tar_w2c": t["w2c"], "tar_ixt": t["ixt"]}
    return t, batch, ref, t["grad"], (img_h, img_w)


def _restated_grads(t, batch, ref, grad, img_hw, bf16):
    leaves = {k: ref[k].float().clone().requires_grad_(True) for k in ("x", "ln_w", "ln_b", "mlp_w", "mlp_b", "embed")}
    V, E = ref["embed"].shape
    out = restated(batch, leaves["x"], leaves["ln_w"], leaves["ln_b"], leaves["mlp_w"], leaves["mlp_b"],
                   leaves["embed"].view(1, V, E, 1, 1, 1), ref["R"], img_hw, V, bf16=bf16)
    (out.reshape(grad.shape) * grad).sum().backward()
    return out.detach().reshape(grad.shape), {k: leaves[v].grad for k, v in GRAD_KEYS.items()}


@pytest.mark.parametrize("which", ["fixture", "b"])
def test_unrounded_reference_is_the_fp32_restatement(which):
    """roundings off: values and autograd gradients equal restated(bf16=False) to the fp32 restatement's own precision"""
    t, batch, ref, grad, img_hw = _fixture_inputs() if which == "fixture" else _case_inputs(which)
    out32, g32 = _restated_grads(t, batch, ref, grad, img_hw, False)
    r = fb.backward(ref, grad.double(), False, False)
    assert (r["fwd"]["out"] - out32).abs().max() <= 1e-5 * out32.abs().max()
    for k in GRAD_KEYS:
        err = float((r[k] - g32[k]).abs().max() / g32[k].abs().max())
        assert err <= 1e-5, f"{k}: {err:.2e}"
    # the TOKENS layout is the transpose lara_batched_transpose makes of it
    B, V, CE, S = grad.shape
    assert torch.equal(r["fwd"]["tokens"], r["fwd"]["out"].permute(0, 3, 1, 2).reshape(B * S, V, CE))


def test_rounded_positions_are_torchs_own_bf16_positions(monkeypatch):
    """roundings on, on the fixture: the sample positions equal what restated(bf16=True) -- torch's bf16 matmul, division and
    normalisation -- feeds grid_sample, bit for bit; and the output is within the restatement's bar of the reference's run"""
    t, batch, ref, grad, (H, W) = _fixture_inputs()
    seen = {}
    real = torch.nn.functional.grid_sample

    def spy(inp, grid, **kw):
        seen["grid"] = grid.detach().clone()
        return real(inp, grid, **kw)
    monkeypatch.setattr(featvol_restate.F, "grid_sample", spy)
    V = batch["tar_rays_down"].shape[1]
    restated(batch, t["img_feats"], t["ln_w"], t["ln_b"], t["mlp_w"], t["mlp_b"], t["view_embed"], 3, (H, W), V, bf16=True)
    monkeypatch.undo()
    g = seen["grid"][:, 0].double()                                   # [B V, S, 2], bf16 values
    h, w = t["img_feats"].shape[2:]
    s = fb.forward(ref, True, True)
    ix, iy, info = fb.positions(fb.dense_grid(3), ref["w2c"].reshape(-1, 4, 4), ref["ixt"].reshape(-1, 3, 3), W, H, h, w)
    assert torch.equal(ix, ((g[..., 0] + 1) * w - 1) / 2) and torch.equal(iy, ((g[..., 1] + 1) * h - 1) / 2)
    rb = t["bf16_feat_vol"]
    assert (s["out"].reshape(rb.shape) - rb).abs().max() <= 1e-3 * (1 + rb.abs().max())


def _taps(case):
    (B, V, C, E, h, w, R), (img_w, img_h), _ = fc.CASES[case]
    w2c, ixt, _ = fc.cameras(case)
    ix, iy, info = fb.positions(fb.dense_grid(R), w2c.view(-1, 4, 4), ixt.view(-1, 3, 3), img_w, img_h, h, w)
    idx, wgt = fb.taps(ix, iy, h, w)
    return ix, iy, idx, wgt, info


@pytest.mark.parametrize("case", list(fc.CASES))
def test_position_condition_holds(case):
    """no (b, v, s) whose operand of a bf16 rounding lies within 4 x the fp32 error of that operand of a rounding tie, or whose
    pixel position lies that close to an integer; no q.z near zero; power-of-two focal lengths; nothing exempted"""
    (B, V, C, E, h, w, R), _, _ = fc.CASES[case]
    assert torch.equal(fb.dense_grid(R), build_dense_grid(R).reshape(-1, 3))
    ix, iy, idx, wgt, info = _taps(case)
    assert int(fb.position_checks(info).sum()) == 0
    assert float(info["qz"].abs().min()) > 1e-3
    w2c, ixt, _ = fc.cameras(case)
    f = torch.stack([ixt[..., 0, 0], ixt[..., 1, 1]])
    assert torch.equal(torch.frexp(f)[0], torch.full_like(f, 0.5)), "focal lengths are powers of two"
    t = w2c[..., :3, 3] / fc.STEP
    assert torch.equal(t, t.round())


@pytest.mark.parametrize("case", list(fc.CASES))
def test_cases_reach_what_the_table_claims(case):
    (B, V, C, E, h, w, R), (img_w, img_h), _ = fc.CASES[case]
    ix, iy, idx, wgt, _ = _taps(case)
    inside = idx >= 0
    n_in = inside.sum(-1)
    counts = torch.stack([torch.bincount(idx[bv][inside[bv]], minlength=h * w) for bv in range(B * V)])
    if case == "a":
        assert (h * w, R, E) == (1, 1, 0) and int(n_in) == 1 and 0 < float(wgt[inside]) < 1
        return
    fx, fy = torch.floor(ix), torch.floor(iy)
    some = (n_in > 0) & (n_in < 4)
    assert (n_in == 4).any(), "points with all four taps inside"
    assert (n_in == 0).any(), "points fully outside"
    for name, hit in (("left", fx == -1), ("right", fx == w - 1), ("top", fy == -1), ("bottom", fy == h - 1)):
        assert (some & hit).any(), f"no point straddles the {name} border"
    assert (inside.sum((1, 2)) == 0).any(), "a view that sees no point"
    if case == "c":
        assert int(counts.max()) > 128
        flat = idx.view(B * V, -1)          # entries e = 4 s + k, placed 64 at a time
        assert any(len(set(ch[ch >= 0].tolist())) == 1 and int((ch >= 0).sum()) > 1
                   for bv in range(B * V) for ch in flat[bv].split(64)), "a 64-entry chunk whose entries all have one key"
    if case == "e":
        assert h * w == 8192 and float((counts == 0).float().mean()) > 0.9


def test_image_and_map_aspects_differ():
    """img_w / w != img_h / h in at least two cases"""
    assert sum(img_w * h != img_h * w for (_, _, _, _, h, w, _), (img_w, img_h), _ in fc.CASES.values()) >= 2


@pytest.mark.parametrize("regime", fc.REGIMES)
@pytest.mark.parametrize("case", list(fc.CASES))
def test_yardstick_measures_bf16_noise(case, regime):
    """N = ||faithful - unrounded||_2 / ||unrounded||_2 is positive and below 5e-2 for every tensor the noise bar is used on"""
    for k, (fa, un) in fc.yardstick_tensors(case, regime).items():
        n2, nmax = fc.rel(fa, un, un)
        assert 0 < n2 < 5e-2 and nmax > 0, f"{case}/{regime} {k}: N = {n2:.3e}"
