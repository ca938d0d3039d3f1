"""`lara_amd.lpips` on the GPU (csrc/lpips.hip): the convolution against `F.conv2d` in float64, the pools against torch (exact),
the whole metric of both networks against the float64 restatement (tests/lpips_restate.py), the in-place strided route
(bit-equal to the contiguous one, scenes independent, reproducible) and `Evaluator` with two `LPIPS` instances.  Reads nothing
outside this repository.

Bars.  A score (the final one and each of the five tap terms): 8 * max(E32, spacing32(value)), the form of
tests/test_evaluate_gpu.py -- E32 is the error, against the restatement, of the SAME network in float32 torch on the CPU,
spacing32 the float32 spacing at the value.  A convolution alone: the relative L2 error of the output against float64, held to 8
times that of float32 `F.conv2d` on the CPU.  Every case prints err, E32 and bar (copied to profiles/lpips_parity.txt).

The 48 x 200 case is 75 whole pixel tiles of 128 for this kernel; the partial last tile is what the 13 x 17 case (442 pixels) and
the stride-2 case (280 pixels) end in."""
import functools
import json
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lara_amd import evaluate
from lara_amd import lpips as L
from tests import lpips_restate as R
from tests.test_lpips import CASES, NETS, NOISES, images, pairs, state_dict, strip

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _bar(e32, value):
    return 8.0 * max(float(e32), float(np.spacing(np.float32(abs(value)))))


@functools.lru_cache(maxsize=None)
def _model(net):
    return L.LPIPS.from_state_dict(net, state_dict(net)).to(DEV)


# (k, stride, pad, cin, cout, H, W, N)
CONVS = [(3, 1, 1, 64, 128, 13, 17, 2), (11, 4, 2, 3, 64, 37, 53, 2), (5, 1, 2, 64, 192, 7, 9, 2), (3, 1, 1, 384, 256, 3, 5, 2),
         (3, 1, 1, 64, 64, 48, 200, 1), (3, 2, 0, 128, 64, 21, 30, 2)]


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("k,stride,pad,cin,cout,H,W,N", CONVS)
def test_convolution_against_float64(hip_lib, k, stride, pad, cin, cout, H, W, N, relu):
    g = torch.Generator().manual_seed(1000 + cin + k + H)
    x = torch.randn(N, cin, H, W, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) * math.sqrt(2.0 / (cin * k * k))
    b = torch.randn(cout, generator=g) * 0.1
    act = F.relu if relu else (lambda t: t)
    y64 = act(F.conv2d(x.double(), w.double(), b.double(), stride=stride, padding=pad))
    y32 = act(F.conv2d(x, w, b, stride=stride, padding=pad))
    got = L.conv2d_nhwc(x.permute(0, 2, 3, 1).contiguous().to(DEV), L.repack(w).to(DEV), b.to(DEV), stride, pad, relu)
    assert tuple(got.shape) == (N, y64.shape[2], y64.shape[3], cout)
    got = got.cpu().permute(0, 3, 1, 2).double()
    norm = float(y64.norm())
    err, e32 = float((got - y64).norm()) / norm, float((y32.double() - y64).norm()) / norm
    bar = 8.0 * e32
    print(f"lpips_parity conv k={k} s={stride} p={pad} {cin}->{cout} {N}x{H}x{W} relu={int(relu)} err={err:.3e} E32={e32:.3e} "
          f"bar={bar:.3e} ratio={err / bar:.3f}")
    assert err <= bar, (err, bar)
    assert float((got - y64).abs().max()) < 1e-4 * max(1.0, float(y64.abs().max()))      # no single wrong element hides in the norm


@pytest.mark.parametrize("k,s,N,H,W,C", [(2, 2, 2, 37, 53, 64), (3, 2, 2, 37, 53, 64), (2, 2, 1, 13, 17, 192), (3, 2, 3, 13, 17, 192),
                                         (3, 2, 1, 3, 3, 4)])
def test_max_pool_is_exact(hip_lib, k, s, N, H, W, C):
    x = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(H + k))
    want = F.max_pool2d(x, k, s)
    got = L.maxpool_nhwc(x.permute(0, 2, 3, 1).contiguous().to(DEV), k, s).cpu().permute(0, 3, 1, 2)
    assert torch.equal(got, want)


@functools.lru_cache(maxsize=None)
def _reference(net, N, H, W, noise):
    """(terms64 [N, 5], total64 [N], E32 of the terms, E32 of the total): computed once per case."""
    a, b = pairs(N, H, W, noise)
    sd = state_dict(net)
    t64, s64 = R.lpips(net, sd, a, b)
    t32, s32 = R.lpips(net, sd, a, b, dtype=torch.float32)
    return t64, s64, (t32.double() - t64).abs(), (s32.double() - s64).abs()


@pytest.mark.parametrize("noise", NOISES)
@pytest.mark.parametrize("N,H,W", CASES)
@pytest.mark.parametrize("net", NETS)
def test_metric_against_the_float64_restatement(hip_lib, net, N, H, W, noise):
    t64, s64, e_t, e_s = _reference(net, N, H, W, noise)
    a, b = pairs(N, H, W, noise)
    m = _model(net)
    rows = m.rows(a.to(DEV), b.to(DEV)).cpu()
    out = m(a.to(DEV), b.to(DEV))
    assert tuple(out.shape) == (N, 1, 1, 1) and out.dtype == torch.float32 and out.is_cuda
    assert torch.equal(out.cpu().reshape(-1), rows[:, 5].float()) and not rows[:, 6:].any()
    failures = []
    for n in range(N):
        for k in range(6):
            want, e32 = (float(t64[n, k]), float(e_t[n, k])) if k < 5 else (float(s64[n]), float(e_s[n]))
            err, bar = abs(float(rows[n, k]) - want), _bar(e32, want)
            print(f"lpips_parity {net} {N}x{H}x{W} noise={noise} image={n} {'tap%d' % k if k < 5 else 'score'}={want:.8f} "
                  f"err={err:.3e} E32={e32:.3e} bar={bar:.3e} ratio={err / bar:.3f}")
            if not err <= bar:
                failures.append((n, k, err, bar))
    assert not failures, failures


@pytest.mark.parametrize("crop", [0, 2])
def test_in_place_route_is_bit_equal_reproducible_and_scene_independent(hip_lib, crop):
    B, V, H, W = 2, 4, 32, 40
    tar, img = images(B, V, H, W, 0.1, seed=77)
    tar, img = tar.to(DEV), img.to(DEV)
    nets = [_model("vgg"), _model("alex")]
    got = L.lpips_device(nets, img, tar, crop)
    assert tuple(got.shape) == (2, B, 8) and got.dtype == torch.float64 and torch.isfinite(got).all() and (got[:, :, :6] > 0).all()
    assert torch.equal(got, L.lpips_device(nets, img, tar, crop))
    x = (img.permute(0, 3, 1, 2)[..., crop * W:] * 2 - 1).contiguous()                      # contiguous cropped copies
    y = (strip(tar).permute(0, 3, 1, 2)[..., crop * W:] * 2 - 1).contiguous()
    for i, m in enumerate(nets):
        assert torch.equal(got[i], m.rows(x, y))
        assert torch.equal(got[i, :, 5].float().reshape(B, 1, 1, 1), m(x, y))
    for s in range(B):
        one = L.lpips_device(nets, img[s:s + 1].contiguous(), tar[s:s + 1].contiguous(), crop)
        assert torch.equal(one[:, 0], got[:, s])
    scenes = L.scene_lpips({"vgg": nets[0], "alex": nets[1]}, img, tar, crop)
    assert [[sc["vgg"], sc["alex"]] for sc in scenes] == got[:, :, 5].T.cpu().tolist()


def test_errors_on_the_device(hip_lib):
    m = _model("alex")
    with pytest.raises(ValueError, match="float32"):
        m(torch.zeros(1, 3, 32, 32, device=DEV, dtype=torch.float64), torch.zeros(1, 3, 32, 32, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError, match="too small"):
        m(torch.zeros(1, 3, 64, 14, device=DEV), torch.zeros(1, 3, 64, 14, device=DEV))
    with pytest.raises(ValueError, match="too small"):
        _model("vgg")(torch.zeros(1, 3, 15, 64, device=DEV), torch.zeros(1, 3, 15, 64, device=DEV))
    with pytest.raises(ValueError, match="no view"):
        L.lpips_device([m], torch.zeros(1, 32, 64, 3, device=DEV), torch.zeros(1, 2, 32, 32, 3, device=DEV), 2)


def test_evaluator_with_two_networks_writes_no_null(hip_lib, tmp_path):
    B, V, H, W, n_views = 2, 4, 32, 40, 2
    tar, img = images(B, V, H, W, 0.1, seed=78)
    batch = {"tar_rgb": tar.to(DEV), "meta": {"scene": ["a.glb", "b.glb"]}}
    output = {"image_fine": img.to(DEV)}
    nets = {"vgg": _model("vgg"), "alex": _model("alex")}
    ev = evaluate.Evaluator(n_views=n_views, lpips=nets)
    ev.add(batch, output)
    want = L.scene_lpips(nets, output["image_fine"], batch["tar_rgb"], n_views)
    s = ev.write(str(tmp_path / "metrics.json"))
    assert s["name"] == ["a", "b"]
    assert s["lpips_vgg"] == [w["vgg"] for w in want] and s["lpips_alex"] == [w["alex"] for w in want]
    assert all(math.isfinite(v) and v > 0 for v in s["lpips_vgg"] + s["lpips_alex"])
    assert s["lpips_vgg_mean"] == sum(s["lpips_vgg"]) / B and s["lpips_alex_mean"] == sum(s["lpips_alex"]) / B
    text = (tmp_path / "metrics.json").read_text()
    assert "null" not in text and json.loads(text) == s
    # a user's own callable keeps the per-scene path, next to a network on the device
    seen = []
    mixed = evaluate.Evaluator(n_views=n_views, lpips={"vgg": nets["vgg"], "alex": lambda gt, im: seen.append(tuple(gt.shape)) or 0.25})
    mixed.add(batch, output)
    assert mixed.summary()["lpips_vgg"] == s["lpips_vgg"] and mixed.summary()["lpips_alex"] == [0.25, 0.25]
    assert seen == [(1, 3, H, (V - n_views) * W)] * B
