"""`lara_amd.lpips` without a GPU: the float64 restatement's own properties (tests/lpips_restate.py), the tap shapes, the mapping
of the `lpips` package's state-dict keys onto the repacked buffers, the errors, and that an `Evaluator` without LPIPS networks
still writes null.  The GPU side is tests/test_lpips_gpu.py, which takes its inputs from `pairs` below."""
import functools

import pytest
import torch

from lara_amd import lpips as L
from lara_amd.evaluate import Evaluator
from tests import lpips_restate as R

NETS = ("vgg", "alex")
SEEDS = {"vgg": 11, "alex": 12}


@functools.lru_cache(maxsize=None)
def state_dict(net):
    return R.make_state_dict(net, SEEDS[net])


def images(B, V, H, W, noise, seed):
    """The seeded smooth-plus-noise pair of tests/test_evaluate_gpu.py (re-implemented): targets [B, V, H, W, 3] and the render
    [B, H, V*W, 3] = targets + noise, clamped to [0, 1]."""
    g = torch.Generator().manual_seed(seed)
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    f = torch.rand(B, V, 1, 1, 3, generator=g) * 0.25 + 0.05
    ph = torch.rand(B, V, 1, 1, 3, generator=g) * 6.28
    tar = 0.5 + 0.35 * torch.sin(f * x[None, None, ..., None] + 0.7 * f * y[None, None, ..., None] + ph)
    img = tar.permute(0, 2, 1, 3, 4).reshape(B, H, V * W, 3)
    img = (img + noise * torch.randn(img.shape, generator=g)).clamp(0, 1)
    return tar.contiguous(), img.contiguous()


def strip(tar):
    """[B, V, H, W, 3] -> [B, H, V*W, 3]: the views side by side, as the render holds them."""
    B, V, H, W, _ = tar.shape
    return tar.permute(0, 2, 1, 3, 4).reshape(B, H, V * W, 3)


@functools.lru_cache(maxsize=None)
def pairs(N, H, W, noise):
    """(in0, in1): [N, 3, H, W] float32 in [-1, 1], the target and the render of `images` with one view."""
    tar, img = images(N, 1, H, W, noise, seed=300 + H + N)
    return (strip(tar).permute(0, 3, 1, 2) * 2 - 1).contiguous(), (img.permute(0, 3, 1, 2) * 2 - 1).contiguous()


CASES = [(1, 32, 32), (2, 37, 53)]
NOISES = (0.02, 0.3)


@pytest.mark.parametrize("net", NETS)
def test_restatement_is_zero_for_identical_images_and_symmetric(net):
    a, b = pairs(2, 37, 53, 0.3)
    sd = state_dict(net)
    terms, total = R.lpips(net, sd, a, a)
    assert torch.equal(terms, torch.zeros_like(terms)) and torch.equal(total, torch.zeros_like(total))
    t_ab, s_ab = R.lpips(net, sd, a, b)
    t_ba, s_ba = R.lpips(net, sd, b, a)
    assert torch.equal(t_ab, t_ba) and torch.equal(s_ab, s_ba)
    assert (t_ab > 0).all() and torch.isfinite(s_ab).all()


@pytest.mark.parametrize("net", NETS)
@pytest.mark.parametrize("H,W", [(32, 32), (37, 53)])
def test_tap_shapes(net, H, W):
    taps = R.features(net, state_dict(net), torch.zeros(1, 3, H, W))
    assert [tuple(t.shape[1:]) for t in taps] == L.tap_shapes(net, H, W)
    assert [t.shape[1] for t in taps] == list(R.TAP_CHANNELS[net])
    want = {("vgg", 32): [(32, 32), (16, 16), (8, 8), (4, 4), (2, 2)], ("vgg", 37): [(37, 53), (18, 26), (9, 13), (4, 6), (2, 3)],
            ("alex", 32): [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)], ("alex", 37): [(8, 12), (3, 5), (1, 2), (1, 2), (1, 2)]}[(net, H)]
    assert [tuple(t.shape[2:]) for t in taps] == want


@pytest.mark.parametrize("net", NETS)
@pytest.mark.parametrize("N,H,W", CASES)
@pytest.mark.parametrize("noise", NOISES)
def test_seeded_weights_leave_no_dead_tap(net, N, H, W, noise):
    """The inputs of the GPU tests: every feature vector's norm is far above the 1e-10 of the normalisation."""
    sd = state_dict(net)
    for t in pairs(N, H, W, noise):
        assert R.min_feature_norm(net, sd, t) > 1e-3


@pytest.mark.parametrize("net", NETS)
@pytest.mark.parametrize("lin_keys", ["lin{k}.model.1.weight", "lins.{k}.model.1.weight"])
def test_state_dict_keys_map_onto_the_repacked_buffers(net, lin_keys):
    sd = R.make_state_dict(net, 5, lin_keys=lin_keys, scaling=True)
    m = L.LPIPS.from_state_dict(net, sd)
    convs = [s for s in R.NETS[net] if s[0] == "conv"]
    assert len(m.weights) == len(convs) == len(m.biases) and len(m.lins) == 5
    for packed, bias, (_, key, cin, cout, k, _, _) in zip(m.weights, m.biases, convs):
        assert tuple(packed.shape) == (cout, k, k, cin) and packed.is_contiguous()
        assert torch.equal(L.unrepack(packed), sd[key + ".weight"]) and torch.equal(bias, sd[key + ".bias"])
        assert packed[3, k - 1, 0, 1] == sd[key + ".weight"][3, 1, k - 1, 0]
    for i, lin in enumerate(m.lins):
        assert torch.equal(lin, sd[lin_keys.format(k=i)].reshape(-1))
    assert m.shift == tuple(float(v) for v in torch.tensor(R.SHIFT)) and m.scale == tuple(float(v) for v in torch.tensor(R.SCALE))
    spec = [(ci, co, k, s, p) for (ci, co, k, s, p, *_) in L.LAYERS[net]]
    assert spec == [(ci, co, k, s, p) for (_, _, ci, co, k, s, p) in convs]


@pytest.mark.parametrize("net,key", [("vgg", "net.slice3.12.weight"), ("alex", "net.slice2.3.bias"), ("alex", "lin4.model.1.weight")])
def test_a_missing_key_raises_and_is_named(net, key):
    sd = dict(state_dict(net))
    del sd[key]
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        L.LPIPS.from_state_dict(net, sd)


def test_errors():
    with pytest.raises(ValueError):
        L.LPIPS("squeeze")
    with pytest.raises(ValueError, match="too small"):
        L.tap_shapes("vgg", 15, 64)
    with pytest.raises(ValueError, match="too small"):
        L.tap_shapes("alex", 64, 14)
    m = L.LPIPS.from_state_dict("alex", state_dict("alex"))
    with pytest.raises(ValueError, match="device"):
        m(torch.zeros(1, 3, 32, 32), torch.zeros(1, 3, 32, 32))
    with pytest.raises(ValueError, match="device"):
        L.lpips_device([m], torch.zeros(1, 32, 64, 3), torch.zeros(1, 2, 32, 32, 3))
    with pytest.raises(ValueError):
        L.LPIPS.from_tensors("alex", [], [])


def test_evaluator_without_lpips_still_writes_null():
    ev = Evaluator(n_views=4)
    ev.add_scores("a", psnr=30.0, ssim=0.9)
    ev.add_scores("b", psnr=28.0, ssim=0.8)
    s = ev.summary()
    assert s["lpips_vgg"] == [None, None] and s["lpips_alex"] == [None, None]
    assert s["lpips_vgg_mean"] is None and s["lpips_alex_mean"] is None
