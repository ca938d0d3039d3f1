"""LPIPS (Zhang et al. 2018) restated in torch on the CPU, from the published method, for both networks `lara_amd.lpips` runs --
the float64 reference of tests/test_lpips.py and tests/test_lpips_gpu.py (and, in float32, the yardstick E32 of their bars).
Independent of lara_amd: its own layer tables, channels-first, `F.conv2d` / `F.max_pool2d`.

Also the seeded weight maker: He-normal convolution weights (std sqrt(2 / fan_in): activations stay O(1) through 13 layers),
biases N(0, 0.1^2), lin weights U(0, 1) / C (non-negative), emitted in the `lpips` package's state-dict key layout (recalled, not
pinned: the package is not available here)."""
import math

import torch
import torch.nn.functional as F

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
EPS = 1e-10

# ("conv", key, cin, cout, k, stride, pad) | ("pool", k, stride) | ("tap",)
VGG = [("conv", "net.slice1.0", 3, 64, 3, 1, 1), ("conv", "net.slice1.2", 64, 64, 3, 1, 1), ("tap",), ("pool", 2, 2),
       ("conv", "net.slice2.5", 64, 128, 3, 1, 1), ("conv", "net.slice2.7", 128, 128, 3, 1, 1), ("tap",), ("pool", 2, 2),
       ("conv", "net.slice3.10", 128, 256, 3, 1, 1), ("conv", "net.slice3.12", 256, 256, 3, 1, 1),
       ("conv", "net.slice3.14", 256, 256, 3, 1, 1), ("tap",), ("pool", 2, 2),
       ("conv", "net.slice4.17", 256, 512, 3, 1, 1), ("conv", "net.slice4.19", 512, 512, 3, 1, 1),
       ("conv", "net.slice4.21", 512, 512, 3, 1, 1), ("tap",), ("pool", 2, 2),
       ("conv", "net.slice5.24", 512, 512, 3, 1, 1), ("conv", "net.slice5.26", 512, 512, 3, 1, 1),
       ("conv", "net.slice5.28", 512, 512, 3, 1, 1), ("tap",)]
ALEX = [("conv", "net.slice1.0", 3, 64, 11, 4, 2), ("tap",), ("pool", 3, 2),
        ("conv", "net.slice2.3", 64, 192, 5, 1, 2), ("tap",), ("pool", 3, 2),
        ("conv", "net.slice3.6", 192, 384, 3, 1, 1), ("tap",),
        ("conv", "net.slice4.8", 384, 256, 3, 1, 1), ("tap",),
        ("conv", "net.slice5.10", 256, 256, 3, 1, 1), ("tap",)]
NETS = {"vgg": VGG, "alex": ALEX}
TAP_CHANNELS = {"vgg": (64, 128, 256, 512, 512), "alex": (64, 192, 384, 256, 256)}


def make_state_dict(net, seed=0, lin_keys="lin{k}.model.1.weight", scaling=False):
    """Seeded float32 weights of ``net`` in the package's key layout."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for step in NETS[net]:
        if step[0] != "conv":
            continue
        _, key, cin, cout, k, _, _ = step
        sd[key + ".weight"] = torch.randn(cout, cin, k, k, generator=g) * math.sqrt(2.0 / (cin * k * k))
        sd[key + ".bias"] = torch.randn(cout, generator=g) * 0.1
    for i, c in enumerate(TAP_CHANNELS[net]):
        sd[lin_keys.format(k=i)] = torch.rand(1, c, 1, 1, generator=g) / c
    if scaling:
        sd["scaling_layer.shift"] = torch.tensor(SHIFT)[None, :, None, None]
        sd["scaling_layer.scale"] = torch.tensor(SCALE)[None, :, None, None]
    return sd


def _lin(sd, k):
    for name in (f"lin{k}.model.1.weight", f"lins.{k}.model.1.weight"):
        if name in sd:
            return sd[name]
    raise KeyError(name)


def features(net, sd, t, dtype=torch.float64):
    """The five taps [N, C, h, w] of images ``t`` [N, 3, H, W] in [-1, 1]."""
    shift = torch.tensor(SHIFT, dtype=dtype, device=t.device)[None, :, None, None]
    scale = torch.tensor(SCALE, dtype=dtype, device=t.device)[None, :, None, None]
    h = (t.to(dtype) - shift) / scale
    taps = []
    for step in NETS[net]:
        if step[0] == "conv":
            _, key, _, _, _, stride, pad = step
            h = F.relu(F.conv2d(h, sd[key + ".weight"].to(dtype), sd[key + ".bias"].to(dtype), stride=stride, padding=pad))
        elif step[0] == "pool":
            h = F.max_pool2d(h, step[1], step[2])
        else:
            taps.append(h)
    return taps


def lpips(net, sd, in0, in1, dtype=torch.float64):
    """(terms [N, 5], score [N]) of [N, 3, H, W] images in [-1, 1], computed in ``dtype``."""
    f0, f1 = features(net, sd, in0, dtype), features(net, sd, in1, dtype)
    terms = []
    for k, (a, b) in enumerate(zip(f0, f1)):
        na = a / (torch.sqrt((a * a).sum(1, keepdim=True)) + EPS)
        nb = b / (torch.sqrt((b * b).sum(1, keepdim=True)) + EPS)
        d = (na - nb) ** 2
        w = _lin(sd, k).to(dtype).reshape(1, -1, 1, 1)
        terms.append((d * w).sum(1).mean((1, 2)))
    terms = torch.stack(terms, 1)
    return terms, terms.sum(1)


def min_feature_norm(net, sd, t):
    """The smallest channel norm over all pixels of all taps: must be far above EPS for the `+ eps` not to be what is tested."""
    return min(float(torch.sqrt((f * f).sum(1)).min()) for f in features(net, sd, t))
