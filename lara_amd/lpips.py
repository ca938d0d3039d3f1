"""LPIPS (Zhang et al. 2018), forward only, for the two networks LaRa's evaluation reports (evaluation.py:48-49, :89-90:
``lpips.LPIPS(net='vgg')`` and ``lpips.LPIPS(net='alex')``), on the device (include/lara_lpips.h, csrc/lpips.hip); opt-in like
every module here.

  * ``LPIPS``         holds one network's weights, repacked once to [Cout][kh][kw][Cin]; an instance is called like the package's
                      (``f(in0, in1)`` on [N, 3, H, W] tensors in [-1, 1] -> [N, 1, 1, 1]), so it is one of ``Evaluator``'s callables;
  * ``lpips_device``  scores the render [B, H, V*W, 3] against the targets [B, V, H, W, 3] where they lie (the "novel views only" crop
                      is a pointer offset, the windows run across view seams as in the reference): device array [nets, B, 8];
  * ``scene_lpips``   the same plus ONE device-to-host copy covering every net.

Limits.  The `lpips` package and `torchvision` are absent from the reference tree's environment here and from the build image:
the VGG-16 variant follows the published method as the reference's vendored copy states it, the AlexNet variant and the package's
state-dict key names are recalled -- PARITY with the `lpips` package is UNPINNED; the kernels are held to a float64 restatement
(tests/lpips_restate.py).  No pretrained weights are shipped or fetched: loading a checkpoint file is the caller's business
(``LPIPS.from_state_dict(net, torch.load(...))``).  Inference only (LaRa's loss does not use LPIPS).  Products are exact fp32
(no bf16).  No CPU path: images must live on the GPU.
"""
from __future__ import annotations

import torch

from ._native import (LPIPS_MAX_LAYERS as MAX_LAYERS, LPIPS_TAPS as TAPS, ImageView as _ImgView, LpipsLayer as _Layer,
                      LpipsNet as _Net, call, query)

ROW = 8                    # include/lara_lpips.h: LARA_LPIPS_ROW: five tap terms, their sum, 0, 0
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)

# (cin, cout, kernel, stride, pad, pool window and stride in FRONT of the convolution, tap after its ReLU, (slice, feature index))
_VGG_WIDTHS = [(3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
               (512, 512), (512, 512), (512, 512)]
_VGG_KEYS = [(1, 0), (1, 2), (2, 5), (2, 7), (3, 10), (3, 12), (3, 14), (4, 17), (4, 19), (4, 21), (5, 24), (5, 26), (5, 28)]
LAYERS = {
    "vgg": [(ci, co, 3, 1, 1, 2 if i in (2, 4, 7, 10) else 0, 2 if i in (2, 4, 7, 10) else 0, i in (1, 3, 6, 9, 12), _VGG_KEYS[i])
            for i, (ci, co) in enumerate(_VGG_WIDTHS)],
    "alex": [(3, 64, 11, 4, 2, 0, 0, True, (1, 0)), (64, 192, 5, 1, 2, 3, 2, True, (2, 3)), (192, 384, 3, 1, 1, 3, 2, True, (3, 6)),
             (384, 256, 3, 1, 1, 0, 0, True, (4, 8)), (256, 256, 3, 1, 1, 0, 0, True, (5, 10))],
}

def _out(side, k, s, pad):
    return (side + 2 * pad - k) // s + 1 if side + 2 * pad >= k else 0


def tap_shapes(net, H, W):
    """[(channels, height, width)] of the five taps of ``net`` on an H x W image; ValueError when the image is too small for the
    net's convolutions and pools."""
    out, h, w = [], int(H), int(W)
    for (_, co, k, s, p, pk, ps, tap, _) in LAYERS[net]:
        if pk:
            h, w = _out(h, pk, ps, 0), _out(w, pk, ps, 0)
        if h > 0 and w > 0:
            h, w = _out(h, k, s, p), _out(w, k, s, p)
        if h <= 0 or w <= 0:
            raise ValueError(f"lara_amd.lpips: an image of {H} x {W} is too small for the '{net}' network's pools")
        if tap:
            out.append((co, h, w))
    return out


def repack(weight):
    """[Cout, Cin, kh, kw] (torch) -> [Cout, kh, kw, Cin], what the kernels read."""
    return weight.detach().permute(0, 2, 3, 1).contiguous()


def unrepack(packed):
    return packed.permute(0, 3, 1, 2).contiguous()


class LPIPS:
    """One LPIPS network ('vgg' or 'alex') with its weights repacked for the kernels.  Build it with ``from_state_dict`` (the
    `lpips` package's key layout) or ``from_tensors``.  ``f(in0, in1)``: [N, 3, H, W] fp32 device tensors in [-1, 1] ->
    [N, 1, 1, 1] fp32 (the package's call shape).  Parity with the package is unpinned (module docstring)."""

    def __init__(self, net="vgg"):
        if net not in LAYERS:
            raise ValueError(f"lara_amd.lpips: net must be 'vgg' or 'alex', got {net!r}")
        self.net = net
        self.weights, self.biases, self.lins = [], [], []      # repacked [Cout, kh, kw, Cin] / [Cout] / [C]
        self.shift, self.scale = SHIFT, SCALE
        self._struct = None

    @classmethod
    def from_tensors(cls, net, convs, lins, shift=None, scale=None):
        """``convs``: (weight [Cout, Cin, kh, kw], bias [Cout]) per convolution in network order; ``lins``: the five 1x1 weights
        ([1, C, 1, 1] or [C]); ``shift`` / ``scale``: the scaling layer's three numbers each (default: the published ones)."""
        self = cls(net)
        spec = LAYERS[net]
        convs, lins = list(convs), list(lins)
        if len(convs) != len(spec) or len(lins) != TAPS:
            raise ValueError(f"lara_amd.lpips: '{net}' takes {len(spec)} convolutions and {TAPS} lin weights, got {len(convs)} and {len(lins)}")
        tap_c = [s[1] for s in spec if s[7]]
        for i, ((w, b), (ci, co, k, *_)) in enumerate(zip(convs, spec)):
            if tuple(w.shape) != (co, ci, k, k) or tuple(b.shape) != (co,):
                raise ValueError(f"lara_amd.lpips: convolution {i} of '{net}' is [{co}, {ci}, {k}, {k}] with bias [{co}], got "
                                 f"{tuple(w.shape)} and {tuple(b.shape)}")
            self.weights.append(repack(w.float()))
            self.biases.append(b.detach().float().contiguous())
        for i, (l, c) in enumerate(zip(lins, tap_c)):
            if l.numel() != c:
                raise ValueError(f"lara_amd.lpips: lin weight {i} of '{net}' has {c} channels, got {tuple(l.shape)}")
            self.lins.append(l.detach().float().reshape(c).contiguous())
        if shift is not None:
            self.shift = tuple(float(v) for v in torch.as_tensor(shift).reshape(-1))
        if scale is not None:
            self.scale = tuple(float(v) for v in torch.as_tensor(scale).reshape(-1))
        if len(self.shift) != 3 or len(self.scale) != 3:
            raise ValueError("lara_amd.lpips: the scaling layer has three shifts and three scales")
        return self

    @classmethod
    def from_state_dict(cls, net, sd):
        """From the `lpips` package's state dict: ``net.sliceK.I.weight`` / ``.bias`` (I: torchvision's feature index),
        ``linK.model.1.weight`` or ``lins.K.model.1.weight``, optional ``scaling_layer.shift`` / ``.scale``.  (Key names recalled,
        not pinned: module docstring.)"""
        if net not in LAYERS:
            raise ValueError(f"lara_amd.lpips: net must be 'vgg' or 'alex', got {net!r}")

        def get(*names):
            for n in names:
                if n in sd:
                    return sd[n]
            raise ValueError(f"lara_amd.lpips.from_state_dict: the state dict lacks {' / '.join(repr(n) for n in names)} ('{net}' network)")
        convs = [(get(f"net.slice{s}.{i}.weight"), get(f"net.slice{s}.{i}.bias")) for (*_, (s, i)) in LAYERS[net]]
        lins = [get(f"lin{k}.model.1.weight", f"lins.{k}.model.1.weight") for k in range(TAPS)]
        return cls.from_tensors(net, convs, lins, sd.get("scaling_layer.shift"), sd.get("scaling_layer.scale"))

    def to(self, device):
        """Moves the weight buffers (in place); returns self."""
        device = torch.device(device)
        if self.weights and self.weights[0].device != device:
            self.weights = [t.to(device) for t in self.weights]
            self.biases = [t.to(device) for t in self.biases]
            self.lins = [t.to(device) for t in self.lins]
            self._struct = None
        return self

    def workspace_bytes(self, B, H, W):
        return query("lara_lpips_workspace_bytes", self._c_net(), B, H, W,
                     error=ValueError(f"lara_amd.lpips: sizes out of range for lara_lpips_forward (B={B}, {H} x {W})"))

    def _c_net(self):
        if not self.weights:
            raise ValueError("lara_amd.lpips: this LPIPS holds no weights; build it with from_state_dict or from_tensors")
        if self._struct is None:
            n = _Net()
            n.n_layers = len(self.weights)
            for i, (ci, co, k, s, p, pk, ps, tap, _) in enumerate(LAYERS[self.net]):
                n.layers[i] = _Layer(self.weights[i].data_ptr(), self.biases[i].data_ptr(), ci, co, k, s, p, pk, ps, int(tap))
            for k in range(TAPS):
                n.lin[k] = self.lins[k].data_ptr()
            n.shift[:] = self.shift
            n.scale[:] = self.scale
            self._struct = n
        return self._struct

    def _forward(self, B, H, W, xv, yv, mul, add, scores, dev):
        tap_shapes(self.net, H, W)                             # ValueError on an image too small
        self.to(dev)
        ws = torch.empty(self.workspace_bytes(B, H, W), dtype=torch.uint8, device=dev)
        call("lara_lpips_forward", dev, self._c_net(), B, H, W, xv, yv, mul, add, scores, ws)

    @torch.no_grad()
    def rows(self, in0, in1):
        """The device array [N, 8] (float64: five tap terms, their sum, 0, 0) for [N, 3, H, W] fp32 tensors in [-1, 1]."""
        _check_images(in0, in1)
        if in0.dim() != 4 or in0.shape[1] != 3 or in0.shape != in1.shape:
            raise ValueError("lara_amd.lpips: expected two [N, 3, H, W] tensors of one shape")
        in0, in1 = in0.detach().contiguous(), in1.detach().contiguous()
        N, _, H, W = in0.shape
        scores = torch.empty(N, ROW, dtype=torch.float64, device=in0.device)
        views = [_ImgView(t.data_ptr(), 3 * H * W, H * W, W, 0, 1, W) for t in (in0, in1)]
        self._forward(N, H, W, views[0], views[1], 1.0, 0.0, scores, in0.device)
        return scores

    def __call__(self, in0, in1):
        rows = self.rows(in0, in1)
        return rows[:, 5].float().reshape(-1, 1, 1, 1)


def _check_images(*tensors):
    for t in tensors:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError("lara_amd.lpips: images must be tensors on an MI355X (HIP) device; there is no CPU path")
        if t.dtype != torch.float32:
            raise ValueError(f"lara_amd.lpips: images must be float32, got {t.dtype}")


def _net_list(nets):
    nets = list(nets.values()) if isinstance(nets, dict) else list(nets)
    if not nets or any(not isinstance(n, LPIPS) for n in nets):
        raise ValueError("lara_amd.lpips: nets must be LPIPS instances")
    return nets


@torch.no_grad()
def lpips_device(nets, image, tar_rgb, skip_views=0):
    """Device array [len(nets), B, 8] (float64; row layout: include/lara_lpips.h) of the render ``image`` [B, H, V*W, 3] against
    ``tar_rgb`` [B, V, H, W, 3] in [0, 1], without their first ``skip_views`` views (evaluation.py:75-78, :89-90: 2 x - 1 happens
    inside the first kernel; nothing is permuted or copied).  ``nets``: LPIPS instances (a list, or a dict's values in order).
    No host synchronisation."""
    nets = _net_list(nets)
    _check_images(image, tar_rgb)
    if tar_rgb.dim() != 5:
        raise ValueError("lara_amd.lpips: expected tar_rgb [B,V,H,W,3] and image [B,H,V*W,3]")
    B, V, H, W = tar_rgb.shape[:4]
    if tuple(tar_rgb.shape) != (B, V, H, W, 3) or tuple(image.shape) != (B, H, V * W, 3):
        raise ValueError("lara_amd.lpips: expected tar_rgb [B,V,H,W,3] and image [B,H,V*W,3]")
    if not 0 <= skip_views < V:
        raise ValueError("lara_amd.lpips: the crop leaves no view to score")
    image, tar_rgb = image.detach().contiguous(), tar_rgb.detach().contiguous()
    Wc = (V - skip_views) * W
    xv = _ImgView(image.data_ptr() + 4 * skip_views * W * 3, H * V * W * 3, 1, V * W * 3, W * 3, 3, W)
    yv = _ImgView(tar_rgb.data_ptr() + 4 * skip_views * H * W * 3, V * H * W * 3, 1, W * 3, H * W * 3, 3, W)
    scores = torch.empty(len(nets), B, ROW, dtype=torch.float64, device=image.device)
    for i, net in enumerate(nets):
        # (evaluation.py:89-90 passes the target first; the metric is symmetric term by term)
        net._forward(B, H, Wc, xv, yv, 2.0, -1.0, scores[i], image.device)
    return scores


@torch.no_grad()
def scene_lpips(nets, image, tar_rgb, skip_views=0):
    """Per scene {name: LPIPS} for ``nets`` = {name: LPIPS instance}: ``lpips_device`` and one device-to-host copy for all nets."""
    names = list(nets.keys())
    rows = lpips_device([nets[k] for k in names], image, tar_rgb, skip_views).cpu().tolist()      # the one host read of the call
    B = len(rows[0])
    return [{k: rows[i][b][5] for i, k in enumerate(names)} for b in range(B)]


# ---------------------------------------------------------------------------------------------------------- building blocks

def conv2d_nhwc(x, packed, bias, stride=1, pad=0, relu=True):
    """``lara_lpips_conv2d`` on a dense NHWC fp32 device tensor with repacked weights [Cout, kh, kw, Cin] (what the tests hold
    against ``F.conv2d``)."""
    _check_images(x, packed, bias)
    x, packed, bias = x.contiguous(), packed.contiguous(), bias.contiguous()
    N, H, W, Cin = x.shape
    Cout, k = packed.shape[0], packed.shape[1]
    Ho, Wo = _out(H, k, stride, pad), _out(W, k, stride, pad)
    if tuple(packed.shape) != (Cout, k, k, Cin) or Ho <= 0 or Wo <= 0:
        raise ValueError("lara_amd.lpips: conv2d_nhwc: weights [Cout,k,k,Cin] do not fit x [N,H,W,Cin]")
    if not ((Cin == 3 and Cout % 16 == 0) or (Cin % 32 == 0 and Cout % 64 == 0)):
        raise ValueError(f"lara_amd.lpips: conv2d_nhwc: no kernel for Cin={Cin}, Cout={Cout} (Cin 3 or a multiple of 32, Cout of 64)")
    y = torch.empty(N, Ho, Wo, Cout, dtype=torch.float32, device=x.device)
    call("lara_lpips_conv2d", x.device, N, H, W, Cin, Cout, k, stride, pad, int(relu), x, packed, bias, y)
    return y


def maxpool_nhwc(x, k, s):
    """``lara_lpips_maxpool``: floor-mode max pool of a dense NHWC fp32 device tensor (channels a multiple of 4)."""
    _check_images(x)
    x = x.contiguous()
    N, H, W, C = x.shape
    if H < k or W < k or C % 4:
        raise ValueError("lara_amd.lpips: maxpool_nhwc: the window does not fit, or channels are no multiple of 4")
    y = torch.empty(N, (H - k) // s + 1, (W - k) // s + 1, C, dtype=torch.float32, device=x.device)
    call("lara_lpips_maxpool", x.device, N, H, W, C, k, s, x, y)
    return y
