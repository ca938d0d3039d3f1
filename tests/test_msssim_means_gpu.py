"""The MS-SSIM kernels (`lara_amd/csrc/msssim.hip`: msssim_pool, msssim_maps<0>, msssim_maps<1>, msssim_means, msssim_back) scale by
scale: their real output `means[5][N*C][2]` and the gradient for ARBITRARY `d_means`, against `tests/loss_restate.ms_ssim_means64`
in float64 on the CPU (tests/test_loss_restate.py holds it to the torch formulation, to explicit loops and to central differences).
tests/test_msssim_gpu.py sees only the final product, in which scale 0 has exponent 0.0448 and half of the means and of the
backward (the SSIM path of scales 0-3, the cs path of scale 4) do not take part at all.

The bar is measured, not chosen: the same inputs go through the project's torch formulation in fp32 ON THE CPU
(`lara_amd.loss._ssim_cs`, `avg_pool2d` between the scales), and its distance y to float64 is the yardstick: both are fp32
evaluations of the same formula in different summation orders; the kernel adds a reciprocal with one Newton step (2 ulp) and
tile-wise partial sums.  Two independent error draws of that size: 4 y covers their sum, plus 16 * 2^-24 for a mean (1e-6 for a
gradient).  So that a large yardstick cannot hide a failure, it is itself bounded: y <= 2e-6 at scales 0-3, 2.5e-5 at scale 4 and
for gradients -- otherwise the test fails as ill-conditioned.  The inputs (`multiscale_images`) have variance at every scale, which
keeps sigma^2 = E[x^2] - mu^2 from cancelling at the coarse ones.  No GPU torch result is used as a reference anywhere (torch's own
`avg_pool2d` backward is wrong for odd sides on this ROCm build)."""
import functools

import pytest
import torch

from tests import loss_restate as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

#        (H, V, W, B, kind)              what it reaches
CASES = [(161, 1, 161, 1, "ms"),       # the smallest legal side; scale 4 is 11 x 11: one filtered position
         (161, 9, 20, 1, "ms"),        # views half a tile wide: several seams inside one LDS load
         (163, 3, 59, 2, "ms"),        # odd sides on several scales, two images
         (171, 1, 202, 1, "ms"),       # filtered height 161 = five tiles + 1 row, filtered width 192 = six tiles; pads at scales 0, 2
         (193, 1, 161, 1, "ms"),       # the back kernel's image height one row past six tiles
         (177, 2, 97, 1, "anti")]      # every mean negative (the worst conditioned: gradient yardstick 1.2e-5 ... 2.2e-5 by host CPU)
MEAN_EPS = 16 * 2.0 ** -24
Y_MAX_MEAN = (2e-6, 2e-6, 2e-6, 2e-6, 2.5e-5)
Y_MAX_GRAD = 2.5e-5


def _torch_means(X, Y):
    """The project's torch formulation of the means, [5, N*C, 2], in the tensors' dtype (fp32: the yardstick)."""
    from lara_amd.loss import _gauss_window, _ssim_cs
    base = _gauss_window("cpu")
    win = base.to(X.dtype)
    win._lara_window = base._lara_window
    out = []
    for lvl in range(5):
        s, cs = _ssim_cs(X, Y, win)
        out.append(torch.stack([s.reshape(-1), cs.reshape(-1)], -1))
        if lvl < 4:
            pad = [d % 2 for d in X.shape[2:]]
            X = torch.nn.functional.avg_pool2d(X, kernel_size=2, padding=pad)
            Y = torch.nn.functional.avg_pool2d(Y, kernel_size=2, padding=pad)
    return torch.stack(out, 0)


def _grad_errors(got, want):
    """(largest error over max |grad|, relative L2) of a gradient against the float64 one."""
    got, want = got.double(), want.double()
    return float((got - want).abs().max() / want.abs().max()), float((got - want).norm() / want.norm())


class _Reference:
    """Inputs (planar, fp32), the float64 means, the fp32 torch formulation's means, and gradients of sum(means * gm) for any gm
    from both (CPU; the graphs are kept so that further gm cost one backward each)."""

    def __init__(self, N, C, H, W, seed, kind):
        self.X, self.Y = R.multiscale_images(N, C, H, W, seed, kind)
        self.x64, self.x32 = self.X.double().requires_grad_(True), self.X.clone().requires_grad_(True)
        self._m64, self._m32 = R.ms_ssim_means64(self.x64, self.Y.double()), _torch_means(self.x32, self.Y)
        self.means64 = self._m64.detach()
        self.y = (self._m32.detach().double() - self.means64).abs().amax((1, 2))         # the yardstick per scale
        self.gm = torch.randn(self.means64.shape, generator=torch.Generator().manual_seed(seed + 1))
        self._grads = {}

    def grads(self, gm):
        """(float64 gradient, (yardstick: max-relative, L2-relative)) for the upstream `gm` [5, N*C, 2] (fp32 values)."""
        key = tuple(gm.flatten().tolist())
        if key not in self._grads:
            g64, = torch.autograd.grad(self._m64, self.x64, gm.double(), retain_graph=True)
            g32, = torch.autograd.grad(self._m32, self.x32, gm, retain_graph=True)
            self._grads[key] = (g64, _grad_errors(g32, g64))
        return self._grads[key]


@functools.lru_cache(maxsize=None)
def _reference(H, V, W, B, kind, C=3):
    return _Reference(B, C, H, V * W, seed=2, kind=kind)


def _check_means(tag, got, ref):
    """Every scale's 2 N C numbers under 4 y_l + 16 * 2^-24, with y_l itself bounded."""
    got = got.detach().cpu().double()
    assert got.shape == ref.means64.shape
    dist = (got - ref.means64).abs().amax((1, 2))
    for lvl in range(5):
        print(f"means {tag} scale {lvl}: yardstick {float(ref.y[lvl]):.3g} kernel {float(dist[lvl]):.3g}")
    for lvl in range(5):
        assert float(ref.y[lvl]) <= Y_MAX_MEAN[lvl], f"ill-conditioned inputs at scale {lvl}: yardstick {float(ref.y[lvl]):.3g}"
        assert float(dist[lvl]) <= 4 * float(ref.y[lvl]) + MEAN_EPS, (tag, lvl, float(dist[lvl]), float(ref.y[lvl]))


def _check_grad(tag, got, ref, gm):
    """A gradient [N,C,H,W] under 4 x the yardstick + 1e-6 on both measures, the yardstick itself bounded."""
    want, yard = ref.grads(gm)
    err = _grad_errors(got.detach().cpu(), want)
    print(f"gradient {tag}: yardstick max {yard[0]:.3g} L2 {yard[1]:.3g} kernel max {err[0]:.3g} L2 {err[1]:.3g}")
    assert torch.isfinite(got).all()
    for k in range(2):
        assert yard[k] <= Y_MAX_GRAD, f"ill-conditioned gradient ({tag}): yardstick {yard[k]:.3g}"
        assert err[k] <= 4 * yard[k] + 1e-6, (tag, ("max", "L2")[k], err[k], yard[k])


def _render(X):
    return R.to_render_layout(X).to(DEV)


def _apply(ref, V, gm=None):
    """`_MsSsimMeans` on the renderer's layouts: (means, dX as planar [B,3,H,V*W] or None)."""
    from lara_amd.loss import _MsSsimMeans
    x = _render(ref.X).requires_grad_(True)
    means = _MsSsimMeans.apply(x, R.to_target_layout(ref.Y, V).to(DEV))
    if gm is None:
        return means.detach(), None
    means.backward(gm.to(DEV))
    return means.detach(), x.grad.permute(0, 3, 1, 2)


@pytest.mark.parametrize("H,V,W,B,kind", CASES)
def test_means_and_gradient_scale_by_scale(hip_lib, H, V, W, B, kind):
    ref = _reference(H, V, W, B, kind)
    means, dX = _apply(ref, V, ref.gm)
    tag = f"{H}x{V}x{W}"
    if kind == "anti":
        assert float(ref.means64.max()) < -0.5 and float(means.max()) < -0.5      # returned with their sign
    else:
        assert float((ref.means64[0, :, 0] - ref.means64[0, :, 1]).abs().min()) > 1e-3      # a mix-up of the two would show
    _check_means(tag, means, ref)
    _check_grad(tag, dX, ref, ref.gm)


@pytest.mark.parametrize("scale", range(5))
@pytest.mark.parametrize("branch", [0, 1], ids=["ssim", "cs"])
def test_one_path_of_the_backward_at_a_time(hip_lib, scale, branch):
    H, V, W, B = 163, 3, 59, 2
    ref = _reference(H, V, W, B, "ms")
    gm = torch.zeros(5, 3 * B, 2)
    gm[scale, :, branch] = 1.0
    _, dX = _apply(ref, V, gm)
    _check_grad(f"{H}x{V}x{W} scale {scale} {('ssim', 'cs')[branch]}", dX, ref, gm)


def test_zero_upstream_gives_an_exactly_zero_gradient(hip_lib):
    ref = _reference(163, 3, 59, 2, "ms")
    _, dX = _apply(ref, 3, torch.zeros(5, 6, 2))
    assert not dX.any() and torch.isfinite(dX).all()


# ---- through the C interface: the layouts Python never builds ----------------------------------------------------------------
def _view(t, layout, Wv):
    """`lara_image_view` of `t` holding [N,C,H,W'] data as "planar" [N,C,H,W'], "render" [B,H,V*Wv,C] or "target" [B,V,H,Wv,C]."""
    from lara_amd._native import ImageView
    if layout == "planar":
        N, C, H, W = t.shape
        return ImageView(t.data_ptr(), C * H * W, H * W, W, 0, 1, W)
    if layout == "render":
        B, H, VW, C = t.shape
        return ImageView(t.data_ptr(), H * VW * C, 1, VW * C, Wv * C, C, Wv)
    B, V, H, W, C = t.shape
    return ImageView(t.data_ptr(), V * H * W * C, 1, W * C, H * W * C, C, W)


def _to_layout(X, layout, V):
    if layout == "planar":
        return X.contiguous().to(DEV)
    return (R.to_render_layout(X) if layout == "render" else R.to_target_layout(X, V)).to(DEV)


def _to_planar(t, layout):
    return t if layout == "planar" else t.permute(0, 3, 1, 2)


def _c_interface(X, Y, V, x_layout, y_layout, gm, fill=float("nan")):
    """lara_ms_ssim_forward / _backward on X, Y [N,C,H,V*Wv] laid out as asked; dX is pre-filled with `fill`.  -> (means, dX planar)"""
    from lara_amd._native import call, query
    from lara_amd.loss import _window_host
    N, C, H, W = X.shape
    Wv = W // V
    x, y = _to_layout(X, x_layout, V), _to_layout(Y, y_layout, V)
    dx = torch.full_like(x, fill)
    Wx = W if x_layout == "planar" else Wv
    xv, yv, dv = _view(x, x_layout, Wx), _view(y, y_layout, W if y_layout == "planar" else Wv), _view(dx, x_layout, Wx)
    ws = torch.empty(query("lara_ms_ssim_workspace_floats", N, C, H, W), dtype=torch.float32, device=DEV)
    means = torch.empty(5, N * C, 2, dtype=torch.float32, device=DEV)
    call("lara_ms_ssim_forward", torch.device(DEV), N, C, H, W, xv, yv, _window_host(), means, ws)
    call("lara_ms_ssim_backward", torch.device(DEV), N, C, H, W, xv, yv, _window_host(), gm.to(DEV).contiguous(), dv, ws)
    torch.cuda.synchronize()
    return means, _to_planar(dx, x_layout)


@pytest.mark.parametrize("H,V,W,B", [(163, 3, 59, 2), (161, 9, 20, 1)])
def test_every_layout_gives_the_same_bits_and_dx_is_fully_overwritten(hip_lib, H, V, W, B):
    """The same data as planar [N,C,H,W] (sV = 0), as the renderer's [B,H,V*W,3] and with the target as [B,V,H,W,3]: the arithmetic
    per element is the same, so means and dX are equal bit for bit; dX, NaN before the call, holds no NaN after it."""
    ref = _reference(H, V, W, B, "ms")
    runs = [_c_interface(ref.X, ref.Y, V, xl, yl, ref.gm) for xl, yl in (("planar", "planar"), ("render", "render"), ("render", "target"))]
    for means, dX in runs:
        assert not torch.isnan(dX).any() and not torch.isnan(means).any()
    for means, dX in runs[1:]:
        assert torch.equal(means.view(torch.int32), runs[0][0].view(torch.int32))
        assert torch.equal(dX.contiguous().view(torch.int32), runs[0][1].contiguous().view(torch.int32))
    a_means, a_dX = _apply(ref, V, ref.gm)                      # and what the autograd function gives
    assert torch.equal(a_means, runs[2][0]) and torch.equal(a_dX, runs[2][1])
    _check_means(f"{H}x{V}x{W} planar", runs[0][0], ref)
    _check_grad(f"{H}x{V}x{W} planar", runs[0][1], ref, ref.gm)


@pytest.mark.parametrize("N,C", [(2, 1), (1, 4)])
def test_other_channel_counts_planar(hip_lib, N, C):
    H, W = 163, 177
    ref = _reference(H, 1, W, N, "ms", C=C)
    means, dX = _c_interface(ref.X, ref.Y, 1, "planar", "planar", ref.gm)
    _check_means(f"planar N={N} C={C}", means, ref)
    _check_grad(f"planar N={N} C={C}", dX, ref, ref.gm)


# ---- the combination, negative means, repeatability, legal sizes ------------------------------------------------------------
def _fused_value_and_grad(X, Y, V):
    from lara_amd.loss import ms_ssim_fused
    x = _render(X).requires_grad_(True)
    val = ms_ssim_fused(x, R.to_target_layout(Y, V).to(DEV))
    val.backward()
    return val.detach().cpu(), x.grad.permute(0, 3, 1, 2).cpu()


def test_negative_means_clamp_to_an_exact_zero_with_a_zero_gradient(hip_lib):
    """render = 1 - target: every mean is negative, relu takes all of them: exactly 0.0, gradient finite and all zero -- as the
    torch formulation on the CPU gives."""
    from lara_amd.loss import ms_ssim
    H, V, W, B = 177, 2, 97, 1
    ref = _reference(H, V, W, B, "anti")
    val, grad = _fused_value_and_grad(ref.X, ref.Y, V)
    x = ref.X.clone().requires_grad_(True)
    want = ms_ssim(x, ref.Y)
    want.backward()
    assert float(want.detach()) == 0.0 and torch.isfinite(x.grad).all() and not x.grad.any()
    assert float(val) == 0.0 and torch.isfinite(grad).all() and not grad.any()


def test_one_inverted_channel_leaves_the_others_their_value_and_gradient(hip_lib):
    """Channel 0 inverted (its means negative: factor 0, gradient 0), channels 1 and 2 as they are: value and gradient against
    float64, under the bars of this file."""
    from lara_amd.loss import ms_ssim
    H, V, W, B = 177, 2, 97, 1
    X, Y = R.multiscale_images(B, 3, H, V * W, seed=5)
    X[:, 0] = 1.0 - Y[:, 0]
    val, grad = _fused_value_and_grad(X, Y, V)
    outs = []
    for dtype in (torch.float64, torch.float32):
        x = X.to(dtype).requires_grad_(True)
        v = R.combine(R.ms_ssim_means64(x, Y.to(dtype))) if dtype == torch.float64 else ms_ssim(x, Y)
        v.backward()
        outs.append((float(v.detach()), x.grad))
    (want, gwant), (v32, g32) = outs
    yard_v, yard_g = abs(v32 - want), _grad_errors(g32, gwant)
    err_g = _grad_errors(grad, gwant)
    print(f"value: yardstick {yard_v:.3g} kernel {abs(float(val) - want):.3g}; gradient: yardstick {yard_g} kernel {err_g}")
    assert 0.3 < want < 0.67                        # two of three channels contribute
    # (the value moves by sum_l w_l y_l / m_l: with the means' own bounds, (0.87 * 2e-6 + 0.13 * 2.5e-5) / 0.8 = 6e-6 at the most)
    assert yard_v <= 6e-6 and abs(float(val) - want) <= 4 * yard_v + MEAN_EPS
    for k in range(2):
        assert yard_g[k] <= Y_MAX_GRAD and err_g[k] <= 4 * yard_g[k] + 1e-6
    assert not grad[:, 0].any() and not gwant[:, 0].any() and grad[:, 1:].any()


def test_bit_repeatable_and_the_workspace_is_not_consumed(hip_lib):
    from lara_amd.loss import _MsSsimMeans
    H, V, W, B = 163, 3, 59, 2
    ref = _reference(H, V, W, B, "ms")
    a, b = _apply(ref, V, ref.gm), _apply(ref, V, ref.gm)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].contiguous().view(torch.int32), b[1].contiguous().view(torch.int32))
    x = _render(ref.X).requires_grad_(True)
    means = _MsSsimMeans.apply(x, R.to_target_layout(ref.Y, V).to(DEV))
    gm = ref.gm.to(DEV)
    means.backward(gm, retain_graph=True)
    first = x.grad.clone()
    x.grad = None
    means.backward(gm, retain_graph=True)      # the pyramid in the workspace serves a second backward
    assert torch.equal(first.view(torch.int32), x.grad.view(torch.int32))
    assert torch.equal(first.permute(0, 3, 1, 2), a[1])


def test_the_smallest_legal_side_is_161(hip_lib):
    """Host code: no kernel runs."""
    from lara_amd._native import query
    for H, W in ((160, 161), (161, 160), (160, 400)):
        with pytest.raises(ValueError):
            query("lara_ms_ssim_workspace_floats", 1, 3, H, W, error=ValueError("too small"))
    assert query("lara_ms_ssim_workspace_floats", 1, 3, 161, 161) > 0
    assert query("lara_ms_ssim_workspace_floats", 2, 3, 161, 400) > query("lara_ms_ssim_workspace_floats", 1, 3, 161, 400)
