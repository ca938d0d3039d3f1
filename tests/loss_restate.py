"""Float64 restatement of what `lara_amd/csrc/loss.hip` and `lara_amd/csrc/msssim.hip` compute (the project's own text, beside
tests/eval_restate.py), sharing no code with `lara_amd/loss.py`:

  * the four pixel terms of lightning/loss.py:28-58 and their five gradients, in numpy, from the formulas of
    include/lara_loss.h; the targets [B,V,H,W,3] reach the maps' side-by-side layout [B,H,V*W,3] by an explicit transpose
    (loss.py:24), not by index arithmetic;
  * the per-scale means of the SSIM map and of its contrast-structure factor, [5, N*C, 2], in torch float64 on the CPU with
    autograd: grouped `conv2d` for the separable 'valid' filter, `avg_pool2d(kernel 2, padding = side % 2)` between scales
    (`pytorch_msssim` as PUBLISHED; the package is absent, parity with it is unpinned).  The 11 taps are the float32 numbers the
    kernels are handed (`lara_amd.loss._window_host()`), widened: an input of the kernels, not part of what is under test;
  * `multiscale_images`: image pairs with structure at every scale of the pyramid, on which sigma^2 = E[x^2] - mu^2 does not
    cancel at the coarse scales (white noise does: its variance shrinks 4x per pooling, and fp32 formulations then disagree with
    float64 by 2e-5 on their own).
"""
import numpy as np
import torch

C1, C2 = 0.01 ** 2, 0.03 ** 2
LEVELS = 5
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


# ---- the pixel terms ---------------------------------------------------------------------------------------------------------
def side_by_side(tar):
    """tar_rgb [B,V,H,W,3] -> [B,H,V*W,3]: the views of a scene next to each other (loss.py:24)."""
    tar = np.asarray(tar)
    B, V, H, W, C = tar.shape
    return np.ascontiguousarray(tar.transpose(0, 2, 1, 3, 4)).reshape(B, H, V * W, C)


def _f64(a):
    return None if a is None else np.asarray(a, np.float64)


def pixel_terms64(tar, image, image_fine, rend_dist, rend_normal, depth_normal, acc):
    """(terms [4], mean |summand| [4]) in float64: mse, mse of the fine image, mean distortion, mean normal error; an absent
    input (None) gives 0 for its term.  A 'summand' is what a pixel (terms 2, 3) or a colour value (terms 0, 1) adds to the sum."""
    tar, image, image_fine, rend_dist, rend_normal, depth_normal, acc = map(
        _f64, (tar, image, image_fine, rend_dist, rend_normal, depth_normal, acc))
    t = side_by_side(tar)
    px = t.shape[:3]
    terms, mags = np.zeros(4), np.zeros(4)
    for q, img in ((0, image), (1, image_fine)):
        if img is not None:
            s = (img - t) ** 2
            terms[q], mags[q] = s.mean(), np.abs(s).mean()
    if rend_dist is not None:
        s = rend_dist.reshape(px)
        terms[2], mags[2] = s.mean(), np.abs(s).mean()
    if rend_normal is not None:
        s = (1.0 - (rend_normal.reshape(px + (3,)) * depth_normal.reshape(px + (3,))).sum(-1)) * acc.reshape(px)
        terms[3], mags[3] = s.mean(), np.abs(s).mean()
    return terms, mags


def pixel_terms_grads64(tar, image, image_fine, rend_dist, rend_normal, depth_normal, acc, g):
    """d(sum_q g[q] terms[q]) / d(image, image_fine, rend_dist, rend_normal, depth_normal) in float64, each in the shape of its
    input (None for an absent one); acc_map is detached (loss.py:55) and the targets get none."""
    tar, image, image_fine, rend_dist, rend_normal, depth_normal, acc, g = map(
        _f64, (tar, image, image_fine, rend_dist, rend_normal, depth_normal, acc, g))
    t = side_by_side(tar)
    px = t.shape[:3]
    n = float(np.prod(px))
    d_image = g[0] * 2.0 * (image - t) / (3.0 * n)
    d_fine = None if image_fine is None else g[1] * 2.0 * (image_fine - t) / (3.0 * n)
    d_dist = None if rend_dist is None else np.full(rend_dist.shape, g[2] / n)
    d_rn = d_dn = None
    if rend_normal is not None:
        w = (-g[3] / n) * acc.reshape(px + (1,))
        d_rn = (w * depth_normal.reshape(px + (3,))).reshape(rend_normal.shape)
        d_dn = (w * rend_normal.reshape(px + (3,))).reshape(depth_normal.shape)
    return d_image, d_fine, d_dist, d_rn, d_dn


# ---- MS-SSIM, scale by scale ------------------------------------------------------------------------------------------------
def taps64():
    """The 11 float32 taps the kernels receive, as a float64 tensor."""
    from lara_amd.loss import _window_host
    return torch.tensor([float(v) for v in _window_host()], dtype=torch.float64)


def _filter(x, w):
    """'valid' separable filter of every plane of x [N,C,H,W]: down the columns, then along the rows, as depthwise convolutions."""
    C = x.shape[1]
    k = w.numel()
    x = torch.nn.functional.conv2d(x, w.view(1, 1, k, 1).expand(C, 1, k, 1), groups=C)
    return torch.nn.functional.conv2d(x, w.view(1, 1, 1, k).expand(C, 1, 1, k), groups=C)


def ms_ssim_maps64(X, Y, taps=None):
    """X, Y [N,C,H,W] (CPU) -> per scale the pair (SSIM map, contrast-structure map) [N,C,H_l - 10,W_l - 10]; differentiable.  In
    the tensors' own dtype (float64 for a reference)."""
    w = (taps64() if taps is None else taps).to(X.dtype)
    maps = []
    for lvl in range(LEVELS):
        mu1, mu2 = _filter(X, w), _filter(Y, w)
        s11 = _filter(X * X, w) - mu1 * mu1
        s22 = _filter(Y * Y, w) - mu2 * mu2
        s12 = _filter(X * Y, w) - mu1 * mu2
        cs = (2 * s12 + C2) / (s11 + s22 + C2)
        maps.append(((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1) * cs, cs))
        if lvl + 1 < LEVELS:
            pad = [X.shape[2] % 2, X.shape[3] % 2]
            X = torch.nn.functional.avg_pool2d(X, kernel_size=2, padding=pad)
            Y = torch.nn.functional.avg_pool2d(Y, kernel_size=2, padding=pad)
    return maps


def ms_ssim_means64(X, Y, taps=None):
    """X, Y [N,C,H,W] (CPU) -> [5, N*C, 2]: per scale and (image, channel) the mean of the SSIM map and of its
    contrast-structure factor; differentiable."""
    NC = X.shape[0] * X.shape[1]
    return torch.stack([torch.stack([ss.mean((-2, -1)).reshape(NC), cs.mean((-2, -1)).reshape(NC)], -1)
                        for ss, cs in ms_ssim_maps64(X, Y, taps)], 0)


def combine(means):
    """MS-SSIM from the means [5, N*C, 2]: cs means of scales 0-3 and the SSIM mean of the last, clamped at zero, raised to the
    published weights, multiplied, averaged over images and channels."""
    vals = torch.cat([means[:4, :, 1], means[4:, :, 0]], 0)
    w = torch.tensor(WEIGHTS, dtype=means.dtype).view(-1, 1)
    return torch.prod(torch.relu(vals) ** w, dim=0).mean()


def ms_ssim_loops64(X, Y, taps):
    """The same value with explicit loops over the taps and a zero-padded reshape for the pooling, in numpy (in the manner of
    tests/test_loss_cpu.py: no convolution, no pooling operator): (means [5, N*C, 2], MS-SSIM)."""
    g = np.asarray(taps, np.float64)
    k = len(g)

    def blur(z):
        a = sum(g[i] * z[i:z.shape[0] - k + 1 + i, :] for i in range(k))
        return sum(g[i] * a[:, i:a.shape[1] - k + 1 + i] for i in range(k))

    def pool(z):
        H, W = z.shape
        zp = np.zeros((H + H % 2 * 2, W + W % 2 * 2))
        zp[H % 2:H % 2 + H, W % 2:W % 2 + W] = z
        Ho, Wo = zp.shape[0] // 2, zp.shape[1] // 2
        return zp[:2 * Ho, :2 * Wo].reshape(Ho, 2, Wo, 2).mean((1, 3))

    N, C = X.shape[:2]
    means = np.zeros((LEVELS, N * C, 2))
    for n in range(N):
        for c in range(C):
            x, y = np.asarray(X[n, c], np.float64), np.asarray(Y[n, c], np.float64)
            for lvl in range(LEVELS):
                mu1, mu2 = blur(x), blur(y)
                cs = (2 * (blur(x * y) - mu1 * mu2) + C2) / ((blur(x * x) - mu1 ** 2) + (blur(y * y) - mu2 ** 2) + C2)
                ss = (2 * mu1 * mu2 + C1) / (mu1 ** 2 + mu2 ** 2 + C1) * cs
                means[lvl, n * C + c] = ss.mean(), cs.mean()
                if lvl + 1 < LEVELS:
                    x, y = pool(x), pool(y)
    vals = np.concatenate([means[:4, :, 1], means[4:, :, 0]], 0)
    return means, (np.maximum(vals, 0.0) ** np.asarray(WEIGHTS)[:, None]).prod(0).mean()


def ms_ssim_means_kernel_order32(X, Y, taps):
    """The means as csrc/msssim.hip rounds them, emulated in numpy: every product and sum in fp32 in the kernels' order (the 11 taps
    along the row, then down the column, each a fused multiply-add onto the running sum; the 2 x 2 pooling as ((a + b) + c) + d
    times 0.25; variances as filtered squares minus squared means), the division correctly rounded, the map summed in float64.
    Not a reference: a way to tell whether a distance between the kernels and float64 is the rounding of this order or a fault."""
    f32 = np.float32
    w = np.asarray(taps, f32)
    c1, c2 = f32(0.01) * f32(0.01), f32(0.03) * f32(0.03)

    def fma(a, b, c):
        return (np.float64(a) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)

    def blur(z):
        H, W = z.shape
        o, a = np.zeros((H, W - 10), f32), np.zeros((H - 10, W - 10), f32)
        for t in range(11):
            o = fma(w[t], z[:, t:t + W - 10], o)
        for t in range(11):
            a = fma(w[t], o[t:t + H - 10, :], a)
        return a

    def pool(z):
        H, W = z.shape
        zp = np.zeros((H + H % 2 * 2, W + W % 2 * 2), f32)
        zp[H % 2:H % 2 + H, W % 2:W % 2 + W] = z
        zp = zp[:zp.shape[0] // 2 * 2, :zp.shape[1] // 2 * 2]
        return f32(0.25) * (((zp[0::2, 0::2] + zp[0::2, 1::2]) + zp[1::2, 0::2]) + zp[1::2, 1::2])

    N, C = X.shape[:2]
    means = np.zeros((LEVELS, N * C, 2))
    for n in range(N):
        for c in range(C):
            x, y = np.asarray(X[n, c], f32), np.asarray(Y[n, c], f32)
            for lvl in range(LEVELS):
                mu1, mu2, xx, yy, xy = blur(x), blur(y), blur(x * x), blur(y * y), blur(x * y)
                m11, m22, m12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
                cs = (f32(2) * (xy - m12) + c2) / ((xx - m11) + (yy - m22) + c2)
                ss = (f32(2) * m12 + c1) / (m11 + m22 + c1) * cs
                assert cs.dtype == ss.dtype == f32
                means[lvl, n * C + c] = ss.astype(np.float64).mean(), cs.astype(np.float64).mean()
                if lvl + 1 < LEVELS:
                    x, y = pool(x), pool(y)
    return means


# ---- well-conditioned inputs -------------------------------------------------------------------------------------------------
def _multiscale_field(N, C, H, W, gen):
    """Mean of nearest-neighbour-upsampled uniform fields at block sizes 1, 2, 4, 8, 16, 32: in [0, 1], variance at every scale."""
    f = torch.zeros(N, C, H, W, dtype=torch.float64)
    blocks = (1, 2, 4, 8, 16, 32)
    for b in blocks:
        h, w = -(-H // b), -(-W // b)
        u = torch.rand(N, C, h, w, generator=gen, dtype=torch.float64)
        f += u.repeat_interleave(b, 2).repeat_interleave(b, 3)[:, :, :H, :W]
    return f / len(blocks)


def multiscale_images(N, C, H, W, seed, kind="ms"):
    """(render X, target Y) [N,C,H,W] float32 on the CPU.  kind "ms": X = clamp(Y + 0.6 (a second field - 0.5), 0, 1) -- the cs
    and SSIM means sit near 0.84 and differ from each other in the third digit; "anti": X = 1 - Y, every mean negative."""
    gen = torch.Generator().manual_seed(seed)
    Y = _multiscale_field(N, C, H, W, gen)
    if kind == "anti":
        return 1.0 - Y.float(), Y.float()
    if kind != "ms":
        raise ValueError(kind)
    X = (Y + 0.6 * (_multiscale_field(N, C, H, W, gen) - 0.5)).clamp(0.0, 1.0)
    return X.float(), Y.float()


def to_render_layout(X):
    """planar [B,3,H,V*W] -> the renderer's [B,H,V*W,3]."""
    return X.permute(0, 2, 3, 1).contiguous()


def to_target_layout(Y, V):
    """planar [B,3,H,V*W] -> batch['tar_rgb'] [B,V,H,W,3]."""
    B, C, H, VW = Y.shape
    return Y.reshape(B, C, H, V, VW // V).permute(0, 3, 2, 4, 1).contiguous()
