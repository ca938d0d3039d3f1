"""Float64 restatement of what `lara_amd.evaluate` computes, in numpy, with torch for the filter taps (the project's own text, beside
tests/dino_restate.py): the three scores of evaluation.py:75-111 and the two quantisations of :131-135.

  * PSNR  = -10 log10(mean((x - y)^2))                                                    evaluation.py:84-85
  * SSIM  = `pytorch_msssim.ssim(X, Y, data_range=1.0, size_average=False)` as PUBLISHED: 11-tap sigma-1.5 Gaussian (the package
            builds the taps in float32 and normalises them there; those float32 numbers are used here, in float64 arithmetic),
            separable 'valid' filter of x, y, x^2, y^2, xy, K = (0.01, 0.03); the mean of the map per (image, channel).  The
            package is absent from the reference tree and the build image: parity with it is unpinned.
  * depth = masked count, mean |pred - gt|, fraction with |pred - gt| < t: the difference and the compare in float32 (what
            numpy does with float32 arrays and a Python float, tools/depth.py), the sums in float64.
  * frames: np.round(x * 255) and np.round((((n * a + 1 - a) + 1) / 2) * 255) in float32 -- these ARE float32 expressions
            (ties to even), so the restatement evaluates them in float32.
"""
import math

import numpy as np
import torch


def gauss_taps(size=11, sigma=1.5):
    """The float32 taps `pytorch_msssim._fspecial_gauss_1d` produces (torch float32 operators, normalised in float32), as
    float64 numbers."""
    c = torch.arange(size, dtype=torch.float32) - size // 2
    g = torch.exp(-(c ** 2) / (2 * sigma ** 2))
    return (g / g.sum()).double().numpy()


def _valid_filter(a, w, axis):
    k = len(w)
    n = a.shape[axis] - k + 1
    out = np.zeros(a.shape[:axis] + (n,) + a.shape[axis + 1:], np.float64)
    for i in range(k):
        sl = [slice(None)] * a.ndim
        sl[axis] = slice(i, i + n)
        out += w[i] * a[tuple(sl)]
    return out


def ssim_map(X, Y, data_range=1.0, K=(0.01, 0.03), taps=None):
    """X, Y [..., H, W] -> (ssim map, cs map) [..., H - 10, W - 10], float64."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    w = gauss_taps() if taps is None else np.asarray(taps, np.float64)
    if min(X.shape[-2:]) < len(w):
        raise ValueError("ssim: a side below the window")
    f = lambda a: _valid_filter(_valid_filter(a, w, a.ndim - 2), w, a.ndim - 1)
    C1, C2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    mu1, mu2 = f(X), f(Y)
    s11, s22, s12 = f(X * X) - mu1 * mu1, f(Y * Y) - mu2 * mu2, f(X * Y) - mu1 * mu2
    cs = (2 * s12 + C2) / (s11 + s22 + C2)
    return ((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * cs, cs


def ssim(X, Y, **kw):
    """Mean of the SSIM map per leading index (image, channel)."""
    return ssim_map(X, Y, **kw)[0].mean(axis=(-2, -1))


def strip(tar):
    """batch['tar_rgb'] [B, V, H, W, C] -> the side-by-side strip [B, C, H, V*W] the reference scores (evaluation.py:65)."""
    tar = np.asarray(tar)
    B, V, H, W, C = tar.shape
    return tar.transpose(0, 4, 2, 1, 3).reshape(B, C, H, V * W)


def image_scores(image, tar_rgb, skip_views=0):
    """image [B, H, V*W, 3], tar_rgb [B, V, H, W, 3] -> (psnr [B], ssim [B, 3], mse [B]) of the strip without its first views."""
    W = np.asarray(tar_rgb).shape[3]
    x = np.asarray(image, np.float64).transpose(0, 3, 1, 2)[..., skip_views * W:]
    y = strip(np.asarray(tar_rgb, np.float64))[..., skip_views * W:]
    mse = ((x - y) ** 2).mean(axis=(1, 2, 3))
    return -10.0 * np.log10(mse), ssim(x, y), mse


def depth_scores(depth_pred, tar_dep, tar_msk, thresholds):
    """depth_pred [B, H, V*W(, 1)], tar_dep / tar_msk [B, V, H, W] -> per scene (masked count, sum |d| (float64 sum of the
    float32 differences), [count below t for t in thresholds])."""
    tar_dep, tar_msk = np.asarray(tar_dep, np.float32), np.asarray(tar_msk)
    B, V, H, W = tar_dep.shape
    pred = np.asarray(depth_pred, np.float32).reshape(B, H, V * W)
    gt = tar_dep.transpose(0, 2, 1, 3).reshape(B, H, V * W)
    inside = (tar_msk != 0).transpose(0, 2, 1, 3).reshape(B, H, V * W)
    out = []
    for b in range(B):
        d = np.abs(pred[b][inside[b]] - gt[b][inside[b]])          # float32
        assert d.dtype == np.float32
        out.append((int(inside[b].sum()), float(d.astype(np.float64).sum()), [int((d < np.float32(t)).sum()) for t in thresholds]))
    return out


def depth_acc(count, abs_sum, below):
    """[mean abs error, acc@t1, ...] as evaluation.py:106-110 lists them; NaN for an empty mask (numpy's mean of nothing)."""
    if count == 0:
        return [math.nan] * (1 + len(below))
    return [abs_sum / count] + [k / count for k in below]


def frames(image):
    return np.round(np.asarray(image, np.float32) * np.float32(255)).astype("uint8")


def normal_frames(normal, alpha):
    n, a = np.asarray(normal, np.float32), np.asarray(alpha, np.float32)[..., None]
    one, two = np.float32(1), np.float32(2)
    return np.round((((n * a + one - a) + one) / two) * np.float32(255)).astype("uint8")


def rays(c2w, fovx, fovy, width, height):
    """Pixel-centre rays of a pinhole camera [H, W, 6] (origin, unnormalised direction with unit camera-z), float64:
    focal = side / (2 tan(fov / 2)), principal point at the centre."""
    c2w = np.asarray(c2w, np.float64)
    fx, fy = 0.5 * width / math.tan(0.5 * fovx), 0.5 * height / math.tan(0.5 * fovy)
    xs, ys = np.meshgrid(np.arange(width) + 0.5, np.arange(height) + 0.5)
    d_cam = np.stack([(xs - width / 2) / fx, (ys - height / 2) / fy, np.ones_like(xs)], -1)
    d = d_cam @ c2w[:3, :3].T
    o = np.broadcast_to(c2w[:3, 3], d.shape)
    return np.concatenate([o, d], -1)
