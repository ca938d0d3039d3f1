/*
 * lara_loss.h -- the pixel terms of LaRa's training loss as one kernel per direction (part of liblara2dgs.so).
 * The caller directly behind the renderer's outputs ("the callers either side of the path"); opt-in.
 *
 * Replaces the elementwise chains of lightning/loss.py:28-58 (without the MS-SSIM term, :42-45) over the stacked outputs
 * of `Network.forward` ([B, H, V*W, C] maps, network.py:527-529) and the targets `batch['tar_rgb']` [B, V, H, W, 3]
 * (loss.py:24 permutes them into the side-by-side layout: here that is index arithmetic):
 *
 *     terms[0] = mean((image      - tar)^2)                                          loss.py:33-34
 *     terms[1] = mean((image_fine - tar)^2)                                          (the '_fine' round of the same loop)
 *     terms[2] = mean(rend_dist)                                                     loss.py:48
 *     terms[3] = mean((1 - sum_c rend_normal_c * depth_normal_c) * acc_map)          loss.py:52-56 (acc_map detached)
 *
 * (the caller forms loss = t0 + t1 + 1000 t2 + 0.2 t3 and the statistics from the four scalars).  Any of image_fine,
 * rend_dist, and the normal triple (rend_normal, depth_normal, acc_map together) may be NULL: its term is 0.
 * torch runs this as ~25 elementwise / reduction kernels forward and ~30 backward over 8.4 M pixels; here each direction
 * is one pass: forward reads 68 bytes per pixel and leaves per-workgroup partial sums (`partials`,
 * lara_loss_partial_floats(pixels) floats) that a second small kernel adds in a fixed order (reproducible, no atomics);
 * backward reads the same maps and the four upstream gradients g[4] (a device array: no host read) and writes
 * d_image, d_image_fine, d_rend_dist, d_rend_normal, d_depth_normal (any may be NULL = not wanted), fully overwritten.
 * Returns 0 or a negative LARA2DGS_E_* code; work is enqueued on `stream`, no host synchronisation.
 */
#ifndef LARA_LOSS_H
#define LARA_LOSS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int64_t lara_loss_partial_floats(int64_t pixels);

int lara_loss_terms_forward(int32_t B, int32_t V, int32_t H, int32_t W, const float *tar_rgb, const float *image,
                            const float *image_fine, const float *rend_dist, const float *rend_normal,
                            const float *depth_normal, const float *acc_map, float *terms, float *partials, void *stream);

int lara_loss_terms_backward(int32_t B, int32_t V, int32_t H, int32_t W, const float *tar_rgb, const float *image,
                             const float *image_fine, const float *rend_normal, const float *depth_normal,
                             const float *acc_map, const float *g_terms, float *d_image, float *d_image_fine,
                             float *d_rend_dist, float *d_rend_normal, float *d_depth_normal, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * The MS-SSIM term (lightning/loss.py:15, :42-45: `0.5 * (1 - MS_SSIM(data_range=1.0, size_average=True, channel=3)(img, tar))`),
 * forward and backward, on the images where they lie.  `pytorch_msssim` is a third-party dependency absent from /root/reference
 * and from this image (version not pinned by the reference): the algorithm is restated from its published form in
 * lara_amd/loss.py: ms_ssim and, in float64 and scale by scale, in tests/loss_restate.py (five scales, 11-tap sigma-1.5 Gaussian
 * 'valid' filters, K = (0.01, 0.03), 2 x 2 average pooling with odd sides padded) -- PARITY UNPINNED by the reference; the kernels
 * are held to those restatements.
 *
 * An image batch is addressed through a view: value(n, c, y, x) = p[n sN + c sC + y sY + (x / Wv) sV + (x % Wv) sX] (element
 * strides), which covers the renderer's side-by-side output [B, H, V*W, 3] (sN = H V W 3, sC = 1, sY = V W 3, sV = W 3, sX = 3,
 * Wv = W), the targets [B, V, H, W, 3] seen side by side (sN = V H W 3, sC = 1, sY = W 3, sV = H W 3, sX = 3, Wv = W) and
 * planar [N, C, H, W] tensors (sV = 0, Wv = W): no permuted copies.
 *
 * forward : means[5][N*C][2] = per scale and (image, channel) the mean of the SSIM map and of its contrast-structure factor.
 *           MS-SSIM = mean over (n, c) of prod_l relu(m_l)^w_l with m_l = cs mean (l < 4) / ssim mean (l = 4): five numbers per
 *           image and channel, combined by the caller (torch, with autograd).
 * backward: d_means (same shape) -> dX through the view `dX` (fully overwritten; Y is a target and gets no gradient).
 * `workspace` (lara_ms_ssim_workspace_floats floats) carries the pooled pyramid from forward to backward.  `window11`: the 11
 * filter taps (HOST pointer).  Requires min(H, W) > 160.  Work is enqueued on `stream`; no atomics (reproducible). */
typedef struct lara_image_view {
    float *p;
    int64_t sN, sC, sY, sV, sX;
    int32_t Wv;
} lara_image_view;
int64_t lara_ms_ssim_workspace_floats(int32_t N, int32_t C, int32_t H, int32_t W);
int lara_ms_ssim_forward(int32_t N, int32_t C, int32_t H, int32_t W, const lara_image_view *X, const lara_image_view *Y,
                         const float *window11, float *means, float *workspace, void *stream);
int lara_ms_ssim_backward(int32_t N, int32_t C, int32_t H, int32_t W, const lara_image_view *X, const lara_image_view *Y,
                          const float *window11, const float *d_means, const lara_image_view *dX, float *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif
