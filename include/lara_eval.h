/*
 * lara_eval.h -- what LaRa's evaluation loop (evaluation.py:54-176) computes per scene behind `Network.forward`, on the device
 * (part of liblara2dgs.so; opt-in, python side: lara_amd/evaluate.py).
 *
 * lara_eval_scores: the scores of B scenes in one call, left in a small device array the caller reads ONCE:
 *
 *     scores[b][ 0] = sum over the strip of (image - target)^2          evaluation.py:84   (PSNR = -10 log10([0] / [1]), :85)
 *     scores[b][ 1] = number of elements of that sum (3 H W)
 *     scores[b][ 2..4] = mean of the single-scale SSIM map of channel 0..2               :87  (the caller averages the three)
 *     scores[b][ 5] = number of masked pixels                                            :98-100
 *     scores[b][ 6] = sum of |depth_pred - depth_gt| over the masked pixels              :107 (tools/depth.py: abs_error)
 *     scores[b][ 7 + k] = number of masked pixels with |depth_pred - depth_gt| < thresholds[k], k < n_thr <= 8   :109-110
 *     scores[b][15] = 0
 *
 * (doubles: counts beyond 2^24 stay exact; LARA_EVAL_ROW per scene.)
 *
 * Images: X (the render, [B, H, V*W, 3]) and Y (batch['tar_rgb'], [B, V, H, W, 3]) are read where they lie through
 * `lara_image_view` (lara_loss.h): value(n, c, y, x) = p[n sN + c sC + y sY + (x / Wv) sV + (x % Wv) sX].  H, W are the sides of
 * the strip that is scored; the "novel views only" crop of evaluation.py:75-78 is a pointer offset of a whole number of views into
 * both views, and the SSIM windows run across the seams of the remaining views as they do in the reference.  X == NULL: no image
 * scores ([0..4] = 0).
 *
 * SSIM is `pytorch_msssim.ssim(X, Y, data_range=1.0, size_average=False)` as published: 11-tap sigma-1.5 Gaussian (`window11`, a
 * HOST pointer), separable, 'valid' (no padding), K = (0.01, 0.03), the mean of the map per (scene, channel).  Sides down to 11
 * (one window) work; a side below 11 returns LARA2DGS_E_INVALID.  `pytorch_msssim` is absent from the reference tree and from the
 * build image (its version is not pinned by the reference): PARITY UNPINNED, as for the MS-SSIM term of lara_loss.h; the kernel is
 * held to a float64 restatement of the published algorithm (tests/eval_restate.py).  The filter runs on x - 1/2 and y - 1/2 and the
 * means, variances and covariance of x, y are recovered exactly (the window's own sum included): the cancellation in
 * E[x^2] - mu^2 loses fewer bits.
 *
 * Depth: over ALL Vd views, never cropped.  depth_pred [B, Hd, Vd*Wd] (a trailing axis of 1 is the same memory), tar_dep and
 * tar_msk [B, Vd, Hd, Wd] read in place; `msk_elem_bytes` is 1 (uint8 / bool) or 4 (float32); a mask value counts as inside when
 * it is nonzero, as `.bool()` does.  The compare is an fp32 compare of the fp32 difference against the threshold rounded to fp32
 * (`thresholds`: HOST pointer to n_thr doubles) -- what numpy does with float32 arrays and a Python float.  Any of the three depth
 * pointers NULL: no depth scores ([5..14] = 0).
 *
 * No float atomics: every sum goes through per-workgroup partials (`workspace`, lara_eval_workspace_doubles doubles) that one
 * small kernel adds in a fixed order, so a call is bit-reproducible and a scene's row does not depend on B.
 *
 * lara_eval_quantize_frames: the float maps of n views -> the uint8 frames a video writer takes (evaluation.py:131-135):
 *
 *     frames[v, y, x, c]        = clamp(rint(image * 255), 0, 255)                                      (np.round: ties to even)
 *     normal_frames[v, y, x, c] = clamp(rint((((normal * alpha + 1 - alpha) + 1) / 2) * 255), 0, 255)
 *
 * the second evaluated as exactly that sequence of fp32 operations (no fused multiply-add).  A pixel (v, y, x) of the inputs
 * lies at pixel offset v pix_sV + y pix_sY + x (times 3 floats for image / rend_normal, 1 for acc_map): the side-by-side maps
 * [H, n*W, .] of `render_views(concat=True)` have pix_sV = W, pix_sY = n W; per-view maps [n, H, W, .] have pix_sV = H W,
 * pix_sY = W.  Outputs are dense [n, H, W, 3]; `frames` (with image) or `normal_frames` (with rend_normal, acc_map) may be NULL.
 *
 * Both return 0 or a negative LARA2DGS_E_* code; work is enqueued on `stream`, no host synchronisation.
 */
#ifndef LARA_EVAL_H
#define LARA_EVAL_H

#include <stdint.h>

#include "lara_loss.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LARA_EVAL_ROW 16
#define LARA_EVAL_MAX_THRESHOLDS 8

int64_t lara_eval_workspace_doubles(int32_t B, int32_t H, int32_t W, int32_t Vd, int32_t Hd, int32_t Wd);

int lara_eval_scores(int32_t B, int32_t H, int32_t W, const lara_image_view *X, const lara_image_view *Y, const float *window11,
                     int32_t Vd, int32_t Hd, int32_t Wd, const float *depth_pred, const float *tar_dep, const void *tar_msk,
                     int32_t msk_elem_bytes, int32_t n_thr, const double *thresholds, double *scores, double *workspace,
                     void *stream);

int lara_eval_quantize_frames(int32_t n, int32_t H, int32_t W, int64_t pix_sV, int64_t pix_sY, const float *image,
                              const float *rend_normal, const float *acc_map, uint8_t *frames, uint8_t *normal_frames,
                              void *stream);

#ifdef __cplusplus
}
#endif
#endif
