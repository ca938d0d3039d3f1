/*
 * lara_lpips.h -- LPIPS (Zhang et al. 2018, "The Unreasonable Effectiveness of Deep Features as a Perceptual Metric"), forward
 * only, for the VGG-16 and AlexNet variants that LaRa's evaluation reports (evaluation.py:48-49, :89-90), on the device (part of
 * liblara2dgs.so; opt-in, python side: lara_amd/lpips.py).  Written from the published method; PARITY with the `lpips` package is
 * UNPINNED (the package and torchvision are absent from the build image): the kernels are held to a float64 restatement
 * (tests/lpips_restate.py).
 *
 * A network is a list of convolutions (each with bias and ReLU, optionally behind a floor-mode max pool, optionally a tap) and
 * five 1x1 "lin" weight vectors, one per tap:
 *
 *     t      = in_mul * x + in_add                       (2 x - 1 of a [0, 1] image, or x as it is)
 *     u      = (t - shift[c]) / scale[c]                 zero padding of the first convolution applies to u
 *     f_k    = the k-th tap (after the ReLU), NHWC
 *     d_k    = mean over pixels of sum_c lin_k[c] (f0 / (|f0| + 1e-10) - f1 / (|f1| + 1e-10))^2,   |f| = sqrt(sum_c f^2)
 *     scores[b] = { d_0, d_1, d_2, d_3, d_4, d_0 + d_1 + d_2 + d_3 + d_4 (in that order), 0, 0 }     LARA_LPIPS_ROW doubles
 *
 * Activations are fp32 NHWC, weights [Cout][kh][kw][Cin] (repacked once by the caller).  Convolutions with Cin % 32 == 0 and
 * Cout % 64 == 0 are an implicit GEMM on the exact-fp32 matrix instruction (M = pixels, N = Cout, K = kh kw Cin; every output is
 * one k-ordered chain of fp32 fused multiply-adds, whatever tile it falls into); the first layer (Cin = 3) is a vector kernel that
 * reads the images where they lie through `lara_image_view` (lara_loss.h) and applies the input scaling on the way.
 *
 * Render X and target Y go through every launch together as a batch of 2 B images (X first).  No float atomics: the pixel sums are
 * double, per thread -> wave -> workgroup partials that one kernel adds in a fixed order; a call is bit-reproducible and a scene's
 * row does not depend on B.  The library keeps no state: `workspace` (lara_lpips_workspace_bytes, 256-byte aligned) holds two
 * activation buffers and the partials.
 *
 * lara_lpips_conv2d / lara_lpips_maxpool are the building blocks on dense NHWC tensors (what the tests hold against torch).
 * All return 0 or a negative LARA2DGS_E_* code; work is enqueued on `stream`, no host synchronisation.
 */
#ifndef LARA_LPIPS_H
#define LARA_LPIPS_H

#include <stdint.h>

#include "lara_loss.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LARA_LPIPS_ROW 8
#define LARA_LPIPS_TAPS 5
#define LARA_LPIPS_MAX_LAYERS 16

typedef struct lara_lpips_layer {
    const float *w;           /* [cout][k][k][cin] */
    const float *bias;        /* [cout] */
    int32_t cin, cout, k, stride, pad;
    int32_t pool_k, pool_s;   /* max pool in FRONT of this convolution (floor mode); pool_k = 0: none */
    int32_t tap;              /* nonzero: the output (after the ReLU) is the next tap */
} lara_lpips_layer;

typedef struct lara_lpips_net {
    int32_t n_layers;
    lara_lpips_layer layers[LARA_LPIPS_MAX_LAYERS];
    const float *lin[LARA_LPIPS_TAPS];   /* [channels of tap k] */
    float shift[3], scale[3];
} lara_lpips_net;

/* negative: the sizes are invalid (an image too small for the net's pools included) */
int64_t lara_lpips_workspace_bytes(const lara_lpips_net *net, int32_t B, int32_t H, int32_t W);

int lara_lpips_forward(const lara_lpips_net *net, int32_t B, int32_t H, int32_t W, const lara_image_view *X,
                       const lara_image_view *Y, float in_mul, float in_add, double *scores, void *workspace, void *stream);

/* y[N, Ho, Wo, Cout] = (relu)(conv(x[N, H, W, Cin], w) + bias); Cin == 3 (vector kernel) or Cin % 32 == 0, Cout % 64 == 0 */
int lara_lpips_conv2d(int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t k, int32_t stride, int32_t pad,
                      int32_t relu, const float *x, const float *w, const float *bias, float *y, void *stream);

/* y[N, (H - k) / s + 1, (W - k) / s + 1, C] = max over the window; C % 4 == 0 */
int lara_lpips_maxpool(int32_t N, int32_t H, int32_t W, int32_t C, int32_t k, int32_t s, const float *x, float *y, void *stream);

#ifdef __cplusplus
}
#endif
#endif
