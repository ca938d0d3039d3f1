/*
 * lara_vit.h -- the DINO ViT image encoder of LaRa (lightning/network.py:14-55 `DinoWrapper`: timm `vit_base_patch16_224.dino`
 * with dynamic_img_size, torchvision Normalize, forward_features(...)[:, 1:]) as HIP kernels, forward and backward (part of
 * liblara2dgs.so).  The kernels mirror the model as it runs under bf16 autocast (train_lightning.py:76 `bf16-mixed`).
 *
 * Indices: n < N image; t < T = 1 + hw token of the image (t = 0: the class token, t = 1 + p: patch p = py w + px of the h x w
 * grid, h = H / 16, w = W / 16); c < C channel; heads of width 64.
 *
 *   1. patch rows:  a[n, p, (ch, ky, kx)] = bf16((img[n, ch, 16 py + ky, 16 px + kx] - mean[ch]) / std[ch])   (ImageNet mean / std,
 *                   a true fp32 division as torchvision's Normalize)
 *   2. tokens:      x0[n, 0] = cls + pos[0];  x0[n, 1 + p] = bf16(a[n, p] . bf16(Wpatch)^T + bf16(bpatch)) + pos[1 + p]     fp32
 *   3. per block:   x' = x + bf16(attn(bf16(LN1(x))));  x'' = x' + bf16(fc2(bf16(GELU(bf16(fc1(bf16(LN2(x'))))))))
 *                   every Linear: bf16 operands, fp32 accumulate, bias in fp32, one rounding to bf16;  LayerNorm in fp32;
 *                   attention: softmax(q k^T / 8) v on bf16 q, k, v with fp32 statistics, bf16 P, bf16 output
 *   4. out[n, p] = LN(x_depth[n, 1 + p]; norm)   fp32 [N, hw, C] (the class token dropped); viewed as [N, C, h, w] it is channels-last
 *
 * Parameters (`params`, fp32, device, LARA_VIT_NPARAMS(depth) pointers in this order; timm's names):
 *   0 cls_token [C]   1 pos_embed [T, C] (already resampled to the h x w grid)   2 patch_embed.proj.weight [C, 3 * 16 * 16]
 *   3 patch_embed.proj.bias [C]
 *   4 + 12 i + { 0 norm1.weight [C], 1 norm1.bias, 2 attn.qkv.weight [3C, C], 3 attn.qkv.bias [3C], 4 attn.proj.weight [C, C],
 *                5 attn.proj.bias, 6 norm2.weight, 7 norm2.bias, 8 mlp.fc1.weight [F, C], 9 mlp.fc1.bias [F], 10 mlp.fc2.weight [C, F],
 *                11 mlp.fc2.bias [C] }   of block i < depth
 *   4 + 12 depth + { 0 norm.weight, 1 norm.bias }
 *
 * Images: fp32, image n = (n / views, n % views) of a [N / views, views, 3, H, W] tensor at the element strides img_stride[5]
 * (contiguous NCHW with views = 1, and LaRa's `batch['tar_rgb'][:, :n_views]` slice of [B, V, H, W, 3] with views = n_views, both
 * read in place).  The images take no gradient.
 *
 * lara_vit_forward: `save` = NULL is the inference form (nothing kept).  Otherwise `save` (lara_vit_save_bytes) receives everything
 * lara_vit_backward reads; the output is the same bit for bit.
 *
 * What `save` holds (lara_vit_save_offsets: byte offsets, n = 17, in this order; every region starts 256-byte aligned).  M = N T token
 * rows (row n T + t), Mp = M rounded up to 128, Tp = T rounded up to 64, NP = N hw patch rows, Pp = NP rounded up to 128, NH = N heads:
 *    0 patches    bf16 [Pp, 768]     step 1's rows, element (ch, ky, kx); rows >= NP are zero
 *    1 xfin       fp32 [M, C]        the residual stream behind the last block (what the final LayerNorm reads)
 *    2 stf        fp32 [M, 2]        (mean, rstd) of xfin's rows; the class-token rows (t = 0) are NOT written
 *    3 the first block's base, 4 the block stride: block i's regions start at base + i * stride + the offsets below
 *    5 xin        fp32 [M, C]        the block's input (block 0: the tokens of step 2; block i + 1's xin is block i's output)
 *    6 xn1        bf16 [Mp, C]       bf16(LN1(xin)); rows >= M are zero
 *    7 st1        fp32 [M, 2]        (mean, rstd) of xin's rows
 *    8 q, 9 k, 10 v  bf16 [NH, Tp, 64]  head-major bf16(xn1 . Wqkv^T + bf16(b)); tokens t >= T are zero
 *   11 o          bf16 [Mp, C]       the attention output, heads merged (head h: columns 64 h ..); rows >= M are zero
 *   12 lse        fp32 [NH, Tp]      max + log(sum exp) of every query's scaled scores; entries t >= T are NOT written
 *   13 xmid       fp32 [M, C]        xin + bf16(o . Wproj^T + bf16(b))
 *   14 xn2        bf16 [Mp, C]       bf16(LN2(xmid)); rows >= M are zero
 *   15 st2        fp32 [M, 2]        (mean, rstd) of xmid's rows
 *   16 h          bf16 [Mp, F]       bf16(xn2 . W1^T + bf16(b1)), the GELU's input (its output is recomputed); rows >= M are zero
 * The zero rows are part of the contract: the weight gradients are products over all Mp (Pp) rows.  Host code only; returns 0, or
 * LARA2DGS_E_INVALID for dims the entry points refuse, a null `offsets` or n != 17.
 *
 * lara_vit_backward: `grad` = dL/d(out) fp32 [N, hw, C]; writes (does not accumulate) every parameter gradient, fp32, in `grads`
 * (same order and shapes as `params`; grads[1] is the gradient of the resampled [T, C] table).  Bit-reproducible: no float atomics.
 * Parameter gradients are fixed-order partial sums (lara_gemm_tn_bf16 for the weights); the attention backward runs one wave per
 * 16 keys (dK, dV: a loop over all queries) and one wave per 16 queries (dQ: a loop over all keys), with D = rowsum(dO o O).
 *
 * Limits: C % 64 == 0, 64 <= C <= LARA_VIT_MAX_C, C == 64 heads; F % 64 == 0, 64 <= F <= LARA_VIT_MAX_F; H, W positive multiples of
 * 16; 1 + (H / 16)(W / 16) <= LARA_VIT_MAX_T; 1 <= depth <= 64; N >= 1, views >= 1, N % views == 0; eps > 0.
 * `workspace`: lara_vit_workspace_bytes(d, training) bytes (training = 0: lara_vit_forward with save = NULL; 1: the training forward
 * and lara_vit_backward).  Returns 0 or a negative LARA2DGS_E_* code (arguments are checked before any launch); work is enqueued on
 * `stream`, no host synchronisation.
 */
#ifndef LARA_VIT_H
#define LARA_VIT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LARA_VIT_MAX_C 1024
#define LARA_VIT_MAX_F 4096
#define LARA_VIT_MAX_T 16384
#define LARA_VIT_HEAD_DIM 64
#define LARA_VIT_PATCH 16
#define LARA_VIT_NPARAMS(depth) (6 + 12 * (depth))

typedef struct {
    int32_t N, views, H, W;    /* images (N % views == 0) and their size */
    int32_t C, heads, F;       /* width, heads (C / 64), MLP hidden width */
    int32_t depth;             /* blocks */
    float eps;                 /* every LayerNorm's eps (1e-6 in DINO) */
    int64_t img_stride[5];     /* image element strides of (n / views, n % views, channel, y, x) */
} lara_vit_dims;

int64_t lara_vit_workspace_bytes(const lara_vit_dims *d, int32_t training);
int64_t lara_vit_save_bytes(const lara_vit_dims *d);
int lara_vit_save_offsets(const lara_vit_dims *d, int64_t *offsets, int32_t n);

int lara_vit_forward(const lara_vit_dims *d, const float *images, const float *const *params, float *out, void *save,
                     void *workspace, void *stream);

int lara_vit_backward(const lara_vit_dims *d, const float *const *params, const void *save, const float *grad,
                      float *const *grads, void *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LARA_VIT_H */
