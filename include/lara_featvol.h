/*
 * lara_featvol.h -- LaRa's image-feature volume (lightning/network.py:352-379 `Network.build_feat_vol` and the view-embedding
 * concatenation :448-452) as HIP kernels, forward and backward (part of liblara2dgs.so).
 *
 * Indices: b < B scene; v < V input view (the first n_views_sel of the batch); t = (y, x) token of the h x w feature map;
 * s = (i R + j) R + k point of the R^3 `volume_grid` (network.py:345-349: grid[s] = ((i, j, k) + 1/2) / R * 2 - 1, times 0.5);
 * c < C image-feature channel; e < E view-embedding channel.
 *
 *   1. ray features per token:  d = rays[3:6] / max(|rays[3:6]|, 1e-12);  m = rays[0:3] x d;  f = [rsh_cart_3(d), rsh_cart_3(m)]  (32)
 *   2. ModLN (network.py:190-213), as it runs under bf16 autocast (train_lightning.py:76):
 *        a     = bf16(SiLU(f))
 *        mod   = bf16(a . bf16(W)^T + bf16(bias))                  W [2C, 32] = dir_norm.mlp[1].weight; mod = [shift | scale]
 *        n     = LayerNorm(x_t; gamma, beta, eps)                  fp32
 *        y_t   = n * bf16(1 + scale) + shift                       fp32 (the 1 + scale of a bf16 tensor stays bf16)
 *   3. projection (network.py:182-187), under autocast too:  p_c = bf16(bf16(p) bf16(R_v)^T) + t_v;  q = bf16(bf16(p_c) bf16(K_v)^T);
 *      (u, u') = bf16(q.xy / q.z)   (the two matmuls run on bf16 operands with bf16 results)
 *   4. grid_sample (bilinear, zero padding, align_corners = False) of y at grid = (u + 1/2) / (img_w, img_h) * 2 - 1 (each step
 *      rounded to bf16: the tensors are bf16), i.e. at feature-map pixel ((g + 1) w - 1) / 2 in fp32: img_w / img_h are the INPUT
 *      IMAGE's size, not the map's
 *   5. out[b, v, c] = sample (c < C),  out[b, v, C + e] = view_embed[v, e]
 *
 * Output layouts (`layout`):
 *   LARA_FEATVOL_VOLUME  (0)  fp32 [B, V, C + E, R, R, R]: network.py:452's feat_vol
 *   LARA_FEATVOL_TOKENS  (1)  bf16 [B R^3, V, C + E]: what lara_batched_transpose(B, V (C + E), R^3, feat_vol, dst_bf16 = 1)
 *                             makes of layout 0 (the volume transformer's cond operand), bit for bit
 *
 * Inputs (device, fp32): img_feats [B V, C, h, w] at the element strides x_stride[4] (contiguous and channels-last both read in
 * place; a channels-last map with 16-byte aligned rows is read with vector loads); rays [B, V, h, w, 6]; w2cs [B, V, 4, 4];
 * ixts [B, V, 3, 3]; grid [R^3, 3]; ln_w, ln_b [C]; mlp_w [2C, 32]; mlp_b [2C]; view_embed [V, E] (NULL when E = 0).
 *
 * Backward: `grad` is dL/d(out) in `grad_layout`, fp32 in both (layout 1's gradient is fp32 [B R^3, V, C + E]).  Writes (does not
 * accumulate) dx (at img_feats' strides), d_ln_w, d_ln_b [C], d_mlp_w [2C, 32], d_mlp_b [2C], d_view_embed [V, E] (sum over b, s;
 * may be NULL).  No gradient to the rays or the cameras.  Bit-reproducible: no float atomics.  The sampling backward is a gather:
 * per view, a texel-keyed list of (point, tap) entries in ascending (point, tap) order is built (integer counts only), and each
 * token sums its entries in list order; the parameter gradients are per-block partial sums added in block order (d_mlp_w:
 * lara_gemm_tn_bf16 over the stored bf16 rows, as autocast's Linear backward forms it).
 *
 * Limits: C % 64 == 0, 64 <= C <= LARA_FEATVOL_MAX_C; 1 <= V <= 8; 0 <= E <= 256, E % 4 == 0; h w <= LARA_FEATVOL_MAX_HW; R >= 1.
 * `workspace`: lara_featvol_workspace_bytes(...) bytes; nothing is kept between calls.  Returns 0 or a negative LARA2DGS_E_* code;
 * work is enqueued on `stream`, no host synchronisation.
 */
#ifndef LARA_FEATVOL_H
#define LARA_FEATVOL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LARA_FEATVOL_VOLUME 0
#define LARA_FEATVOL_TOKENS 1
#define LARA_FEATVOL_MAX_C 1024
#define LARA_FEATVOL_MAX_HW 8192

typedef struct {
    int32_t B, V, C, E, h, w, R;
    int32_t img_w, img_h;      /* input image size (tar_rgb), the grid_sample normalisation */
    float eps;                 /* dir_norm.norm.eps */
    int64_t x_stride[4];       /* img_feats element strides of (B V, C, h, w) */
} lara_featvol_dims;

int64_t lara_featvol_workspace_bytes(const lara_featvol_dims *d);

int lara_featvol_forward(const lara_featvol_dims *d, const float *img_feats, const float *rays, const float *w2cs, const float *ixts,
                         const float *grid, const float *ln_w, const float *ln_b, const float *mlp_w, const float *mlp_b,
                         const float *view_embed, int32_t layout, void *out, void *workspace, void *stream);

int lara_featvol_backward(const lara_featvol_dims *d, const float *img_feats, const float *rays, const float *w2cs, const float *ixts,
                          const float *grid, const float *ln_w, const float *ln_b, const float *mlp_w, const float *mlp_b,
                          const float *grad, int32_t grad_layout, float *dx, float *d_ln_w, float *d_ln_b, float *d_mlp_w,
                          float *d_mlp_b, float *d_view_embed, void *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LARA_FEATVOL_H */
