/*
 * meshtexture/lara_meshtexture.h -- a texture atlas for a mesh, baked from rendered views: every triangle gets the same small patch
 * of a closed-form atlas, every texel the blend of the views that see its surface point, and the atlas is read back bilinearly at
 * (face, barycentrics) (part of liblara2dgs.so; opt-in, python side: lara_amd/meshtexture.py; kernels: csrc/meshtexture.hip; the
 * layout and the three per-element functions: csrc/texatlas.h).  All pointers are device pointers unless a parameter says HOST.
 * Returns 0 or a negative LARA2DGS_E_* code.  Work is enqueued on `stream`; no entry point reads anything back to the host.  One
 * thread per texel or sample, no atomics, no LDS: two calls give the same bits.  Built with -ffp-contract=off: the sequences
 * written here are the instructions, double arithmetic on the fp32 inputs with one rounding at the end.  Every entry has a twin
 * `..._host` without the stream that runs the same function over HOST arrays on the CPU; no device is touched.
 *
 * ---- the layout (S, C, T) --------------------------------------------------------------------------------------------------------------
 * S >= 3 the patch size, C >= 1 the cells per row, T >= 0 the triangles.  Triangles 2c and 2c + 1 share cell c, S + 1 texels wide
 * and S high, at column c % C, row c / C of the atlas:  Wa = C (S + 1),  Ha = max(1, ceil(ceil(T / 2) / C)) S  (T = 0: an S-high
 * atlas without an owner).  lara_meshtexture_atlas_size writes {Wa, Ha} to HOST size[2].  Texel (i, j) of a cell, 0 <= i <= S,
 * 0 <= j < S, belongs to the even triangle when i + j <= S - 1, with local coordinates (a, b) = (i, j); else to the odd one, with
 * (a, b) = (S - i, S - 1 - j): a half-turn, orientation is kept.  Its barycentrics are
 *     b1 = a / (S - 2),   b2 = b / (S - 2),   b0 = (1 - b1) - b2
 * so the corners sit on the texel centres (0, 0), (S - 2, 0), (0, S - 2), and the row a + b = S - 1 is an extrapolated gutter of the
 * same patch.  A bilinear read inside a triangle's UV triangle, corners and edges included, touches only texels the triangle owns:
 * no dilation pass, no bleeding between triangles at mip level 0.  A texel is UNOWNED (face -1) in the odd half of the last cell
 * when T is odd, in the cells after it, and where its triangle is invalid by the rule of the mesh searches (an index outside
 * [0, Nv) or a coordinate that is not finite).
 *
 * ---- lara_meshtexture_texels -----------------------------------------------------------------------------------------------------------
 * vertices [Nv][3] f32, triangles [T][3] i32 -> per texel y Wa + x: face i32, point [3] f32, anchor [3] f32.
 *     point  = (b0 p0 + b1 p1) + b2 p2                                  extrapolated on the gutter
 *     anchor = (w0 p0 + w1 p1) + w2 p2,  w = c / ((c0 + c1) + c2),  c0 = max(b0, 0), c1 = b1, c2 = b2      on the triangle
 * Unowned texels get -1 and NaN.
 *
 * ---- lara_meshtexture_bake -------------------------------------------------------------------------------------------------------------
 * face, point, anchor as lara_meshtexture_texels wrote them; images [V][H][W][3] f32 in [0, 1]; k [V][4] f32 = fx, fy, cx, cy;
 * w2c [V][16] f32 row-major world-to-camera; eyes [V][3] f32 the camera centres; mask [Ha Wa] i64 or NULL (all views): bit e set when
 * view e sees the texel (lara_meshray_visible's output on the anchors); vertex_colors [Nv][3] f32 or NULL.  V <= 64, power in [0, 8],
 * blend LARA_MESHTEXTURE_WEIGHTED or LARA_MESHTEXTURE_BEST, V H W < 2^31.  Per owned texel, over the views e in index order, with
 * X = point, A = anchor, n = (p1 - p0) x (p2 - p0) of the texel's triangle:
 *     skip e when its bit is not set in the mask
 *     x_c = ((M0 X0 + M1 X1) + M2 X2) + M3, y_c and z_c from rows 1 and 2 likewise;   skip unless z_c > near
 *     g_x = (fx (x_c / z_c) + cx) - 0.5,  g_y = (fy (y_c / z_c) + cy) - 0.5           pixel (y, x) is centred at (x + 0.5, y + 0.5)
 *     skip unless 0 <= g_x < W - 1 and 0 <= g_y < H - 1                               all four bilinear taps inside the image
 *     d = eye - A,  cos = ((n0 d0 + n1 d1) + n2 d2) / (|n| |d|),  |v| = sqrt((v0 v0 + v1 v1) + v2 v2);  two_sided: cos = |cos|
 *     skip unless cos >= min_cos                                                      (a triangle without area: cos is NaN)
 *     w = 1, then `power` times w = w cos
 *     t_x = g_x - floor(g_x), t_y likewise;  colour = ((1 - t_x)(1 - t_y) I00 + t_x (1 - t_y) I10) + ((1 - t_x) t_y I01 + t_x t_y I11)
 * WEIGHTED: colour = (sum of w colour) / (sum of w), weight = the sum of w, view = THE NUMBER OF ACCEPTED VIEWS.
 * BEST: the colour, w and index of the view of largest w (a tie: the smaller index) in colour, weight, view.
 * A texel whose weight is not > 0 -- no view accepted -- takes (w0 c0 + w1 c1) + w2 c2 of its triangle's vertex_colors (the anchor's
 * weights) when they are given, else fill; its alpha is 0, its weight 0, its view 0 (WEIGHTED) or -1 (BEST).  Every other owned texel has
 * alpha 255.  An unowned texel gets fill, alpha 0, weight 0, view 0 or -1.
 * -> texture [Ha][Wa][4] u8, each channel floor(255 c + 0.5) clamped to [0, 255] (NaN: 0); weight [Ha][Wa] f32; view [Ha][Wa] i32.
 *
 * ---- lara_meshtexture_sample -----------------------------------------------------------------------------------------------------------
 * texture as baked, face [N] i32, bary [N][3] f32 (b1 and b2 are read), channels 3 (RGB) or 4 (RGB, alpha) -> out [N][channels] f32 in
 * [0, 1].  face outside [0, T): the background, alpha 0.  Else, with d = S - 2:
 *     a = min(max(b1 d, 0), d),   b = min(max(b2 d, 0), d - a)                        clamped into the triangle, in texel units
 *     (g_x, g_y) = (a, b) for an even face, (S - a, S - 1 - b) for an odd one;  x0 = floor(g_x), t_x = g_x - x0,  y likewise
 *     x1 = x0 + 1 when t_x > 0, else x0;   y1 likewise                                a tap of weight 0 is not a foreign texel
 *     out = (((1 - t_x)(1 - t_y) T00 + t_x (1 - t_y) T10) + ((1 - t_x) t_y T01 + t_x t_y T11)) / 255,  Tij the byte at (xi, yj)
 *
 * Limits: 3 <= S <= 4096, Wa Ha < 2^30, N < 2^30.  N == 0 is a no-op for sample.
 */
#ifndef LARA_MESHTEXTURE_H
#define LARA_MESHTEXTURE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LARA_MESHTEXTURE_MIN_PATCH 3
#define LARA_MESHTEXTURE_MAX_PATCH 4096
#define LARA_MESHTEXTURE_MAX_VIEWS 64
#define LARA_MESHTEXTURE_MAX_POWER 8
#define LARA_MESHTEXTURE_WEIGHTED 0
#define LARA_MESHTEXTURE_BEST 1

int lara_meshtexture_atlas_size(int32_t S, int32_t C, int32_t T, int64_t *size);

int lara_meshtexture_texels(int32_t S, int32_t C, int32_t T, int32_t Nv, const float *vertices, const int32_t *triangles, int32_t *face,
                            float *point, float *anchor, void *stream);

int lara_meshtexture_texels_host(int32_t S, int32_t C, int32_t T, int32_t Nv, const float *vertices, const int32_t *triangles,
                                 int32_t *face, float *point, float *anchor);

int lara_meshtexture_bake(int32_t S, int32_t C, int32_t T, int32_t Nv, const float *vertices, const int32_t *triangles,
                          const int32_t *face, const float *point, const float *anchor, int32_t V, int32_t H, int32_t W,
                          const float *images, const float *k, const float *w2c, const float *eyes, const int64_t *mask, float near,
                          float min_cos, int32_t power, int32_t two_sided, int32_t blend, const float *vertex_colors, float fill_r,
                          float fill_g, float fill_b, uint8_t *texture, float *weight, int32_t *view, void *stream);

int lara_meshtexture_bake_host(int32_t S, int32_t C, int32_t T, int32_t Nv, const float *vertices, const int32_t *triangles,
                               const int32_t *face, const float *point, const float *anchor, int32_t V, int32_t H, int32_t W,
                               const float *images, const float *k, const float *w2c, const float *eyes, const int64_t *mask,
                               float near, float min_cos, int32_t power, int32_t two_sided, int32_t blend, const float *vertex_colors,
                               float fill_r, float fill_g, float fill_b, uint8_t *texture, float *weight, int32_t *view);

int lara_meshtexture_sample(int32_t S, int32_t C, int32_t T, int64_t N, const uint8_t *texture, const int32_t *face, const float *bary,
                            int32_t channels, float bg_r, float bg_g, float bg_b, float *out, void *stream);

int lara_meshtexture_sample_host(int32_t S, int32_t C, int32_t T, int64_t N, const uint8_t *texture, const int32_t *face,
                                 const float *bary, int32_t channels, float bg_r, float bg_g, float bg_b, float *out);

#ifdef __cplusplus
}
#endif
#endif
