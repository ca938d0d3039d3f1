// meshtexture.hip -- a texture atlas for a mesh, baked from rendered views, on gfx950: the surface point of every texel of the
// closed-form atlas, the blend of the views that see it, and bilinear reads of the result.  The three per-element functions live in
// texatlas.h, one definition for the device and the host; the kernels here and the *_host entries below run them over the texels
// or samples.  Visibility is meshray.hip's walk, called from python between the first two kernels.  Interface, the layout and the
// orders of operations in include/lara_meshtexture.h.
//
//   mt_texels_kernel     one thread per texel: owner, point, anchor
//   mt_bake_kernel       one thread per texel: the views in index order
//   mt_sample_kernel     one thread per (face, barycentrics) pair: four taps
// No LDS, no atomics: two calls give the same bits.  Built with -ffp-contract=off.
#include "common.h"
#include "texatlas.h"
#include "../../include/lara_meshtexture.h"

namespace {

constexpr int64_t MT_MAX_TEXELS = 1ll << 30, MT_MAX_SAMPLES = 1ll << 30;
static_assert(LARA_MESHTEXTURE_MAX_VIEWS == LARA_TEXATLAS_MAX_VIEWS && LARA_MESHTEXTURE_MAX_POWER == LARA_TEXATLAS_MAX_POWER, "one limit");

// the layout, or false for sizes the entries refuse
bool mt_atlas(const int32_t S, const int32_t C, const int32_t T, LaraTexAtlas &L) {
    if (S < LARA_MESHTEXTURE_MIN_PATCH || S > LARA_MESHTEXTURE_MAX_PATCH || C < 1 || T < 0 || (int64_t)C * (S + 1) >= MT_MAX_TEXELS)
        return false;
    L = lara_texatlas_make(S, C, T);
    return L.Wa * L.Ha < MT_MAX_TEXELS;
}

__global__ void __launch_bounds__(256)
mt_texels_kernel(const LaraTexAtlas L, const int32_t Nv, const float *__restrict__ vertices, const int32_t *__restrict__ triangles,
                 int32_t *__restrict__ face, float *__restrict__ point, float *__restrict__ anchor) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= L.Wa * L.Ha) return;
    lara_texatlas_texel(L, Nv, vertices, triangles, i, face, point, anchor);
}

__global__ void __launch_bounds__(256)
mt_bake_kernel(const LaraTexBake B) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B.L.Wa * B.L.Ha) return;
    lara_texatlas_bake_texel(B, i);
}

struct MtBackground { float c[3]; };

__global__ void __launch_bounds__(256)
mt_sample_kernel(const LaraTexAtlas L, const int64_t N, const uint8_t *__restrict__ texture, const int32_t *__restrict__ face,
                 const float *__restrict__ bary, const int32_t channels, const MtBackground bg, float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    lara_texatlas_sample(L, texture, face, bary, channels, bg.c, i, out);
}

// the checked parameters of a bake, or false
bool mt_bake_args(const int32_t S, const int32_t C, const int32_t T, const int32_t Nv, const float *vertices, const int32_t *triangles,
                  const int32_t *face, const float *point, const float *anchor, const int32_t V, const int32_t H, const int32_t W,
                  const float *images, const float *k, const float *w2c, const float *eyes, const int64_t *mask, const float near,
                  const float min_cos, const int32_t power, const int32_t two_sided, const int32_t blend, const float *vertex_colors,
                  const float fill_r, const float fill_g, const float fill_b, uint8_t *texture, float *weight, int32_t *view,
                  LaraTexBake &B) {
    if (!mt_atlas(S, C, T, B.L) || Nv < 0 || V < 0 || V > LARA_MESHTEXTURE_MAX_VIEWS || H < 0 || W < 0 || power < 0 ||
        power > LARA_MESHTEXTURE_MAX_POWER || (blend != LARA_MESHTEXTURE_WEIGHTED && blend != LARA_MESHTEXTURE_BEST) || near != near ||
        min_cos != min_cos || (int64_t)V * H * W >= (1ll << 31))
        return false;
    if (!face || !point || !anchor || !texture || !weight || !view || (T > 0 && (!vertices || !triangles)) ||
        (V > 0 && (!images || !k || !w2c || !eyes)))
        return false;
    B.Nv = Nv; B.V = V; B.H = H; B.W = W; B.power = power; B.two_sided = two_sided ? 1 : 0; B.best = blend == LARA_MESHTEXTURE_BEST;
    B.near = (double)near; B.min_cos = (double)min_cos;
    B.fill[0] = fill_r; B.fill[1] = fill_g; B.fill[2] = fill_b;
    B.vertices = vertices; B.images = images; B.k = k; B.w2c = w2c; B.eyes = eyes; B.vertex_colors = vertex_colors;
    B.point = point; B.anchor = anchor; B.triangles = triangles; B.face = face; B.mask = mask;
    B.texture = texture; B.weight = weight; B.view = view;
    return true;
}

unsigned mt_blocks(const int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

extern "C" {

int lara_meshtexture_atlas_size(int32_t S, int32_t C, int32_t T, int64_t *size) {
    LaraTexAtlas L;
    if (!size || !mt_atlas(S, C, T, L)) return LARA2DGS_E_INVALID;
    size[0] = L.Wa;
    size[1] = L.Ha;
    return LARA2DGS_OK;
}

int lara_meshtexture_texels(int32_t S, int32_t C, int32_t T, int32_t Nv, const float *vertices, const int32_t *triangles, int32_t *face,
                            float *point, float *anchor, void *stream) {
    LaraTexAtlas L;
    if (!mt_atlas(S, C, T, L) || Nv < 0 || !face || !point || !anchor || (T > 0 && (!vertices || !triangles))) return LARA2DGS_E_INVALID;
    L2D_LAUNCH_IN_SCOPE((hipStream_t)stream, mt_texels_kernel, dim3(mt_blocks(L.Wa * L.Ha)), dim3(256), 0, L, Nv, vertices, triangles,
                        face, point, anchor);
    return LARA2DGS_OK;
}

int lara_meshtexture_texels_host(int32_t S, int32_t C, int32_t T, int32_t Nv, const float *vertices, const int32_t *triangles,
                                 int32_t *face, float *point, float *anchor) {
    LaraTexAtlas L;
    if (!mt_atlas(S, C, T, L) || Nv < 0 || !face || !point || !anchor || (T > 0 && (!vertices || !triangles))) return LARA2DGS_E_INVALID;
    for (int64_t i = 0; i < L.Wa * L.Ha; ++i) lara_texatlas_texel(L, Nv, vertices, triangles, i, face, point, anchor);
    return LARA2DGS_OK;
}

int lara_meshtexture_bake(int32_t S, int32_t C, int32_t T, int32_t Nv, const float *vertices, const int32_t *triangles,
                          const int32_t *face, const float *point, const float *anchor, int32_t V, int32_t H, int32_t W,
                          const float *images, const float *k, const float *w2c, const float *eyes, const int64_t *mask, float near,
                          float min_cos, int32_t power, int32_t two_sided, int32_t blend, const float *vertex_colors, float fill_r,
                          float fill_g, float fill_b, uint8_t *texture, float *weight, int32_t *view, void *stream) {
    LaraTexBake B;
    if (!mt_bake_args(S, C, T, Nv, vertices, triangles, face, point, anchor, V, H, W, images, k, w2c, eyes, mask, near, min_cos, power,
                      two_sided, blend, vertex_colors, fill_r, fill_g, fill_b, texture, weight, view, B))
        return LARA2DGS_E_INVALID;
    L2D_LAUNCH_IN_SCOPE((hipStream_t)stream, mt_bake_kernel, dim3(mt_blocks(B.L.Wa * B.L.Ha)), dim3(256), 0, B);
    return LARA2DGS_OK;
}

int lara_meshtexture_bake_host(int32_t S, int32_t C, int32_t T, int32_t Nv, const float *vertices, const int32_t *triangles,
                               const int32_t *face, const float *point, const float *anchor, int32_t V, int32_t H, int32_t W,
                               const float *images, const float *k, const float *w2c, const float *eyes, const int64_t *mask,
                               float near, float min_cos, int32_t power, int32_t two_sided, int32_t blend, const float *vertex_colors,
                               float fill_r, float fill_g, float fill_b, uint8_t *texture, float *weight, int32_t *view) {
    LaraTexBake B;
    if (!mt_bake_args(S, C, T, Nv, vertices, triangles, face, point, anchor, V, H, W, images, k, w2c, eyes, mask, near, min_cos, power,
                      two_sided, blend, vertex_colors, fill_r, fill_g, fill_b, texture, weight, view, B))
        return LARA2DGS_E_INVALID;
    for (int64_t i = 0; i < B.L.Wa * B.L.Ha; ++i) lara_texatlas_bake_texel(B, i);
    return LARA2DGS_OK;
}

int lara_meshtexture_sample(int32_t S, int32_t C, int32_t T, int64_t N, const uint8_t *texture, const int32_t *face, const float *bary,
                            int32_t channels, float bg_r, float bg_g, float bg_b, float *out, void *stream) {
    LaraTexAtlas L;
    if (!mt_atlas(S, C, T, L) || N < 0 || N >= MT_MAX_SAMPLES || (channels != 3 && channels != 4)) return LARA2DGS_E_INVALID;
    if (N == 0) return LARA2DGS_OK;
    if (!texture || !face || !bary || !out) return LARA2DGS_E_INVALID;
    const MtBackground bg = {{bg_r, bg_g, bg_b}};
    L2D_LAUNCH_IN_SCOPE((hipStream_t)stream, mt_sample_kernel, dim3(mt_blocks(N)), dim3(256), 0, L, N, texture, face, bary, channels, bg,
                        out);
    return LARA2DGS_OK;
}

int lara_meshtexture_sample_host(int32_t S, int32_t C, int32_t T, int64_t N, const uint8_t *texture, const int32_t *face,
                                 const float *bary, int32_t channels, float bg_r, float bg_g, float bg_b, float *out) {
    LaraTexAtlas L;
    if (!mt_atlas(S, C, T, L) || N < 0 || N >= MT_MAX_SAMPLES || (channels != 3 && channels != 4)) return LARA2DGS_E_INVALID;
    if (N == 0) return LARA2DGS_OK;
    if (!texture || !face || !bary || !out) return LARA2DGS_E_INVALID;
    const float bg[3] = {bg_r, bg_g, bg_b};
    for (int64_t i = 0; i < N; ++i) lara_texatlas_sample(L, texture, face, bary, channels, bg, i, out);
    return LARA2DGS_OK;
}

}  // extern "C"
