// texatlas.h -- the closed-form texture atlas of include/lara_meshtexture.h and its three per-element functions, one
// definition for the device and the host (meshtexture.hip's kernels, the lara_meshtexture_*_host entries,
// tools/meshtexture_hostcheck.cpp): the owner of a texel, a texel's surface point and anchor, a texel's baked colour over the views,
// and a bilinear read of the atlas at (face, barycentrics).  Integer arithmetic for the layout; double arithmetic on the fp32 inputs
// in the written order, one rounding at the end.  Include it from units built with -ffp-contract=off only.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LARA_TEXATLAS_HD __host__ __device__ __forceinline__
#else
#define LARA_TEXATLAS_HD inline
#endif

#define LARA_TEXATLAS_MAX_VIEWS 64
#define LARA_TEXATLAS_MAX_POWER 8

// ---- the layout -------------------------------------------------------------------------------------------------------------------

// S >= 3 the patch size, C >= 1 the cells per row, T >= 0 the triangles; Wa = C (S + 1), Ha = max(1, ceil(ceil(T / 2) / C)) S
struct LaraTexAtlas { int32_t S, C, T; int64_t Wa, Ha; };

LARA_TEXATLAS_HD LaraTexAtlas lara_texatlas_make(const int32_t S, const int32_t C, const int32_t T) {
    LaraTexAtlas L;
    L.S = S; L.C = C; L.T = T;
    const int64_t cells = ((int64_t)T + 1) / 2, rows = (cells + C - 1) / C;
    L.Wa = (int64_t)C * (S + 1);
    L.Ha = (rows > 1 ? rows : 1) * S;
    return L;
}

// The triangle that owns texel (x, y) of the atlas, or -1 (the odd half of the last cell when T is odd, the cells after it), and the
// texel's local coordinates (a, b): a, b >= 0, a + b <= S - 1.
LARA_TEXATLAS_HD int32_t lara_texatlas_owner(const LaraTexAtlas &L, const int64_t x, const int64_t y, int32_t &a, int32_t &b) {
    const int32_t S = L.S;
    const int64_t cell = (y / S) * L.C + x / (S + 1);
    const int32_t i = (int32_t)(x % (S + 1)), j = (int32_t)(y % S);
    const bool even = i + j <= S - 1;
    a = even ? i : S - i;
    b = even ? j : S - 1 - j;
    const int64_t f = 2 * cell + (even ? 0 : 1);
    return f < L.T ? (int32_t)f : -1;
}

// trimesh.h's rule: every index inside [0, Nv) and every coordinate finite.  p is written only when the triangle is valid.
LARA_TEXATLAS_HD bool lara_texatlas_fetch(const int32_t Nv, const float *vertices, const int32_t *triangles, const int64_t f,
                                          const float *p[3]) {
    for (int k = 0; k < 3; ++k) {
        const int32_t id = triangles[3 * f + k];
        if (id < 0 || id >= Nv) return false;
        p[k] = vertices + 3 * (int64_t)id;
        for (int c = 0; c < 3; ++c)
            if (!(fabsf(p[k][c]) < __builtin_inff())) return false;
    }
    return true;
}

// b0, b1, b2 of local coordinates (a, b) and, in w, the same clamped at 0 and divided by their sum
LARA_TEXATLAS_HD void lara_texatlas_bary(const int32_t S, const int32_t a, const int32_t b, double bary[3], double w[3]) {
    const double d = (double)(S - 2);
    bary[1] = (double)a / d;
    bary[2] = (double)b / d;
    bary[0] = (1.0 - bary[1]) - bary[2];
    const double c0 = bary[0] > 0.0 ? bary[0] : 0.0;
    const double s = (c0 + bary[1]) + bary[2];
    w[0] = c0 / s;
    w[1] = bary[1] / s;
    w[2] = bary[2] / s;
}

// ---- lara_meshtexture_texels ------------------------------------------------------------------------------------------------------

// texel i = y Wa + x: face[i], point[3 i ..], anchor[3 i ..]
LARA_TEXATLAS_HD void lara_texatlas_texel(const LaraTexAtlas &L, const int32_t Nv, const float *vertices, const int32_t *triangles,
                                          const int64_t i, int32_t *face, float *point, float *anchor) {
    int32_t a, b;
    int32_t f = lara_texatlas_owner(L, i % L.Wa, i / L.Wa, a, b);
    const float *p[3];
    if (f >= 0 && !lara_texatlas_fetch(Nv, vertices, triangles, f, p)) f = -1;
    face[i] = f;
    if (f < 0) {
        for (int c = 0; c < 3; ++c) point[3 * i + c] = anchor[3 * i + c] = __builtin_nanf("");
        return;
    }
    double bary[3], w[3];
    lara_texatlas_bary(L.S, a, b, bary, w);
    for (int c = 0; c < 3; ++c) {
        point[3 * i + c] = (float)((bary[0] * (double)p[0][c] + bary[1] * (double)p[1][c]) + bary[2] * (double)p[2][c]);
        anchor[3 * i + c] = (float)((w[0] * (double)p[0][c] + w[1] * (double)p[1][c]) + w[2] * (double)p[2][c]);
    }
}

// ---- lara_meshtexture_bake --------------------------------------------------------------------------------------------------------

struct LaraTexBake {
    LaraTexAtlas L;
    int32_t Nv, V, H, W, power, two_sided, best;
    double near, min_cos;
    float fill[3];
    const float *vertices, *images, *k, *w2c, *eyes, *vertex_colors, *point, *anchor;
    const int32_t *triangles, *face;
    const int64_t *mask;
    uint8_t *texture;
    float *weight;
    int32_t *view;
};

LARA_TEXATLAS_HD uint8_t lara_texatlas_quantize(const double c) {
    const double q = floor(255.0 * c + 0.5);
    return !(q > 0.0) ? 0 : q > 255.0 ? 255 : (uint8_t)q;
}

LARA_TEXATLAS_HD void lara_texatlas_bake_texel(const LaraTexBake &B, const int64_t i) {
    const int32_t f = B.face[i];
    const float *p[3];
    uint8_t *out = B.texture + 4 * i;
    const bool owned = f >= 0 && f < B.L.T && lara_texatlas_fetch(B.Nv, B.vertices, B.triangles, f, p);
    if (!owned) {
        for (int c = 0; c < 3; ++c) out[c] = lara_texatlas_quantize((double)B.fill[c]);
        out[3] = 0;
        B.weight[i] = 0.0f;
        B.view[i] = B.best ? -1 : 0;
        return;
    }
    const double X[3] = {(double)B.point[3 * i], (double)B.point[3 * i + 1], (double)B.point[3 * i + 2]};
    const double A[3] = {(double)B.anchor[3 * i], (double)B.anchor[3 * i + 1], (double)B.anchor[3 * i + 2]};
    double u[3], v[3];
    for (int c = 0; c < 3; ++c) {
        u[c] = (double)p[1][c] - (double)p[0][c];
        v[c] = (double)p[2][c] - (double)p[0][c];
    }
    const double n[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
    const double nl = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    const uint64_t seen = B.mask ? (uint64_t)B.mask[i] : ~(uint64_t)0;
    double sum[3] = {0.0, 0.0, 0.0}, sum_w = 0.0, best_c[3] = {0.0, 0.0, 0.0}, best_w = 0.0;
    int32_t accepted = 0, best = -1;
    for (int32_t e = 0; e < B.V; ++e) {
        if (!((seen >> e) & 1)) continue;
        const float *M = B.w2c + 16 * (int64_t)e, *k = B.k + 4 * (int64_t)e;
        const double xc = (((double)M[0] * X[0] + (double)M[1] * X[1]) + (double)M[2] * X[2]) + (double)M[3];
        const double yc = (((double)M[4] * X[0] + (double)M[5] * X[1]) + (double)M[6] * X[2]) + (double)M[7];
        const double zc = (((double)M[8] * X[0] + (double)M[9] * X[1]) + (double)M[10] * X[2]) + (double)M[11];
        if (!(zc > B.near)) continue;
        const double gx = ((double)k[0] * (xc / zc) + (double)k[2]) - 0.5, gy = ((double)k[1] * (yc / zc) + (double)k[3]) - 0.5;
        if (!(gx >= 0.0 && gx < (double)(B.W - 1) && gy >= 0.0 && gy < (double)(B.H - 1))) continue;
        const float *eye = B.eyes + 3 * (int64_t)e;
        const double d[3] = {(double)eye[0] - A[0], (double)eye[1] - A[1], (double)eye[2] - A[2]};
        const double dl = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
        double cs = ((n[0] * d[0] + n[1] * d[1]) + n[2] * d[2]) / (nl * dl);
        if (B.two_sided) cs = fabs(cs);
        if (!(cs >= B.min_cos)) continue;
        double w = 1.0;
        for (int32_t r = 0; r < B.power; ++r) w = w * cs;
        const double fx = floor(gx), fy = floor(gy), tx = gx - fx, ty = gy - fy;
        const int64_t x0 = (int64_t)fx, y0 = (int64_t)fy;
        const float *I = B.images + 3 * (((int64_t)e * B.H + y0) * B.W + x0);
        const int64_t down = 3 * (int64_t)B.W;
        const double w00 = (1.0 - tx) * (1.0 - ty), w10 = tx * (1.0 - ty), w01 = (1.0 - tx) * ty, w11 = tx * ty;
        double col[3];
        for (int c = 0; c < 3; ++c)
            col[c] = (w00 * (double)I[c] + w10 * (double)I[3 + c]) + (w01 * (double)I[down + c] + w11 * (double)I[down + 3 + c]);
        ++accepted;
        sum_w += w;
        for (int c = 0; c < 3; ++c) sum[c] += w * col[c];
        if (best < 0 || w > best_w) {
            best = e;
            best_w = w;
            for (int c = 0; c < 3; ++c) best_c[c] = col[c];
        }
    }
    const double total = B.best ? best_w : sum_w;
    double col[3];
    const bool coloured = total > 0.0;
    if (coloured) {
        for (int c = 0; c < 3; ++c) col[c] = B.best ? best_c[c] : sum[c] / sum_w;
    } else if (B.vertex_colors) {
        int32_t a, b;
        double bary[3], w[3];
        lara_texatlas_owner(B.L, i % B.L.Wa, i / B.L.Wa, a, b);
        lara_texatlas_bary(B.L.S, a, b, bary, w);
        const float *c0 = B.vertex_colors + 3 * (int64_t)B.triangles[3 * (int64_t)f];
        const float *c1 = B.vertex_colors + 3 * (int64_t)B.triangles[3 * (int64_t)f + 1];
        const float *c2 = B.vertex_colors + 3 * (int64_t)B.triangles[3 * (int64_t)f + 2];
        for (int c = 0; c < 3; ++c) col[c] = (w[0] * (double)c0[c] + w[1] * (double)c1[c]) + w[2] * (double)c2[c];
    } else {
        for (int c = 0; c < 3; ++c) col[c] = (double)B.fill[c];
    }
    for (int c = 0; c < 3; ++c) out[c] = lara_texatlas_quantize(col[c]);
    out[3] = coloured ? 255 : 0;
    B.weight[i] = coloured ? (float)total : 0.0f;
    B.view[i] = B.best ? (coloured ? best : -1) : accepted;
}

// ---- lara_meshtexture_sample ------------------------------------------------------------------------------------------------------

// The four taps of (face, b1, b2): tap[k] = the texel index y Wa + x of (x0, y0), (x1, y0), (x0, y1), (x1, y1), wt[k] its weight.
// The position is clamped into the triangle in texel units first, and x1 = x0 (y1 = y0) where the fraction is zero: every tap is a
// texel the face owns.
LARA_TEXATLAS_HD void lara_texatlas_taps(const LaraTexAtlas &L, const int32_t f, const float b1, const float b2, int64_t tap[4],
                                         double wt[4]) {
    const int32_t S = L.S;
    const double d = (double)(S - 2);
    double a = (double)b1 * d, b = (double)b2 * d;
    a = a > 0.0 ? (a < d ? a : d) : 0.0;
    const double room = d - a;
    b = b > 0.0 ? (b < room ? b : room) : 0.0;
    const int64_t cell = f / 2;
    const double gx = (f & 1) ? (double)S - a : a, gy = (f & 1) ? (double)(S - 1) - b : b;
    const double fx = floor(gx), fy = floor(gy), tx = gx - fx, ty = gy - fy;
    const int64_t x0 = (cell % L.C) * (S + 1) + (int64_t)fx, y0 = (cell / L.C) * S + (int64_t)fy;
    const int64_t x1 = x0 + (tx > 0.0 ? 1 : 0), y1 = y0 + (ty > 0.0 ? 1 : 0);
    tap[0] = y0 * L.Wa + x0; tap[1] = y0 * L.Wa + x1; tap[2] = y1 * L.Wa + x0; tap[3] = y1 * L.Wa + x1;
    wt[0] = (1.0 - tx) * (1.0 - ty); wt[1] = tx * (1.0 - ty); wt[2] = (1.0 - tx) * ty; wt[3] = tx * ty;
}

// out[channels i ..]: channels = 3 (RGB) or 4 (RGB and alpha), each in [0, 1]; face outside [0, T): background, alpha 0
LARA_TEXATLAS_HD void lara_texatlas_sample(const LaraTexAtlas &L, const uint8_t *texture, const int32_t *face, const float *bary,
                                           const int32_t channels, const float background[3], const int64_t i, float *out) {
    const int32_t f = face[i];
    float *o = out + (int64_t)channels * i;
    if (f < 0 || f >= L.T) {
        for (int c = 0; c < channels; ++c) o[c] = c < 3 ? background[c] : 0.0f;
        return;
    }
    int64_t tap[4];
    double wt[4];
    lara_texatlas_taps(L, f, bary[3 * i + 1], bary[3 * i + 2], tap, wt);
    for (int c = 0; c < channels; ++c) {
        const double t0 = (double)texture[4 * tap[0] + c], t1 = (double)texture[4 * tap[1] + c];
        const double t2 = (double)texture[4 * tap[2] + c], t3 = (double)texture[4 * tap[3] + c];
        o[c] = (float)(((wt[0] * t0 + wt[1] * t1) + (wt[2] * t2 + wt[3] * t3)) / 255.0);
    }
}
