// batchfinish_ops.h -- the per-pixel function of lara_batchfinish.h, one definition for the device and the host
// (batchfinish.hip's kernel, lara_batch_finish_host, tools/batchfinish_hostcheck.cpp): one stored pixel -- four uint8 of RGBA and,
// optionally, three uint8 of a normal -- finished into the fp32 colour over the view's background, the uint8 mask and the rotated
// fp32 normal.  fp32 throughout, every operation rounded, the order of the header.  Include it from units built with
// -ffp-contract=off only: the two fmaf below are the only fused operations, and they are written out.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define LARA_BATCHFINISH_HD __host__ __device__ __forceinline__
#else
#define LARA_BATCHFINISH_HD inline
#endif

// (float)u / 255.0f, correctly rounded, without the division: q = fl(u r) with r = fl(1 / 255) is within an ulp of the quotient, the
// residual e = u - 255 q is exact in one fma, and fl(q + e r) is the correctly rounded quotient (Markstein's correction step; r is
// the correctly rounded reciprocal).  There are 256 arguments: tests/test_batchfinish.py holds every one to numpy's division.
LARA_BATCHFINISH_HD float lara_batchfinish_unit(const uint8_t u) {
    const float x = (float)u, r = 1.0f / 255.0f;
    const float q = x * r;
    const float e = __builtin_fmaf(-q, 255.0f, x);
    return __builtin_fmaf(e, r, q);
}

// The colour and the mask of one pixel.  rgba: its 4 stored bytes; bg: the 3 floats of its view's background; rgb: 3 floats out.
LARA_BATCHFINISH_HD void lara_batchfinish_colour(const uint8_t *rgba, const float *bg, float *rgb, uint8_t *msk) {
    const float a = lara_batchfinish_unit(rgba[3]);
    const float rest = 1.0f - a;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float front = lara_batchfinish_unit(rgba[c]) * a;
        const float back = bg[c] * rest;
        rgb[c] = front + back;
    }
    *msk = rgba[3] > 0 ? 1 : 0;
}

// The normal of one pixel.  n_u8: its 3 stored bytes; R: the scene's 3x3, row-major; nrm: 3 floats out.
LARA_BATCHFINISH_HD void lara_batchfinish_normal(const uint8_t *n_u8, const float *R, float *nrm) {
    float n[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) n[k] = lara_batchfinish_unit(n_u8[k]) * 2.0f - 1.0f;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float p0 = n[0] * R[3 * j], p1 = n[1] * R[3 * j + 1], p2 = n[2] * R[3 * j + 2];
        nrm[j] = (p0 + p1) + p2;
    }
}

// One pixel: its colour and mask and, where n_u8 is not null, its normal (n_u8, R and nrm go together).  The kernel's wide paths call
// the two halves on the pixels of a 16-byte load; everything else calls this.
LARA_BATCHFINISH_HD void lara_batchfinish_pixel(const uint8_t *rgba, const float *bg, const uint8_t *n_u8, const float *R, float *rgb,
                                                uint8_t *msk, float *nrm) {
    lara_batchfinish_colour(rgba, bg, rgb, msk);
    if (n_u8) lara_batchfinish_normal(n_u8, R, nrm);
}

// where the normal of pixel (b, v, h, w) lies in tar_nrm [B][H][V W][3]: the (1, 0, 2, 3) transpose of the views, folded into the address
LARA_BATCHFINISH_HD int64_t lara_batchfinish_nrm_at(const int64_t b, const int64_t v, const int64_t h, const int64_t w, const int64_t V,
                                                    const int64_t H, const int64_t W) {
    return (((b * H + h) * V + v) * W + w) * 3;
}

// The host entry's loop (lara_batch_finish_host, tools/batchfinish_hostcheck.cpp): every pixel in the order of the flat index.
inline void lara_batchfinish_host_pixels(const uint8_t *rgba, const float *bg, const uint8_t *n_u8, const float *rot, const int64_t B,
                                         const int64_t V, const int64_t H, const int64_t W, float *out_rgb, uint8_t *out_msk,
                                         float *out_nrm) {
    int64_t p = 0;
    for (int64_t b = 0; b < B; ++b)
        for (int64_t v = 0; v < V; ++v)
            for (int64_t h = 0; h < H; ++h)
                for (int64_t w = 0; w < W; ++w, ++p)
                    lara_batchfinish_pixel(rgba + 4 * p, bg + 3 * (b * V + v), n_u8 ? n_u8 + 3 * p : nullptr, n_u8 ? rot + 9 * b : nullptr,
                                           out_rgb + 3 * p, out_msk + p, n_u8 ? out_nrm + lara_batchfinish_nrm_at(b, v, h, w, V, H, W) : nullptr);
}
