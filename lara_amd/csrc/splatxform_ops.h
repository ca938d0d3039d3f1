// splatxform_ops.h -- the per-surfel function of lara_splatxform.h, one definition for the device and the host
// (splatxform.hip's kernel, lara_splatxform_apply_host, tools/splatxform_hostcheck.cpp): one surfel's centre, SH coefficients, scales
// and quaternion under the plan of a similarity.  Double arithmetic on the fp32 inputs, one rounding to fp32 per output, the
// operation order of the header; a NaN is stored as one canonical word.  Every group of outputs is written after all of its inputs
// have been read, so each output pointer may be its input pointer (the kernel's rows in LDS).  Include it from units built with
// -ffp-contract=off only.
#pragma once

#include <stdint.h>

#include "surfel_ops.h"                          // lara_surfel_round: fl32 of the header, the one rounding; a NaN becomes 0x7FC00000

#define LARA_SPLATXFORM_HD LARA_SURFEL_HD

// offsets into the plan (lara_splatxform.h)
#define LARA_SPLATXFORM_A 0
#define LARA_SPLATXFORM_T 9
#define LARA_SPLATXFORM_R 12
#define LARA_SPLATXFORM_LOGS 16
#define LARA_SPLATXFORM_D1 17
#define LARA_SPLATXFORM_D2 26
#define LARA_SPLATXFORM_D3 51

LARA_SPLATXFORM_HD void lara_splatxform_copy_word(const float *src, float *dst) {
    if (dst != src) __builtin_memcpy(dst, src, sizeof(float));
}

// band l = L of one surfel: rows [L^2, L^2 + 2L] of sh [n][3], the three channels one after the other
template <int L>
LARA_SPLATXFORM_HD void lara_splatxform_band(const double *D, const float *sh, float *out) {
    constexpr int W = 2 * L + 1;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        double c[W];
#pragma unroll
        for (int j = 0; j < W; ++j) c[j] = (double)sh[3 * (L * L + j) + ch];
#pragma unroll
        for (int i = 0; i < W; ++i) {
            double acc = D[W * i] * c[0];
#pragma unroll
            for (int j = 1; j < W; ++j) acc = acc + D[W * i + j] * c[j];
            out[3 * (L * L + i) + ch] = lara_surfel_round(acc);
        }
    }
}

// One surfel.  DEG is its SH degree: sh and out_sh are [(DEG + 1)^2][3].
template <int DEG>
LARA_SPLATXFORM_HD void lara_splatxform_surfel(const double *plan, const float *center, const float *sh, const float *opacity,
                                               const float *scale, const float *rot, float *out_center, float *out_sh,
                                               float *out_opacity, float *out_scale, float *out_rot) {
    {
        const double *A = plan + LARA_SPLATXFORM_A, *t = plan + LARA_SPLATXFORM_T;
        const double x = (double)center[0], y = (double)center[1], z = (double)center[2];
#pragma unroll
        for (int i = 0; i < 3; ++i) out_center[i] = lara_surfel_round(((A[3 * i] * x + A[3 * i + 1] * y) + A[3 * i + 2] * z) + t[i]);
    }
    {
        const double *r = plan + LARA_SPLATXFORM_R;
        const double w = (double)rot[0], x = (double)rot[1], y = (double)rot[2], z = (double)rot[3];
        out_rot[0] = lara_surfel_round(((r[0] * w - r[1] * x) - r[2] * y) - r[3] * z);
        out_rot[1] = lara_surfel_round(((r[0] * x + r[1] * w) + r[2] * z) - r[3] * y);
        out_rot[2] = lara_surfel_round(((r[0] * y - r[1] * z) + r[2] * w) + r[3] * x);
        out_rot[3] = lara_surfel_round(((r[0] * z + r[1] * y) - r[2] * x) + r[3] * w);
    }
    {
        const double log_s = plan[LARA_SPLATXFORM_LOGS];
        const double a = (double)scale[0], b = (double)scale[1];
        out_scale[0] = lara_surfel_round(a + log_s);
        out_scale[1] = lara_surfel_round(b + log_s);
    }
    lara_splatxform_copy_word(opacity, out_opacity);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) lara_splatxform_copy_word(sh + ch, out_sh + ch);
    if (DEG >= 1) lara_splatxform_band<1>(plan + LARA_SPLATXFORM_D1, sh, out_sh);
    if (DEG >= 2) lara_splatxform_band<2>(plan + LARA_SPLATXFORM_D2, sh, out_sh);
    if (DEG >= 3) lara_splatxform_band<3>(plan + LARA_SPLATXFORM_D3, sh, out_sh);
}

// The host entry's loop (lara_splatxform_apply_host, tools/splatxform_hostcheck.cpp): rows 0 .. P - 1 in order, row p written to row
// out_row0 + p of the outputs.  sh_degree is 0..3 (the caller has checked it).
template <int DEG>
inline void lara_splatxform_host_rows_of(const double *plan, const int64_t P, const float *centers, const float *shs, const float *opacity,
                                         const float *scales, const float *rotations, float *out_centers, float *out_shs,
                                         float *out_opacity, float *out_scales, float *out_rotations, const int64_t out_row0) {
    constexpr int64_t WS = 3 * (DEG + 1) * (DEG + 1);
    for (int64_t p = 0; p < P; ++p) {
        const int64_t o = out_row0 + p;
        lara_splatxform_surfel<DEG>(plan, centers + 3 * p, shs + WS * p, opacity + p, scales + 2 * p, rotations + 4 * p, out_centers + 3 * o,
                                    out_shs + WS * o, out_opacity + o, out_scales + 2 * o, out_rotations + 4 * o);
    }
}

inline void lara_splatxform_host_rows(const double *plan, const int sh_degree, const int64_t P, const float *centers, const float *shs,
                                      const float *opacity, const float *scales, const float *rotations, float *out_centers,
                                      float *out_shs, float *out_opacity, float *out_scales, float *out_rotations, const int64_t out_row0) {
#define LARA_SPLATXFORM_GO(DEG)                                                                                                    \
    lara_splatxform_host_rows_of<DEG>(plan, P, centers, shs, opacity, scales, rotations, out_centers, out_shs, out_opacity, out_scales, \
                                      out_rotations, out_row0)
    switch (sh_degree) {
    case 0: LARA_SPLATXFORM_GO(0); break;
    case 1: LARA_SPLATXFORM_GO(1); break;
    case 2: LARA_SPLATXFORM_GO(2); break;
    default: LARA_SPLATXFORM_GO(3); break;
    }
#undef LARA_SPLATXFORM_GO
}
