// splatpack_ops.h -- the per-row functions of lara_splatpack.h, one definition for the device and the host (splatpack.hip's kernels, the
// *_host entries, tools/splatpack_hostcheck.cpp): a row's validity, its sort keys, the nine values a chunk's bounds are taken over, its
// four packed words, its SH bytes, its 32-byte .splat row, and the reverse of each.  Double arithmetic on the fp32 words, one rounding to
// fp32 per stored fp32, the operation order of the header.  The calls that are not correctly rounded IEEE operations are the double exp
// (alpha, the importance, .splat's scales) and the double log (the decoded logit, .splat's decoded scales).  Include it from units built
// with -ffp-contract=off only.
#pragma once

#include <math.h>
#include <stdint.h>

#include "surfel_ops.h"                          // the five fields and their widths, lara_surfel_finite, lara_surfel_round

#define LARA_SPLATPACK_HD LARA_SURFEL_HD

#define LARA_SPLATPACK_C0 0.28209479177387814
#define LARA_SPLATPACK_ROWS 256                  // rows per chunk
#define LARA_SPLATPACK_RECORD 18                 // fp32 values per chunk record
#define LARA_SPLATPACK_VALUES 9                  // centre xyz, clamped log scales xyz, colour rgb

// offsets into the plan (lara_splatpack.h)
#define LARA_SPLATPACK_S2 0
#define LARA_SPLATPACK_THICKNESS 1

// -0.0 becomes +0.0, every other word keeps its bits: a minimum or maximum over such words does not depend on the order it is taken in
LARA_SPLATPACK_HD float lara_splatpack_canon(const float v) { return v + 0.0f; }

LARA_SPLATPACK_HD float lara_splatpack_clamp_scale(const float s) { return lara_splatpack_canon(s < -20.0f ? -20.0f : s > 20.0f ? 20.0f : s); }

// pack(x, b) = clamp(floor(x (2^b - 1) + 0.5), 0, 2^b - 1); a NaN packs to 0
LARA_SPLATPACK_HD uint32_t lara_splatpack_pack(const double x, const int bits) {
    const double m = (double)((1u << bits) - 1u);
    const double v = floor(x * m + 0.5);
    if (!(v >= 0.0)) return 0u;
    return v > m ? (uint32_t)m : (uint32_t)v;
}

// the position of v between lo and hi; 0 where they coincide
LARA_SPLATPACK_HD double lara_splatpack_unit(const float v, const float lo, const float hi) {
    return hi == lo ? 0.0 : ((double)v - (double)lo) / ((double)hi - (double)lo);
}

// A row is valid when every word of its five fields is finite and its quaternion's squared norm is neither 0 nor non-finite.
LARA_SPLATPACK_HD bool lara_splatpack_row_valid(const int sh_degree, const int64_t s, const float *const *in) {
    bool ok = true;
    for (int f = 0; f < LARA_SURFEL_FIELDS; ++f) {
        const int64_t W = lara_surfel_width(f, sh_degree);
        const float *row = in[f] + s * W;
        for (int64_t r = 0; r < W; ++r) ok = ok && lara_surfel_finite(row[r]);
    }
    const float *q = in[4] + 4 * s;
    const double w = (double)q[0], x = (double)q[1], y = (double)q[2], z = (double)q[3];
    const double n2 = ((w * w + x * x) + y * y) + z * z;
    return ok && n2 > 0.0 && n2 <= 1.7976931348623157e308;
}

// The 30-bit Morton code of a centre inside box = (lo xyz, hi xyz): 10 bits per axis, x the most significant bit of each triple.
LARA_SPLATPACK_HD uint32_t lara_splatpack_morton(const float *center, const float *box) {
    uint32_t code = 0;
    uint32_t q[3];
    for (int a = 0; a < 3; ++a) {
        const float v = lara_splatpack_canon(center[a]), lo = box[a], hi = box[3 + a];
        double t = hi == lo ? 0.0 : floor(((double)v - (double)lo) / ((double)hi - (double)lo) * 1024.0);
        if (!(t >= 0.0)) t = 0.0;
        q[a] = t > 1023.0 ? 1023u : (uint32_t)t;
    }
    for (int b = 9; b >= 0; --b)
        for (int a = 0; a < 3; ++a) code = (code << 1) | ((q[a] >> b) & 1u);
    return code;
}

LARA_SPLATPACK_HD int64_t lara_splatpack_morton_key(const int64_t s, const bool valid, const float *center, const float *box) {
    if (!valid) return ((int64_t)1 << 62) | s;
    return ((int64_t)lara_splatpack_morton(center, box) << 32) | s;
}

LARA_SPLATPACK_HD double lara_splatpack_alpha(const float opacity) { return 1.0 / (1.0 + exp(-(double)opacity)); }

// The importance of a row: fl32(exp(s0 + s1 + s2) alpha); larger sorts first.
LARA_SPLATPACK_HD float lara_splatpack_importance(const double *plan, const float opacity, const float *scale) {
    const double s = ((double)scale[0] + (double)scale[1]) + plan[LARA_SPLATPACK_S2];
    return lara_surfel_round(exp(s) * lara_splatpack_alpha(opacity));
}

LARA_SPLATPACK_HD int64_t lara_splatpack_importance_key(const double *plan, const int64_t s, const bool valid, const float opacity, const float *scale) {
    if (!valid) return ((int64_t)1 << 62) | s;
    const float imp = lara_splatpack_importance(plan, opacity, scale);
    uint32_t w;
    __builtin_memcpy(&w, &imp, sizeof w);
    return ((int64_t)(0x7FFFFFFFu - (w & 0x7FFFFFFFu)) << 31) | s;      // (31: the largest stays below the invalid rows' 1 << 62)
}

// The nine values a chunk's bounds are taken over: the centre, the clamped log scales with s2 as z, k = fl32(0.5 + C0 f_dc).
LARA_SPLATPACK_HD void lara_splatpack_values(const double *plan, const float *center, const float *dc, const float *scale, float *v) {
    for (int a = 0; a < 3; ++a) v[a] = lara_splatpack_canon(center[a]);
    v[3] = lara_splatpack_clamp_scale(scale[0]);
    v[4] = lara_splatpack_clamp_scale(scale[1]);
    v[5] = lara_splatpack_clamp_scale((float)plan[LARA_SPLATPACK_S2]);
    for (int a = 0; a < 3; ++a) v[6 + a] = lara_splatpack_canon(lara_surfel_round(0.5 + LARA_SPLATPACK_C0 * (double)dc[a]));
}

// where value j of lara_splatpack_values has its minimum and its maximum in a chunk record
LARA_SPLATPACK_HD int lara_splatpack_min_slot(const int j) { return 6 * (j / 3) + j % 3; }
LARA_SPLATPACK_HD int lara_splatpack_max_slot(const int j) { return 6 * (j / 3) + 3 + j % 3; }

LARA_SPLATPACK_HD uint32_t lara_splatpack_rotation_word(const float *rot) {
    double q[4];
    for (int i = 0; i < 4; ++i) q[i] = (double)rot[i];
    const double n = __builtin_sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    int L = 0;
    for (int i = 0; i < 4; ++i) q[i] = q[i] / n;
    for (int i = 1; i < 4; ++i)
        if (fabs(q[i]) > fabs(q[L])) L = i;
    const bool flip = q[L] < 0.0;
    uint32_t word = (uint32_t)L;
    for (int i = 0; i < 4; ++i) {
        if (i == L) continue;
        const double c = flip ? -q[i] : q[i];
        word = (word << 10) | lara_splatpack_pack(c * 0.70710678118654752 + 0.5, 10);
    }
    return word;
}

// The four words of a row against its chunk's record: position, rotation, scale, colour (the file's property order).
LARA_SPLATPACK_HD void lara_splatpack_row_words(const float *v, const float *rec, const float opacity, const float *rot, uint32_t *w) {
    uint32_t p[LARA_SPLATPACK_VALUES];
    const int bits[LARA_SPLATPACK_VALUES] = {11, 10, 11, 11, 10, 11, 8, 8, 8};
    for (int j = 0; j < LARA_SPLATPACK_VALUES; ++j)
        p[j] = lara_splatpack_pack(lara_splatpack_unit(v[j], rec[lara_splatpack_min_slot(j)], rec[lara_splatpack_max_slot(j)]), bits[j]);
    w[0] = p[0] << 21 | p[1] << 11 | p[2];
    w[1] = lara_splatpack_rotation_word(rot);
    w[2] = p[3] << 21 | p[4] << 11 | p[5];
    w[3] = p[6] << 24 | p[7] << 16 | p[8] << 8 | lara_splatpack_pack(lara_splatpack_alpha(opacity), 8);
}

// code = clamp(floor((f / 8 + 0.5) 256), 0, 255)
LARA_SPLATPACK_HD uint32_t lara_splatpack_sh_code(const float f) {
    const double v = floor(((double)f / 8.0 + 0.5) * 256.0);
    if (!(v >= 0.0)) return 0u;
    return v > 255.0 ? 255u : (uint32_t)v;
}

// Byte j of a row's SH record: f_rest_j = shs[1 + k][c] with j = c (n - 1) + k.  `shs` is the row's [n][3] words.
LARA_SPLATPACK_HD uint32_t lara_splatpack_sh_byte(const float *shs, const int n, const int j) {
    const int c = j / (n - 1), k = j % (n - 1);
    return lara_splatpack_sh_code(shs[3 * (1 + k) + c]);
}

// ---- the reverse ---------------------------------------------------------------------------------------------------------------------------

LARA_SPLATPACK_HD float lara_splatpack_lerp(const float lo, const float hi, const uint32_t code, const int bits) {
    const double m = (double)((1u << bits) - 1u);
    return lara_surfel_round((double)lo + (double)code / m * ((double)hi - (double)lo));
}

// k -> f_dc, with k between lo and hi
LARA_SPLATPACK_HD float lara_splatpack_dc(const float lo, const float hi, const uint32_t code) {
    const double k = (double)lo + (double)code / 255.0 * ((double)hi - (double)lo);
    return lara_surfel_round((k - 0.5) / LARA_SPLATPACK_C0);
}

// the opacity logit of an 8-bit alpha: never infinite
LARA_SPLATPACK_HD float lara_splatpack_logit(const uint32_t code) {
    double c = (double)code;
    c = c < 0.5 ? 0.5 : c > 254.5 ? 254.5 : c;
    const double a = c / 255.0;
    return lara_surfel_round(log(a / (1.0 - a)));
}

LARA_SPLATPACK_HD void lara_splatpack_unrow(const float *rec, const uint32_t *w, float *center, float *dc, float *opacity, float *scale, float *rot) {
    center[0] = lara_splatpack_lerp(rec[0], rec[3], w[0] >> 21, 11);
    center[1] = lara_splatpack_lerp(rec[1], rec[4], (w[0] >> 11) & 1023u, 10);
    center[2] = lara_splatpack_lerp(rec[2], rec[5], w[0] & 2047u, 11);
    scale[0] = lara_splatpack_lerp(rec[6], rec[9], w[2] >> 21, 11);
    scale[1] = lara_splatpack_lerp(rec[7], rec[10], (w[2] >> 11) & 1023u, 10);
    dc[0] = lara_splatpack_dc(rec[12], rec[15], w[3] >> 24);
    dc[1] = lara_splatpack_dc(rec[13], rec[16], (w[3] >> 16) & 255u);
    dc[2] = lara_splatpack_dc(rec[14], rec[17], (w[3] >> 8) & 255u);
    opacity[0] = lara_splatpack_logit(w[3] & 255u);
    const int L = (int)(w[1] >> 30);
    double sum = 0.0, q[4];
    int shift = 20;
    for (int i = 0; i < 4; ++i) {
        if (i == L) continue;
        q[i] = ((double)((w[1] >> shift) & 1023u) / 1023.0 - 0.5) * 1.4142135623730951;
        sum = sum + q[i] * q[i];
        shift -= 10;
    }
    const double rest = 1.0 - sum;
    q[L] = __builtin_sqrt(rest > 0.0 ? rest : 0.0);
    for (int i = 0; i < 4; ++i) rot[i] = lara_surfel_round(q[i]);
}

// ((code + 0.5) / 256 - 0.5) 8
LARA_SPLATPACK_HD float lara_splatpack_sh_value(const uint32_t code) { return lara_surfel_round((((double)code + 0.5) / 256.0 - 0.5) * 8.0); }

// ---- the 32-byte .splat row as eight words ---------------------------------------------------------------------------------------------------

LARA_SPLATPACK_HD void lara_splatpack_splat_row(const double *plan, const float *center, const float *dc, const float opacity, const float *scale,
                                                const float *rot, uint32_t *w) {
    __builtin_memcpy(w, center, 3 * sizeof(float));
    const float e[3] = {lara_surfel_round(exp((double)scale[0])), lara_surfel_round(exp((double)scale[1])), (float)plan[LARA_SPLATPACK_THICKNESS]};
    __builtin_memcpy(w + 3, e, 3 * sizeof(float));
    uint32_t colour = 0, quat = 0;
    for (int a = 0; a < 3; ++a) {
        const double k = (double)lara_surfel_round(0.5 + LARA_SPLATPACK_C0 * (double)dc[a]);
        colour |= lara_splatpack_pack(k < 0.0 ? 0.0 : k > 1.0 ? 1.0 : k, 8) << (8 * a);
    }
    colour |= lara_splatpack_pack(lara_splatpack_alpha(opacity), 8) << 24;
    double q[4];
    for (int i = 0; i < 4; ++i) q[i] = (double)rot[i];
    const double n = __builtin_sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    for (int i = 0; i < 4; ++i) {
        const double v = floor(q[i] / n * 128.0 + 128.0 + 0.5);
        quat |= (!(v >= 0.0) ? 0u : v > 255.0 ? 255u : (uint32_t)v) << (8 * i);
    }
    w[6] = colour, w[7] = quat;
}

LARA_SPLATPACK_HD void lara_splatpack_splat_unrow(const uint32_t *w, float *center, float *dc, float *opacity, float *scale, float *rot) {
    __builtin_memcpy(center, w, 3 * sizeof(float));
    float e[2];
    __builtin_memcpy(e, w + 3, 2 * sizeof(float));
    scale[0] = lara_surfel_round(log((double)e[0]));
    scale[1] = lara_surfel_round(log((double)e[1]));
    for (int a = 0; a < 3; ++a) dc[a] = lara_surfel_round(((double)((w[6] >> (8 * a)) & 255u) / 255.0 - 0.5) / LARA_SPLATPACK_C0);
    opacity[0] = lara_splatpack_logit(w[6] >> 24);
    for (int i = 0; i < 4; ++i) rot[i] = lara_surfel_round(((double)((w[7] >> (8 * i)) & 255u) - 128.0) / 128.0);
}

// ---- the host entries' loops (lara_splatpack_*_host, tools/splatpack_hostcheck.cpp) ----------------------------------------------------------

inline void lara_splatpack_host_bounds(const int sh_degree, const int64_t P, const float *const *in, uint8_t *valid, float *box, int64_t *dropped) {
    int64_t gone = 0;
    for (int a = 0; a < 3; ++a) box[a] = INFINITY, box[3 + a] = -INFINITY;
    for (int64_t s = 0; s < P; ++s) {
        const bool ok = lara_splatpack_row_valid(sh_degree, s, in);
        valid[s] = ok ? 1 : 0;
        gone += ok ? 0 : 1;
        for (int a = 0; ok && a < 3; ++a) {
            const float v = lara_splatpack_canon(in[0][3 * s + a]);
            box[a] = v < box[a] ? v : box[a];
            box[3 + a] = v > box[3 + a] ? v : box[3 + a];
        }
    }
    *dropped = gone;
}

inline void lara_splatpack_host_morton_keys(const int64_t P, const float *centers, const uint8_t *valid, const float *box, int64_t *keys) {
    for (int64_t s = 0; s < P; ++s) keys[s] = lara_splatpack_morton_key(s, valid[s] != 0, centers + 3 * s, box);
}

inline void lara_splatpack_host_importance_keys(const double *plan, const int64_t P, const float *opacity, const float *scales, const uint8_t *valid,
                                                int64_t *keys) {
    for (int64_t s = 0; s < P; ++s) keys[s] = lara_splatpack_importance_key(plan, s, valid[s] != 0, opacity[s], scales + 2 * s);
}

// A source row outside 0 .. P - 1 takes no part in the bounds and packs to zero words and zero bytes.
inline void lara_splatpack_host_encode(const double *plan, const int sh_degree, const int64_t P, const int64_t P_out, const float *const *in,
                                       const int64_t *order, float *chunks, uint32_t *words, uint8_t *sh) {
    const int n = (sh_degree + 1) * (sh_degree + 1), W = 3 * (n - 1);
    for (int64_t c0 = 0; c0 < P_out; c0 += LARA_SPLATPACK_ROWS) {
        const int64_t rows = P_out - c0 < LARA_SPLATPACK_ROWS ? P_out - c0 : LARA_SPLATPACK_ROWS;
        float *rec = chunks + c0 / LARA_SPLATPACK_ROWS * LARA_SPLATPACK_RECORD;
        for (int j = 0; j < LARA_SPLATPACK_VALUES; ++j) rec[lara_splatpack_min_slot(j)] = INFINITY, rec[lara_splatpack_max_slot(j)] = -INFINITY;
        for (int pass = 0; pass < 2; ++pass)
            for (int64_t i = c0; i < c0 + rows; ++i) {
                const int64_t s = order[i];
                const bool live = s >= 0 && s < P;
                float v[LARA_SPLATPACK_VALUES];
                if (live) lara_splatpack_values(plan, in[0] + 3 * s, in[1] + 3 * n * s, in[3] + 2 * s, v);
                if (pass == 0) {
                    for (int j = 0; live && j < LARA_SPLATPACK_VALUES; ++j) {
                        float *lo = rec + lara_splatpack_min_slot(j), *hi = rec + lara_splatpack_max_slot(j);
                        *lo = v[j] < *lo ? v[j] : *lo;
                        *hi = v[j] > *hi ? v[j] : *hi;
                    }
                    continue;
                }
                uint32_t w[4] = {0u, 0u, 0u, 0u};
                if (live) lara_splatpack_row_words(v, rec, in[2][s], in[4] + 4 * s, w);
                __builtin_memcpy(words + 4 * i, w, sizeof w);
                for (int j = 0; j < W; ++j) sh[i * W + j] = live ? (uint8_t)lara_splatpack_sh_byte(in[1] + 3 * n * s, n, j) : (uint8_t)0;
            }
    }
}

inline void lara_splatpack_host_decode(const int sh_degree, const int64_t P_out, const float *chunks, const uint32_t *words, const uint8_t *sh,
                                       float *const *out) {
    const int n = (sh_degree + 1) * (sh_degree + 1), W = 3 * (n - 1);
    for (int64_t i = 0; i < P_out; ++i) {
        lara_splatpack_unrow(chunks + i / LARA_SPLATPACK_ROWS * LARA_SPLATPACK_RECORD, words + 4 * i, out[0] + 3 * i, out[1] + 3 * n * i, out[2] + i,
                             out[3] + 2 * i, out[4] + 4 * i);
        for (int j = 0; j < W; ++j) out[1][3 * n * i + 3 * (1 + j % (n - 1)) + j / (n - 1)] = lara_splatpack_sh_value(sh[i * W + j]);
    }
}

inline void lara_splatpack_host_splat_encode(const double *plan, const int sh_degree, const int64_t P, const int64_t P_out, const float *const *in,
                                             const int64_t *order, uint32_t *rows) {
    const int n = (sh_degree + 1) * (sh_degree + 1);
    for (int64_t i = 0; i < P_out; ++i) {
        const int64_t s = order[i];
        uint32_t w[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        if (s >= 0 && s < P) lara_splatpack_splat_row(plan, in[0] + 3 * s, in[1] + 3 * n * s, in[2][s], in[3] + 2 * s, in[4] + 4 * s, w);
        __builtin_memcpy(rows + 8 * i, w, sizeof w);
    }
}

inline void lara_splatpack_host_splat_decode(const int64_t P_out, const uint32_t *rows, float *const *out) {
    for (int64_t i = 0; i < P_out; ++i)
        lara_splatpack_splat_unrow(rows + 8 * i, out[0] + 3 * i, out[1] + 3 * i, out[2] + i, out[3] + 2 * i, out[4] + 4 * i);
}
