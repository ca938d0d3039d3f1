// splatdensify_ops.h -- the per-row functions of lara_splatdensify.h, one definition for the device and the host (splatdensify.hip's
// kernels, the *_host entries, tools/splatdensify_hostcheck.cpp): one surfel's statistics, one surfel's action, one surfel's output
// rows, one output word.  Double arithmetic on the fp32 words, one rounding to fp32 per store, the operation order of the header; the
// only call that is not a correctly rounded IEEE operation is the double exp of a split child's centre.  Include it from units built
// with -ffp-contract=off only.
#pragma once

#include <math.h>
#include <stdint.h>

#include "surfel_ops.h"                          // the five fields and their widths, lara_surfel_finite, lara_surfel_round

#define LARA_SPLATDENSIFY_HD LARA_SURFEL_HD

// offsets into the plan (lara_splatdensify.h)
#define LARA_SPLATDENSIFY_GRAD 0
#define LARA_SPLATDENSIFY_LOG_DENSE 1
#define LARA_SPLATDENSIFY_LOGIT_MIN 2
#define LARA_SPLATDENSIFY_MAX_SCREEN 3
#define LARA_SPLATDENSIFY_LOG_WORLD 4
#define LARA_SPLATDENSIFY_LOG_SHRINK 5
#define LARA_SPLATDENSIFY_N 6
#define LARA_SPLATDENSIFY_FLAGS 7

#define LARA_SPLATDENSIFY_ALLOW_CLONE 1
#define LARA_SPLATDENSIFY_ALLOW_SPLIT 2
#define LARA_SPLATDENSIFY_ALLOW_PRUNE 4

#define LARA_SPLATDENSIFY_KEEP 0
#define LARA_SPLATDENSIFY_CLONE 1
#define LARA_SPLATDENSIFY_SPLIT 2
#define LARA_SPLATDENSIFY_PRUNE 3
#define LARA_SPLATDENSIFY_NO_CHILD 255

// The children per split of a plan, clamped to 1..8 (the entries refuse a plan outside it).
LARA_SPLATDENSIFY_HD int lara_splatdensify_children(const double *plan) {
    const double n = plan[LARA_SPLATDENSIFY_N];
    return n >= 1.0 && n <= 8.0 ? (int)n : 1;
}

// The statistics of surfel s after one render call: radii is [V][P], grad is the surfel's row of grad_means2D.
LARA_SPLATDENSIFY_HD void lara_splatdensify_accumulate_row(const int64_t P, const int V, const int64_t s, const float *grad, const int32_t *radii,
                                                           float *grad_sum, int32_t *seen, int32_t *max_radius) {
    bool any = false;
    int32_t most = 0;
    for (int v = 0; v < V; ++v) {
        const int32_t r = radii[(int64_t)v * P + s];
        any = any || r > 0;
        most = r > most ? r : most;
    }
    if (!any) return;
    const float gx = grad[0], gy = grad[1];
    if (lara_surfel_finite(gx) && lara_surfel_finite(gy)) {      // (n is finite exactly then: a square of an fp32 is far inside double)
        const double x = (double)gx, y = (double)gy;
        const double n = __builtin_sqrt(x * x + y * y);
        *grad_sum = lara_surfel_round((double)*grad_sum + n);
        *seen += 1;
    }
    if (most > *max_radius) *max_radius = most;
}

// The action of one surfel from its stored opacity logit, its two log scales and its statistics.
LARA_SPLATDENSIFY_HD int lara_splatdensify_action(const double *plan, const float opacity, const float s0, const float s1, const float grad_sum,
                                                  const int32_t seen, const int32_t max_radius) {
    const int flags = (int)plan[LARA_SPLATDENSIFY_FLAGS];
    const double avg = seen > 0 ? (double)grad_sum / (double)seen : 0.0;
    const bool hot = avg >= plan[LARA_SPLATDENSIFY_GRAD];                                   // (a NaN is not hot)
    const double a = (double)s0, b = (double)s1;
    const double smax = a > b ? a : b;
    if (flags & LARA_SPLATDENSIFY_ALLOW_PRUNE) {
        bool gone = (double)opacity < plan[LARA_SPLATDENSIFY_LOGIT_MIN];
        gone = gone || !lara_surfel_finite(opacity) || !lara_surfel_finite(s0) || !lara_surfel_finite(s1);
        if (plan[LARA_SPLATDENSIFY_MAX_SCREEN] > 0.0)
            gone = gone || (double)max_radius > plan[LARA_SPLATDENSIFY_MAX_SCREEN] || smax > plan[LARA_SPLATDENSIFY_LOG_WORLD];
        if (gone) return LARA_SPLATDENSIFY_PRUNE;
    }
    if (hot && smax > plan[LARA_SPLATDENSIFY_LOG_DENSE]) return (flags & LARA_SPLATDENSIFY_ALLOW_SPLIT) ? LARA_SPLATDENSIFY_SPLIT : LARA_SPLATDENSIFY_KEEP;
    if (hot && smax <= plan[LARA_SPLATDENSIFY_LOG_DENSE]) return (flags & LARA_SPLATDENSIFY_ALLOW_CLONE) ? LARA_SPLATDENSIFY_CLONE : LARA_SPLATDENSIFY_KEEP;
    return LARA_SPLATDENSIFY_KEEP;
}

// What surfel s contributes to the three segments of the scanned row: [s] a surviving original, [P + s] a clone, [2 P + s] children.
LARA_SPLATDENSIFY_HD void lara_splatdensify_flags(const int action, const int n_split, int32_t *first, int32_t *second, int32_t *third) {
    *first = action == LARA_SPLATDENSIFY_KEEP || action == LARA_SPLATDENSIFY_CLONE ? 1 : 0;
    *second = action == LARA_SPLATDENSIFY_CLONE ? 1 : 0;
    *third = action == LARA_SPLATDENSIFY_SPLIT ? n_split : 0;
}

// The five counts from the three segment totals: kept (action keep), cloned, split parents, pruned, P_out.
LARA_SPLATDENSIFY_HD void lara_splatdensify_counts(const int64_t P, const int n_split, const int64_t first, const int64_t second, const int64_t third,
                                                   int64_t *counts) {
    const int64_t parents = third / n_split;
    counts[0] = first - second;
    counts[1] = second;
    counts[2] = parents;
    counts[3] = P - first - parents;
    counts[4] = first + second + third;
}

// The output rows of source surfel s: row_source and row_child through the exclusive offsets.  A row at or beyond P_out is not written.
LARA_SPLATDENSIFY_HD void lara_splatdensify_rows_of(const int64_t P, const int n_split, const int64_t s, const int action, const int32_t *offset,
                                                    const int64_t P_out, int32_t *row_source, uint8_t *row_child) {
    if (action == LARA_SPLATDENSIFY_KEEP || action == LARA_SPLATDENSIFY_CLONE) {
        const int64_t o = offset[s];
        if (o >= 0 && o < P_out) row_source[o] = (int32_t)s, row_child[o] = LARA_SPLATDENSIFY_NO_CHILD;
    }
    if (action == LARA_SPLATDENSIFY_CLONE) {
        const int64_t o = offset[P + s];
        if (o >= 0 && o < P_out) row_source[o] = (int32_t)s, row_child[o] = LARA_SPLATDENSIFY_NO_CHILD;
    }
    if (action == LARA_SPLATDENSIFY_SPLIT) {
        const int64_t o0 = offset[2 * P + s];
        for (int k = 0; k < n_split; ++k) {
            const int64_t o = o0 + k;
            if (o >= 0 && o < P_out) row_source[o] = (int32_t)s, row_child[o] = (uint8_t)k;
        }
    }
}

// Coordinate r of a split child's centre: c + R(q / |q|) (exp(s0) z0, exp(s1) z1, 0), the rasteriser's (w, x, y, z) convention.
LARA_SPLATDENSIFY_HD float lara_splatdensify_child_center(const int r, const float *center, const float *scale, const float *rot, const float *z) {
    const double qw = (double)rot[0], qx = (double)rot[1], qy = (double)rot[2], qz = (double)rot[3];
    const double n2 = ((qw * qw + qx * qx) + qy * qy) + qz * qz;
    const double inv = 1.0 / __builtin_sqrt(n2);
    const double w = qw * inv, x = qx * inv, y = qy * inv, zz = qz * inv;
    double r0, r1;
    if (r == 0) {
        r0 = 1.0 - 2.0 * (y * y + zz * zz);
        r1 = 2.0 * (x * y - w * zz);
    } else if (r == 1) {
        r0 = 2.0 * (x * y + w * zz);
        r1 = 1.0 - 2.0 * (x * x + zz * zz);
    } else {
        r0 = 2.0 * (x * zz - w * y);
        r1 = 2.0 * (y * zz + w * x);
    }
    const double u = exp((double)scale[0]) * (double)z[0];
    const double v = exp((double)scale[1]) * (double)z[1];
    return lara_surfel_round((double)center[r] + (r0 * u + r1 * v));
}

// One output word: word r of row o of field F (width W), with its two moments.  `in` and `out` are the field's parameter, exp_avg and
// exp_avg_sq arrays; centers, scales and rotations are the INPUT cloud's (a split child reads them whatever its field).  Rows below
// `survivors` are surviving originals: their moments travel.  A source outside 0 .. P - 1 is not read: the three words become +0.0.
LARA_SPLATDENSIFY_HD void lara_splatdensify_word(const double *plan, const int field, const int64_t W, const int64_t o, const int64_t r, const int64_t P,
                                                 const int64_t survivors, const int n_split, const int32_t *row_source, const uint8_t *row_child,
                                                 const float *noise, const float *centers, const float *scales, const float *rotations,
                                                 const float *const *in, float *const *out) {
    const int64_t i = o * W + r;
    const int64_t src = row_source[o];
    const int child = row_child[o];
    if (src < 0 || src >= P || (child != LARA_SPLATDENSIFY_NO_CHILD && child >= n_split)) {
        out[0][i] = 0.0f, out[1][i] = 0.0f, out[2][i] = 0.0f;
        return;
    }
    const int64_t j = src * W + r;
    if (child != LARA_SPLATDENSIFY_NO_CHILD && field == 0)
        out[0][i] = lara_splatdensify_child_center((int)r, centers + 3 * src, scales + 2 * src, rotations + 4 * src,
                                                   noise + (src * n_split + child) * 2);
    else if (child != LARA_SPLATDENSIFY_NO_CHILD && field == 3)
        out[0][i] = lara_surfel_round((double)in[0][j] - plan[LARA_SPLATDENSIFY_LOG_SHRINK]);
    else
        __builtin_memcpy(out[0] + i, in[0] + j, sizeof(float));
    if (o < survivors) {
        __builtin_memcpy(out[1] + i, in[1] + j, sizeof(float));
        __builtin_memcpy(out[2] + i, in[2] + j, sizeof(float));
    } else {
        out[1][i] = 0.0f, out[2][i] = 0.0f;
    }
}

// ---- the host entries' loops (lara_splatdensify_*_host, tools/splatdensify_hostcheck.cpp) ---------------------------------------------------

inline void lara_splatdensify_host_accumulate(const int64_t P, const int V, const float *grad_means2D, const int32_t *radii, float *grad_sum,
                                              int32_t *seen, int32_t *max_radius) {
    for (int64_t s = 0; s < P; ++s) lara_splatdensify_accumulate_row(P, V, s, grad_means2D + 3 * s, radii, grad_sum + s, seen + s, max_radius + s);
}

inline void lara_splatdensify_host_decide(const double *plan, const int64_t P, const float *opacity, const float *scales, const float *grad_sum,
                                          const int32_t *seen, const int32_t *max_radius, uint8_t *action, int32_t *offset, int64_t *counts) {
    const int n_split = lara_splatdensify_children(plan);
    for (int64_t s = 0; s < P; ++s) {
        const int a = lara_splatdensify_action(plan, opacity[s], scales[2 * s], scales[2 * s + 1], grad_sum[s], seen[s], max_radius[s]);
        action[s] = (uint8_t)a;
        lara_splatdensify_flags(a, n_split, offset + s, offset + P + s, offset + 2 * P + s);
    }
    int64_t total[3] = {0, 0, 0}, run = 0;
    for (int seg = 0; seg < 3; ++seg)
        for (int64_t s = 0; s < P; ++s) {
            const int32_t f = offset[seg * P + s];
            offset[seg * P + s] = (int32_t)run;
            run += f;
            total[seg] += f;
        }
    lara_splatdensify_counts(P, n_split, total[0], total[1], total[2], counts);
}

// params / exp_avg / exp_avg_sq: five arrays each, in and out
inline void lara_splatdensify_host_apply(const double *plan, const int sh_degree, const int64_t P, const int64_t P_out, const int64_t survivors,
                                         const uint8_t *action, const int32_t *offset, const float *noise, const float *const *in,
                                         float *const *out, int32_t *row_source, uint8_t *row_child) {
    const int n_split = lara_splatdensify_children(plan);
    for (int64_t s = 0; s < P; ++s) lara_splatdensify_rows_of(P, n_split, s, action[s], offset, P_out, row_source, row_child);
    for (int f = 0; f < LARA_SURFEL_FIELDS; ++f) {
        const int64_t W = lara_surfel_width(f, sh_degree);
        const float *const fin[3] = {in[f], in[LARA_SURFEL_FIELDS + f], in[2 * LARA_SURFEL_FIELDS + f]};
        float *const fout[3] = {out[f], out[LARA_SURFEL_FIELDS + f], out[2 * LARA_SURFEL_FIELDS + f]};
        for (int64_t o = 0; o < P_out; ++o)
            for (int64_t r = 0; r < W; ++r)
                lara_splatdensify_word(plan, f, W, o, r, P, survivors, n_split, row_source, row_child, noise, in[0], in[3], in[4], fin, fout);
    }
}
