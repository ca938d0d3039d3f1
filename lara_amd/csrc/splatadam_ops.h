// splatadam_ops.h -- the per-word function of lara_splatadam.h, one definition for the device and the host (splatadam.hip's kernel,
// lara_splatadam_step_host, tools/splatadam_hostcheck.cpp): one fp32 word of a parameter with its gradient and its two moments under
// the plan of one Adam step.  Double arithmetic on the fp32 inputs with + - * / and sqrt only, one rounding to fp32 per store, the
// operation order of the header.  Include it from units built with -ffp-contract=off only.
#pragma once

#include <stdint.h>

#include "surfel_ops.h"                          // the five fields and their widths, lara_surfel_finite, lara_surfel_round

#define LARA_SPLATADAM_HD LARA_SURFEL_HD

// offsets into the plan (lara_splatadam.h)
#define LARA_SPLATADAM_B1 0
#define LARA_SPLATADAM_1MB1 1
#define LARA_SPLATADAM_B2 2
#define LARA_SPLATADAM_1MB2 3
#define LARA_SPLATADAM_BC1 4
#define LARA_SPLATADAM_SQRT_BC2 5
#define LARA_SPLATADAM_EPS 6
#define LARA_SPLATADAM_LR 7                      // centres, SH coefficient 0, SH coefficients >= 1, opacity, scales, rotations

// the learning rate of word r of a surfel's row of field f (r < 3 of shs: coefficient 0); selects, no indexed read of the plan
LARA_SPLATADAM_HD double lara_splatadam_rate(const double *plan, const int field, const int64_t r) {
    const double *lr = plan + LARA_SPLATADAM_LR;
    return field == 0 ? lr[0] : field == 1 ? (r < 3 ? lr[1] : lr[2]) : field == 2 ? lr[3] : field == 3 ? lr[4] : lr[5];
}

// One word whose surfel is visible.  Returns 1 where the gradient is not finite: p, m and v then stay as they are.  A NaN (from a
// moment or a parameter that came in non-finite) is stored as 0x7FC00000 on either side.
LARA_SPLATADAM_HD int lara_splatadam_word(const double *plan, const double lr, float *p, float *g, float *m, float *v, const int zero_grads) {
    const float gf = *g;
    if (zero_grads) *g = 0.0f;
    if (!lara_surfel_finite(gf)) return 1;
    const double gd = (double)gf, md = (double)*m, vd = (double)*v, pd = (double)*p;
    const double m1 = md + (gd - md) * plan[LARA_SPLATADAM_1MB1];
    const double v1 = plan[LARA_SPLATADAM_B2] * vd + (plan[LARA_SPLATADAM_1MB2] * gd) * gd;
    const double denom = __builtin_sqrt(v1) / plan[LARA_SPLATADAM_SQRT_BC2] + plan[LARA_SPLATADAM_EPS];
    const double p1 = pd - (lr / plan[LARA_SPLATADAM_BC1]) * (m1 / denom);
    *m = lara_surfel_round(m1);
    *v = lara_surfel_round(v1);
    *p = lara_surfel_round(p1);
    return 0;
}

// The host entry's loop (lara_splatadam_step_host, tools/splatadam_hostcheck.cpp): field by field, word by word.  Returns the number
// of words skipped for a non-finite gradient.
inline int64_t lara_splatadam_host_words(const double *plan, const int sh_degree, const int64_t P, float *const *params, float *const *grads,
                                         float *const *exp_avg, float *const *exp_avg_sq, const uint8_t *visible, const int zero_grads) {
    int64_t skipped = 0;
    for (int f = 0; f < LARA_SURFEL_FIELDS; ++f) {
        const int64_t W = lara_surfel_width(f, sh_degree);
        for (int64_t s = 0; s < P; ++s)
            for (int64_t r = 0; r < W; ++r) {
                const int64_t i = s * W + r;
                if (visible && !visible[s]) {
                    if (zero_grads) grads[f][i] = 0.0f;
                    continue;
                }
                skipped += lara_splatadam_word(plan, lara_splatadam_rate(plan, f, r), params[f] + i, grads[f] + i, exp_avg[f] + i,
                                               exp_avg_sq[f] + i, zero_grads);
            }
    }
    return skipped;
}
