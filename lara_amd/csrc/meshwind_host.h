// meshwind_host.h -- the two host entries of include/lara_meshwind.h as plain C++ on solidangle.h: meshwind.hip's
// lara_meshwind_solid_host and lara_meshwind_brute_host are these loops behind their argument checks, and
// tools/meshwind_hostcheck.cpp builds the same loops into a stand-alone program.  No device is touched.
#pragma once

#include <cmath>
#include <cstdint>

#include "solidangle.h"

// omega[i] = Omega of triangle i seen from point i
inline void lara_meshwind_solid_loop(const int64_t n, const float *points, const float *triangles9, double *omega) {
    for (int64_t i = 0; i < n; ++i) {
        const float *t = triangles9 + 9 * i;
        omega[i] = lara_solidangle(points + 3 * i, t, t + 3, t + 6);
    }
}

// w[i] = (the sum of Omega over the T triangles, in their order) / 4 pi; NaN for a point with a coordinate that is not finite
inline void lara_meshwind_brute_loop(const int64_t N, const float *points, const int64_t T, const float *triangles9, double *w) {
    for (int64_t i = 0; i < N; ++i) {
        const float *q = points + 3 * i;
        if (!(std::fabs(q[0]) < INFINITY && std::fabs(q[1]) < INFINITY && std::fabs(q[2]) < INFINITY)) {
            w[i] = (double)NAN;
            continue;
        }
        double sum = 0.0;
        for (int64_t j = 0; j < T; ++j) {
            const float *t = triangles9 + 9 * j;
            sum += lara_solidangle(q, t, t + 3, t + 6);
        }
        w[i] = sum / 12.566370614359172;
    }
}
