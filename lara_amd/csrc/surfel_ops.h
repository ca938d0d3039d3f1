// surfel_ops.h -- what the three surfel units share (splatxform_ops.h, splatadam_ops.h, splatdensify_ops.h include it): the fields of a
// cloud and their widths, the finite test and the one rounding of an fp32 word, one definition for the device and the host, and the
// host-side layout of a grid that gives every field its own run of workgroups (splatadam.hip, splatdensify.hip).  Include it from
// units built with -ffp-contract=off only.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define LARA_SURFEL_HD __host__ __device__ __forceinline__
#else
#define LARA_SURFEL_HD inline
#endif

#define LARA_SURFEL_FIELDS 5

// words per surfel of field f (centers, shs, opacity, scales, rotations) at an SH degree
LARA_SURFEL_HD int64_t lara_surfel_width(const int field, const int sh_degree) {
    return field == 0 ? 3 : field == 1 ? 3 * (int64_t)(sh_degree + 1) * (sh_degree + 1) : field == 2 ? 1 : field == 3 ? 2 : 4;
}

// a finite fp32 word: its exponent field is not all ones
LARA_SURFEL_HD bool lara_surfel_finite(const float g) {
    uint32_t w;
    __builtin_memcpy(&w, &g, sizeof w);
    return (w & 0x7F800000u) != 0x7F800000u;
}

// fl32 of the headers: the one rounding; a NaN becomes 0x7FC00000
LARA_SURFEL_HD float lara_surfel_round(const double v) {
    const float f = (float)v;
    const uint32_t qnan = 0x7FC00000u;
    float n;
    __builtin_memcpy(&n, &qnan, sizeof n);
    return f == f ? f : n;
}

// The grid of a kernel that runs `span` words of ONE field per workgroup over `rows` surfels: words[f] the fp32 words of field f,
// first[f] its first workgroup, first[5] the grid.  Host code.  False where the grid would exceed the 2^31 - 1 workgroups of a launch.
inline bool lara_surfel_grid(const int64_t rows, const int sh_degree, const int span, long long *words, unsigned *first) {
    int64_t blocks = 0;
    for (int f = 0; f < LARA_SURFEL_FIELDS; ++f) {
        words[f] = (long long)(rows * lara_surfel_width(f, sh_degree));
        first[f] = (unsigned)blocks;
        blocks += (words[f] + span - 1) / span;
        if (blocks > 0x7fffffffll) return false;
    }
    first[LARA_SURFEL_FIELDS] = (unsigned)blocks;
    return true;
}
