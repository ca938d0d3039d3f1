// meshtopo_ops.h -- the two per-vertex functions of include/lara_meshtopo.h, one definition for the device and the host
// (meshtopo.hip's kernels, lara_meshtopo_normals_host, lara_meshtopo_smooth_host, tools/meshtopo_hostcheck.cpp): the normal of a
// vertex over its row of the face table and the smoothing step of a vertex over its row of the neighbour table.  Double arithmetic
// on the fp32 inputs, one rounding to fp32 at the end; the rows are walked from their first entry to their last, and that order is
// the contract.  Include it from units built with -ffp-contract=off only.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LARA_MESHTOPO_HD __host__ __device__ __forceinline__
#else
#define LARA_MESHTOPO_HD inline
#endif

// The normal of the vertex whose row of `faces` [.][2] (triangle, corner) is [begin, end): weighting 0 sums the raw cross products
// (area weights), 1 their unit vectors (a face without area is skipped).  Returns 1 when the sum has no direction -- its length is
// zero, infinite or NaN -- and out is then (0, 0, 0); else 0.
LARA_MESHTOPO_HD int lara_meshtopo_normal(const float *vertices, const int32_t *triangles, const int32_t *faces, const int64_t begin,
                                          const int64_t end, const int weighting, float out[3]) {
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int64_t i = begin; i < end; ++i) {
        const int32_t *f = triangles + 3 * (int64_t)faces[2 * i];
        const float *p0 = vertices + 3 * (int64_t)f[0], *p1 = vertices + 3 * (int64_t)f[1], *p2 = vertices + 3 * (int64_t)f[2];
        const double ux = (double)p1[0] - (double)p0[0], uy = (double)p1[1] - (double)p0[1], uz = (double)p1[2] - (double)p0[2];
        const double wx = (double)p2[0] - (double)p0[0], wy = (double)p2[1] - (double)p0[1], wz = (double)p2[2] - (double)p0[2];
        double cx = uy * wz - uz * wy, cy = uz * wx - ux * wz, cz = ux * wy - uy * wx;
        if (weighting != 0) {
            const double l = sqrt((cx * cx + cy * cy) + cz * cz);
            if (l == 0.0) continue;
            cx = cx / l;
            cy = cy / l;
            cz = cz / l;
        }
        sx += cx;
        sy += cy;
        sz += cz;
    }
    const double L = sqrt((sx * sx + sy * sy) + sz * sz);
    if (!(L > 0.0) || !(L < __builtin_inf())) {
        out[0] = out[1] = out[2] = 0.0f;
        return 1;
    }
    out[0] = (float)(sx / L);
    out[1] = (float)(sy / L);
    out[2] = (float)(sz / L);
    return 0;
}

// The smoothing step of vertex v, whose row of `neighbors` is [begin, end): x' = x + s (mean - x).  An empty row, and keep != 0,
// copy the position.
LARA_MESHTOPO_HD void lara_meshtopo_smooth(const float *src, const int32_t *neighbors, const int64_t begin, const int64_t end,
                                           const double s, const int keep, const int64_t v, float out[3]) {
    const float *x = src + 3 * v;
    if (end <= begin || keep) {
        out[0] = x[0];
        out[1] = x[1];
        out[2] = x[2];
        return;
    }
    double mx = 0.0, my = 0.0, mz = 0.0;
    for (int64_t i = begin; i < end; ++i) {
        const float *q = src + 3 * (int64_t)neighbors[i];
        mx += (double)q[0];
        my += (double)q[1];
        mz += (double)q[2];
    }
    const double degree = (double)(end - begin);
    mx = mx / degree;
    my = my / degree;
    mz = mz / degree;
    out[0] = (float)((double)x[0] + s * (mx - (double)x[0]));
    out[1] = (float)((double)x[1] + s * (my - (double)x[1]));
    out[2] = (float)((double)x[2] + s * (mz - (double)x[2]));
}
