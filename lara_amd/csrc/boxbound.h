// boxbound.h -- the margined lower bound of the squared distance from a point to an axis-aligned box, one function for the device
// and the host (meshbvh.hip's query kernel and lara_meshbvh_box_bound_host).  fp32 inputs, every operation in double, in the order
// written here and stated in include/lara_meshbvh.h, where the margin is derived; the unit is built with -ffp-contract=off.
// The result never exceeds the d2 lara_tridist (tridist.h) computes for a triangle with its vertices in the box.
#pragma once

#if defined(__HIPCC__)
#define LARA_BOXBOUND_HD __host__ __device__ __forceinline__
#else
#define LARA_BOXBOUND_HD inline
#endif

#define LARA_BOXBOUND_REL 0.000244140625                   // 2^-12
#define LARA_BOXBOUND_ABS 9.094947017729282379150390625e-13      // 2^-40

LARA_BOXBOUND_HD double lara_boxbound_abs(const float x) { return x < 0.0f ? -(double)x : (double)x; }

// g g of one axis, g = max(lo - q, q - hi, 0); M <- max(M, |q|, |lo|, |hi|)
LARA_BOXBOUND_HD double lara_boxbound_axis(const float qf, const float lof, const float hif, double &M) {
    const double q = (double)qf, lo = (double)lof, hi = (double)hif;
    const double below = lo - q, above = q - hi;
    double g = below > above ? below : above;
    g = g > 0.0 ? g : 0.0;
    const double m0 = lara_boxbound_abs(qf), m1 = lara_boxbound_abs(lof), m2 = lara_boxbound_abs(hif);
    const double m = m0 > m1 ? (m0 > m2 ? m0 : m2) : (m1 > m2 ? m1 : m2);
    M = m > M ? m : M;
    return g * g;
}

// +inf for an empty box (not lo_x <= hi_x, which a NaN is too); else max(0, s - (2^-12 s + 2^-40 M M))
LARA_BOXBOUND_HD double lara_boxbound(const float qf[3], const float lof[3], const float hif[3]) {
    if (!(lof[0] <= hif[0])) return __builtin_inf();
    double M = 0.0;
    const double gx = lara_boxbound_axis(qf[0], lof[0], hif[0], M);
    const double gy = lara_boxbound_axis(qf[1], lof[1], hif[1], M);
    const double gz = lara_boxbound_axis(qf[2], lof[2], hif[2], M);
    const double s = (gx + gy) + gz;
    const double b = s - (LARA_BOXBOUND_REL * s + LARA_BOXBOUND_ABS * (M * M));
    return b > 0.0 ? b : 0.0;
}
