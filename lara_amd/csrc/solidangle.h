// solidangle.h -- the signed solid angle of one triangle seen from a point (Van Oosterom and Strackee): one function for the device
// and the host (meshwind.hip's walk, lara_meshwind_solid_host, lara_meshwind_brute_host, tools/meshwind_hostcheck.cpp).  All
// arithmetic is double on the fp32 inputs, in the order written here; under -ffp-contract=off the sequence is the instructions, and
// atan2 is the only operation that is not correctly rounded.  Stated in include/lara_meshwind.h.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define LARA_SOLIDANGLE_HD __host__ __device__ __forceinline__
#else
#define LARA_SOLIDANGLE_HD inline
#endif

// Omega in (-2 pi, 2 pi]: positive when the point sees the face whose normal (p1 - p0) x (p2 - p0) points away from it.
//     a = p0 - q, b = p1 - q, c = p2 - q                                   (componentwise)
//     x = b x c:  x_0 = b_1 c_2 - b_2 c_1,  x_1 = b_2 c_0 - b_0 c_2,  x_2 = b_0 c_1 - b_1 c_0
//     num = (a_0 x_0 + a_1 x_1) + a_2 x_2
//     |v| = sqrt((v_0 v_0 + v_1 v_1) + v_2 v_2),   u . v = (u_0 v_0 + u_1 v_1) + u_2 v_2
//     den = (|a| (|b| |c|) + (b . c) |a|) + ((a . b) |c| + (c . a) |b|)
//     Omega = 2 atan2(num, den)
// The rule: num == 0 gives exactly 0 -- a triangle without area, q in the triangle's plane (on the triangle or beside it), q at a
// vertex.  It is a test on num: atan2(+-0, negative) is +-pi, which would count half a turn for a point ON a face.
// den is written symmetric in p1 and p2, and num changes its sign exactly under that swap: the flipped triangle gives -Omega, bit for bit.
LARA_SOLIDANGLE_HD double lara_solidangle(const float q[3], const float p0[3], const float p1[3], const float p2[3]) {
    const double a[3] = {(double)p0[0] - (double)q[0], (double)p0[1] - (double)q[1], (double)p0[2] - (double)q[2]};
    const double b[3] = {(double)p1[0] - (double)q[0], (double)p1[1] - (double)q[1], (double)p1[2] - (double)q[2]};
    const double c[3] = {(double)p2[0] - (double)q[0], (double)p2[1] - (double)q[1], (double)p2[2] - (double)q[2]};
    const double x0 = b[1] * c[2] - b[2] * c[1], x1 = b[2] * c[0] - b[0] * c[2], x2 = b[0] * c[1] - b[1] * c[0];
    const double num = (a[0] * x0 + a[1] * x1) + a[2] * x2;
    if (num == 0.0) return 0.0;
    const double la = sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
    const double lb = sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]);
    const double lc = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
    const double ab = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
    const double bc = (b[0] * c[0] + b[1] * c[1]) + b[2] * c[2];
    const double ca = (c[0] * a[0] + c[1] * a[1]) + c[2] * a[2];
    const double den = (la * (lb * lc) + bc * la) + (ab * lc + ca * lb);
    return 2.0 * atan2(num, den);
}
