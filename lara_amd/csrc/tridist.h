// tridist.h -- the squared distance from a point to a triangle and the closest point, one function for the device and the host
// (meshdist.hip's kernels and lara_meshdist_point_triangle_host).  fp32 inputs, every operation in double, in the order written
// here and stated in include/lara_meshdist.h; the unit is built with -ffp-contract=off, so this sequence is the
// instruction sequence.  With finite fp32 inputs no intermediate leaves double's range (|n . n| < 2^520) and the result is finite.
#pragma once

#if defined(__HIPCC__)
#define LARA_TRIDIST_HD __host__ __device__ __forceinline__
#else
#define LARA_TRIDIST_HD inline
#endif

// (a x b) . n, summed left to right
LARA_TRIDIST_HD double lara_tridist_edge(const double e[3], const double w[3], const double n[3]) {
    const double cx = e[1] * w[2] - e[2] * w[1], cy = e[2] * w[0] - e[0] * w[2], cz = e[0] * w[1] - e[1] * w[0];
    return (cx * n[0] + cy * n[1]) + cz * n[2];
}

// the squared distance from q to the segment a b; c = the closest point
LARA_TRIDIST_HD double lara_tridist_segment(const double q[3], const double a[3], const double b[3], double c[3]) {
    const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
    const double aq[3] = {q[0] - a[0], q[1] - a[1], q[2] - a[2]};
    const double den = (ab[0] * ab[0] + ab[1] * ab[1]) + ab[2] * ab[2];
    const double num = (aq[0] * ab[0] + aq[1] * ab[1]) + aq[2] * ab[2];
    double t = 0.0;
    if (den > 0.0) {
        t = num / den;
        t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    }
    c[0] = a[0] + t * ab[0];
    c[1] = a[1] + t * ab[1];
    c[2] = a[2] + t * ab[2];
    const double dx = q[0] - c[0], dy = q[1] - c[1], dz = q[2] - c[2];
    return (dx * dx + dy * dy) + dz * dz;
}

// d2 = the squared distance from q to the triangle p0 p1 p2; closest[3] = the point of the triangle that attains it
LARA_TRIDIST_HD double lara_tridist(const float qf[3], const float p0f[3], const float p1f[3], const float p2f[3], double closest[3]) {
    const double q[3] = {(double)qf[0], (double)qf[1], (double)qf[2]};
    const double p0[3] = {(double)p0f[0], (double)p0f[1], (double)p0f[2]};
    const double p1[3] = {(double)p1f[0], (double)p1f[1], (double)p1f[2]};
    const double p2[3] = {(double)p2f[0], (double)p2f[1], (double)p2f[2]};
    const double e0[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
    const double e2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
    const double n[3] = {e0[1] * e2[2] - e0[2] * e2[1], e0[2] * e2[0] - e0[0] * e2[2], e0[0] * e2[1] - e0[1] * e2[0]};
    const double nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
    if (nn > 0.0) {
        const double e1[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
        const double e3[3] = {p0[0] - p2[0], p0[1] - p2[1], p0[2] - p2[2]};
        const double w0[3] = {q[0] - p0[0], q[1] - p0[1], q[2] - p0[2]};
        const double w1[3] = {q[0] - p1[0], q[1] - p1[1], q[2] - p1[2]};
        const double w2[3] = {q[0] - p2[0], q[1] - p2[1], q[2] - p2[2]};
        const double f0 = lara_tridist_edge(e0, w0, n), f1 = lara_tridist_edge(e1, w1, n), f2 = lara_tridist_edge(e3, w2, n);
        if (f0 >= 0.0 && f1 >= 0.0 && f2 >= 0.0) {      // the projection of q lies in the triangle
            const double s = (n[0] * w0[0] + n[1] * w0[1]) + n[2] * w0[2];
            const double t = s / nn;
            closest[0] = q[0] - t * n[0];
            closest[1] = q[1] - t * n[1];
            closest[2] = q[2] - t * n[2];
            return (s * s) / nn;
        }
    }
    // the three sides, in the order p0 p1, p1 p2, p2 p0; a later side wins only when strictly nearer
    double c[3];
    double d2 = lara_tridist_segment(q, p0, p1, closest);
    double d = lara_tridist_segment(q, p1, p2, c);
    if (d < d2) { d2 = d; closest[0] = c[0]; closest[1] = c[1]; closest[2] = c[2]; }
    d = lara_tridist_segment(q, p2, p0, c);
    if (d < d2) { d2 = d; closest[0] = c[0]; closest[1] = c[1]; closest[2] = c[2]; }
    return d2;
}
