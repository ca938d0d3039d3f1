// raytri.h -- does a ray meet a triangle, and where: one function for the device and the host (meshray.hip's kernels and
// lara_meshray_raytri_host).  fp32 inputs, every operation in double, in the order written here and stated in
// include/lara_meshray.h; the unit is built with -ffp-contract=off, so this sequence is the instruction sequence.
// The ray is sheared so that it runs along +z, once per ray (lara_ray_setup); a vertex's sheared position depends on the ray and
// the vertex alone, so every triangle around an edge or a vertex classifies the ray against the same computed points, and the
// edge functions U, V, W -- one product pair and one subtraction each, monotone under rounding -- never give two neighbours
// contradicting signs: a ray cannot slip between two triangles of a closed surface.
#pragma once

#if defined(__HIPCC__)
#define LARA_RAYTRI_HD __host__ __device__ __forceinline__
#else
#define LARA_RAYTRI_HD inline
#endif

#define LARA_RAYTRI_SANITY 9.5367431640625e-07      // 2^-20

// what lara_raytri and lara_raybox need of a ray, computed once
struct LaraRay {
    double o[3], d[3];
    double inv[3];            // 1 / d_a (raybox.h; unused where d_a == 0)
    double Sx, Sy, Sz;        // the shear
    int kx, ky, kz;
    bool ok;                  // false: the ray never hits (a component that is not finite, or d = 0)
};

LARA_RAYTRI_HD double lara_raytri_abs(const double x) { return x < 0.0 ? -x : x; }
LARA_RAYTRI_HD bool lara_raytri_finite(const float x) { return lara_raytri_abs((double)x) < __builtin_inf(); }

LARA_RAYTRI_HD LaraRay lara_ray_setup(const float of[3], const float df[3]) {
    LaraRay r;
    bool ok = true;
    for (int a = 0; a < 3; a++) {
        r.o[a] = (double)of[a];
        r.d[a] = (double)df[a];
        ok = ok && lara_raytri_finite(of[a]) && lara_raytri_finite(df[a]);
    }
    const double ax = lara_raytri_abs(r.d[0]), ay = lara_raytri_abs(r.d[1]), az = lara_raytri_abs(r.d[2]);
    int kz = 0;                                   // the axis of the largest |d_a|, the first one on a tie
    if (ay > ax) kz = 1;
    if (az > (kz == 1 ? ay : ax)) kz = 2;
    int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
    const double dz = kz == 0 ? r.d[0] : (kz == 1 ? r.d[1] : r.d[2]);
    if (dz < 0.0) { const int s = kx; kx = ky; ky = s; }
    const double dx = kx == 0 ? r.d[0] : (kx == 1 ? r.d[1] : r.d[2]);
    const double dy = ky == 0 ? r.d[0] : (ky == 1 ? r.d[1] : r.d[2]);
    ok = ok && dz != 0.0;
    const double den = ok ? dz : 1.0;
    r.Sx = dx / den;
    r.Sy = dy / den;
    r.Sz = 1.0 / den;
    for (int a = 0; a < 3; a++) r.inv[a] = 1.0 / (r.d[a] != 0.0 && ok ? r.d[a] : 1.0);
    r.kx = kx; r.ky = ky; r.kz = kz;
    r.ok = ok;
    return r;
}

LARA_RAYTRI_HD double lara_raytri_pick(const double a[3], const int k) { return k == 0 ? a[0] : (k == 1 ? a[1] : a[2]); }

// the sheared position of vertex p: X, Y across the ray, Z along it (in units of t)
LARA_RAYTRI_HD void lara_raytri_shear(const LaraRay &r, const float pf[3], double &X, double &Y, double &Z) {
    const double a[3] = {(double)pf[0] - r.o[0], (double)pf[1] - r.o[1], (double)pf[2] - r.o[2]};
    const double az = lara_raytri_pick(a, r.kz);
    X = lara_raytri_pick(a, r.kx) - r.Sx * az;
    Y = lara_raytri_pick(a, r.ky) - r.Sy * az;
    Z = r.Sz * az;
}

// true: the ray meets the triangle p0 p1 p2 at o + t d with t_min <= t <= t_max; b[3] = the barycentric weights of p0, p1, p2.
// Both sides count, zeros of the edge functions are inclusive.  The sanity clause: the computed point lies in the triangle's
// box, widened by 2^-20 of the larger of |o_a| and the vertices' |p_a|, on every axis.
LARA_RAYTRI_HD bool lara_raytri(const LaraRay &r, const double t_min, const double t_max, const float p0[3], const float p1[3],
                                const float p2[3], double &t, double b[3]) {
    if (!r.ok) return false;
    double Ax, Ay, Az, Bx, By, Bz, Cx, Cy, Cz;
    lara_raytri_shear(r, p0, Ax, Ay, Az);
    lara_raytri_shear(r, p1, Bx, By, Bz);
    lara_raytri_shear(r, p2, Cx, Cy, Cz);
    const double U = Cx * By - Cy * Bx;
    const double V = Ax * Cy - Ay * Cx;
    const double W = Bx * Ay - By * Ax;
    if (!((U >= 0.0 && V >= 0.0 && W >= 0.0) || (U <= 0.0 && V <= 0.0 && W <= 0.0))) return false;
    const double det = (U + V) + W;
    if (!(det != 0.0)) return false;
    const double tt = ((U * Az + V * Bz) + W * Cz) / det;
    if (!(t_min <= tt && tt <= t_max)) return false;
    for (int a = 0; a < 3; a++) {
        const double q0 = (double)p0[a], q1 = (double)p1[a], q2 = (double)p2[a];
        double mn = q0 < q1 ? q0 : q1, mx = q0 > q1 ? q0 : q1;
        mn = mn < q2 ? mn : q2;
        mx = mx > q2 ? mx : q2;
        const double m0 = lara_raytri_abs(r.o[a]), m1 = lara_raytri_abs(mn), m2 = lara_raytri_abs(mx);
        const double m = LARA_RAYTRI_SANITY * (m0 > m1 ? (m0 > m2 ? m0 : m2) : (m1 > m2 ? m1 : m2));
        const double x = r.o[a] + tt * r.d[a];
        if (!(x >= mn - m && x <= mx + m)) return false;
    }
    t = tt;
    b[0] = U / det;
    b[1] = V / det;
    b[2] = W / det;
    return true;
}
