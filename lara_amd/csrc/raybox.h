// raybox.h -- the margined entry parameter of a ray into an axis-aligned box, one function for the device and the host
// (meshray.hip's walk and lara_meshray_box_entry_host).  fp32 box, the ray as lara_ray_setup (raytri.h) left it, every operation in
// double, in the order written here and stated in include/lara_meshray.h, where the margins are derived; the unit is built
// with -ffp-contract=off.  Whenever lara_raytri computes a hit at t for a triangle with its vertices in the box, the result is
// finite and <= t.
#pragma once

#include "raytri.h"

#define LARA_RAYBOX_INFLATE 1.9073486328125e-06                  // 2^-19
#define LARA_RAYBOX_REL 9.094947017729282379150390625e-13        // 2^-40

// one axis: [near, far] <- its intersection with the slab's own parameter interval; false: the ray runs beside the slab
LARA_RAYTRI_HD bool lara_raybox_axis(const double o, const double d, const double inv, const float lof, const float hif,
                                     double &near, double &far) {
    const double lo = (double)lof, hi = (double)hif;
    const double m0 = lara_raytri_abs(o), m1 = lara_raytri_abs(lo), m2 = lara_raytri_abs(hi);
    const double e = LARA_RAYBOX_INFLATE * (m0 > m1 ? (m0 > m2 ? m0 : m2) : (m1 > m2 ? m1 : m2));
    const double l = lo - e, h = hi + e;
    if (d == 0.0) return o >= l && o <= h;
    const double t1 = (l - o) * inv, t2 = (h - o) * inv;
    double n = t1 < t2 ? t1 : t2, f = t1 < t2 ? t2 : t1;
    n = n - LARA_RAYBOX_REL * lara_raytri_abs(n);
    f = f + LARA_RAYBOX_REL * lara_raytri_abs(f);
    near = n > near ? n : near;
    far = f < far ? f : far;
    return true;
}

// +inf: an empty box (not lo_x <= hi_x, which a NaN is too), a ray that never hits, or no parameter in [t_min, t_hi] inside the
// inflated box; else max(t_min, the widened entry parameter)
LARA_RAYTRI_HD double lara_raybox(const LaraRay &r, const float lof[3], const float hif[3], const double t_min, const double t_hi) {
    const double none = __builtin_inf();
    if (!(lof[0] <= hif[0]) || !r.ok) return none;
    double near = t_min, far = t_hi;
    if (!lara_raybox_axis(r.o[0], r.d[0], r.inv[0], lof[0], hif[0], near, far)) return none;
    if (!lara_raybox_axis(r.o[1], r.d[1], r.inv[1], lof[1], hif[1], near, far)) return none;
    if (!lara_raybox_axis(r.o[2], r.d[2], r.inv[2], lof[2], hif[2], near, far)) return none;
    return near <= far ? near : none;
}
