// raycross.h -- one crossing of a ray through a triangle, with its orientation: one function for the device and the host
// (meshsign.hip's counting walk, lara_meshsign_cross_host, tools/meshsign_hostcheck.cpp).  It accepts exactly when lara_raytri
// (raytri.h) accepts in the window [0, +inf), and computes U, V, W again through lara_raytri_shear in raytri.h's order: under
// -ffp-contract=off the same sequence gives the same bits.  Stated in include/lara_meshsign.h.
#pragma once

#include "raytri.h"

// true: the ray o + t d, t >= 0, crosses the triangle p0 p1 p2.  orient = +1 when det = (U + V) + W < 0: the ray leaves through a
// face whose normal (p1 - p0) x (p2 - p0) points along it; else -1.  touch = 1 when one of U, V, W is exactly zero: the ray meets
// an edge or a vertex of the triangle as computed, and every triangle around that edge or vertex counts it too.
LARA_RAYTRI_HD bool lara_raycross(const LaraRay &r, const float p0[3], const float p1[3], const float p2[3], int &orient, int &touch) {
    double t, b[3];
    if (!lara_raytri(r, 0.0, __builtin_inf(), p0, p1, p2, t, b)) return false;
    double Ax, Ay, Az, Bx, By, Bz, Cx, Cy, Cz;
    lara_raytri_shear(r, p0, Ax, Ay, Az);
    lara_raytri_shear(r, p1, Bx, By, Bz);
    lara_raytri_shear(r, p2, Cx, Cy, Cz);
    const double U = Cx * By - Cy * Bx;
    const double V = Ax * Cy - Ay * Cx;
    const double W = Bx * Ay - By * Ax;
    const double det = (U + V) + W;
    orient = det < 0.0 ? 1 : -1;
    touch = (U == 0.0 || V == 0.0 || W == 0.0) ? 1 : 0;
    return true;
}
