// tilebox.h -- which cells of a pixel grid a surfel's cull box meets: the ONE statement of that test, used by the composite's
// staging (2x2 pixel blocks of a tile) and by the preprocess's opt-in tight binning (16x16 tiles of the image), so that a
// (surfel, tile) pair the binning drops is a pair the staging would have dropped.  Plain C++: also compiled for the host by
// tests/test_tilebox_cpu.py.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define L2D_TILEBOX_FN __host__ __device__ __forceinline__
#else
#define L2D_TILEBOX_FN static inline
#endif

// Pixels sit at integer coordinates.  Cell g of a row of n cells of S pixels that starts at pixel `origin` covers the pixels
// origin + S g ... origin + S g + S - 1; the interval [lo, hi] meets it iff lo <= origin + S g + S - 1 and hi >= origin + S g.
// g0 / g1 = the first / last such cell of [0, n); none <=> g0 > g1.  (S a power of two: the scaling is exact.)
//   +-INF bounds clamp: the unbounded box (-INF, INF) gives [0, n - 1], the empty box (INF, -INF) gives (n, -1);
//   a NaN bound gives no cell on its side (fmaxf returns the other operand: g0 = 0 resp. g1 = -1) -- callers that must keep
//   such a surfel test for NaN themselves (l2d_tight_rect does).
template <int S>
L2D_TILEBOX_FN void l2d_box_cells(const float lo, const float hi, const float origin, const float n, int &g0, int &g1) {
    g0 = (int)ceilf(fminf(fmaxf((lo - origin - (float)(S - 1)) * (1.0f / (float)S), 0.f), n));
    g1 = (int)floorf(fminf(fmaxf((hi - origin) * (1.0f / (float)S), -1.f), n - 1.f));
}

// The 3-sigma tile rectangle [rx0, rx1) x [ry0, ry1) of a surfel cut down to the tiles its cull box (minx, maxx, miny, maxy)
// meets.  The empty box leaves no tile; the unbounded box, and a box with a NaN bound, leave the rectangle as it is.
// (Tiles are the binning contract's 16 x 16 pixels, gx x gy of them.)
L2D_TILEBOX_FN void l2d_tight_rect(const float minx, const float maxx, const float miny, const float maxy, const int gx,
                                   const int gy, int &rx0, int &ry0, int &rx1, int &ry1) {
    if (minx != minx || maxx != maxx || miny != miny || maxy != maxy) return;       // NaN: no statement about the surfel
    if (minx > maxx || miny > maxy) { rx0 = ry0 = rx1 = ry1 = 0; return; }         // empty: alpha never reaches 1/255
    int tx0, tx1, ty0, ty1;
    l2d_box_cells<16>(minx, maxx, 0.f, (float)gx, tx0, tx1);
    l2d_box_cells<16>(miny, maxy, 0.f, (float)gy, ty0, ty1);
    rx0 = rx0 > tx0 ? rx0 : tx0; rx1 = rx1 < tx1 + 1 ? rx1 : tx1 + 1;
    ry0 = ry0 > ty0 ? ry0 : ty0; ry1 = ry1 < ty1 + 1 ? ry1 : ty1 + 1;
    if (rx1 <= rx0 || ry1 <= ry0) rx0 = ry0 = rx1 = ry1 = 0;
}
