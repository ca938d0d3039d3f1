// Host program of tests/test_tilebox_cpu.py: lara_amd/csrc/tilebox.h against a brute-force loop over pixel coordinates.
//   cell g of n cells of S pixels from `origin` meets [lo, hi]  <=>  some pixel p of the cell has lo <= p and some has hi >= p
// Prints one line "cases <n> mismatches <m>" (and the first mismatches) and exits non-zero on any.
#include <cstdio>
#include <limits>
#include <vector>

#include "tilebox.h"

static int bad = 0;
static long cases = 0;

template <int S>
static void check_cells(float lo, float hi, float origin, int n) {
    int g0, g1;
    l2d_box_cells<S>(lo, hi, origin, (float)n, g0, g1);
    for (int g = 0; g < n; g++) {
        bool below = false, above = false;
        for (int k = 0; k < S; k++) {
            const double p = (double)origin + (double)(S * g + k);
            below = below || (double)lo <= p;
            above = above || (double)hi >= p;
        }
        const bool want = below && above, got = g0 <= g && g <= g1;
        cases++;
        if (want != got && bad++ < 10) std::printf("cells<%d> lo %g hi %g origin %g n %d cell %d: want %d got %d (g0 %d g1 %d)\n", S, lo, hi, origin, n, g, (int)want, (int)got, g0, g1);
    }
    if (g0 < 0 || g0 > n || g1 < -1 || g1 > n - 1) { if (bad++ < 10) std::printf("cells<%d> lo %g hi %g: range (%d, %d) outside the clamp\n", S, lo, hi, g0, g1); }
}

int main() {
    const float INF = std::numeric_limits<float>::infinity(), NAN_ = std::numeric_limits<float>::quiet_NaN();
    std::vector<float> b = {-INF, -1e30f, -100.f, -17.f, -16.f, -15.5f, -1.f, -0.5f, -1e-6f, 0.f, 1e-6f, 0.5f, 1.f, 14.5f, 14.999999f, 15.f,
                            15.000001f, 15.5f, 16.f, 16.000002f, 17.f, 30.999998f, 31.f, 31.000002f, 32.f, 47.f, 47.5f, 63.f, 63.000004f,
                            64.f, 79.f, 79.5f, 80.f, 95.f, 95.99999f, 96.f, 1000.f, 1e30f, INF};
    for (float lo : b)
        for (float hi : b)
            for (int n : {1, 4, 6}) {
                check_cells<16>(lo, hi, 0.f, n);
                if (lo > -1e29f && hi < 1e29f)      // (the staging's form: 2-pixel blocks of the tile at pixel `origin`)
                    for (float origin : {0.f, 16.f, 48.f}) check_cells<2>(lo, hi, origin, 8);
            }
    // the rectangle: every tile of the 3-sigma rectangle stays iff the box meets it in x and in y; special boxes
    const int gx = 6, gy = 4;
    std::vector<float> c = b;
    c.push_back(NAN_);
    const int rects[4][4] = {{0, 0, 6, 4}, {1, 1, 3, 2}, {2, 0, 6, 4}, {5, 3, 6, 4}};
    for (float minx : c) for (float maxx : c) for (float miny : {-INF, -3.f, 20.f, 70.f, INF, NAN_}) for (float maxy : {-INF, 15.f, 33.f, INF, NAN_})
        for (const auto &r : rects) {
            int x0 = r[0], y0 = r[1], x1 = r[2], y1 = r[3];
            l2d_tight_rect(minx, maxx, miny, maxy, gx, gy, x0, y0, x1, y1);
            const bool nan = minx != minx || maxx != maxx || miny != miny || maxy != maxy;
            const bool unbounded = minx == -INF && maxx == INF && miny == -INF && maxy == INF;
            const bool empty = !nan && (minx > maxx || miny > maxy);
            for (int ty = r[1]; ty < r[3]; ty++)
                for (int tx = r[0]; tx < r[2]; tx++) {
                    bool want;
                    if (nan || unbounded) want = true;
                    else if (empty) want = false;
                    else want = (double)minx <= 16.0 * tx + 15.0 && (double)maxx >= 16.0 * tx && (double)miny <= 16.0 * ty + 15.0 && (double)maxy >= 16.0 * ty;
                    const bool got = x0 <= tx && tx < x1 && y0 <= ty && ty < y1;
                    cases++;
                    if (want != got && bad++ < 10) std::printf("rect box (%g %g %g %g) in (%d %d %d %d) tile (%d, %d): want %d got %d\n", minx, maxx, miny, maxy, r[0], r[1], r[2], r[3], tx, ty, (int)want, (int)got);
                }
            // what is left is a rectangle inside the old one (or the empty one)
            const bool inside = (x0 == 0 && y0 == 0 && x1 == 0 && y1 == 0) || (x0 >= r[0] && y0 >= r[1] && x1 <= r[2] && y1 <= r[3] && x0 < x1 && y0 < y1);
            if (!inside && bad++ < 10) std::printf("rect box (%g %g %g %g): (%d %d %d %d) not inside (%d %d %d %d)\n", minx, maxx, miny, maxy, x0, y0, x1, y1, r[0], r[1], r[2], r[3]);
        }
    std::printf("cases %ld mismatches %d\n", cases, bad);
    return bad ? 1 : 0;
}
