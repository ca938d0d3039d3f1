// meshsign_hostcheck.cpp -- csrc/raycross.h (on csrc/raytri.h) as plain host C++, over the (ray, triangle) groups of
// tests/meshray_cases.bound_groups and the crafted rays at the corners and edges of the dyadic cube (tests/meshsign_cases.py), for
// a build with -fsanitize=address,undefined (tools/meshsign_hostcheck.py writes the records, compiles this file and runs it;
// nothing here touches a device or is loaded into python).
//   meshsign_hostcheck <records.bin>     int64 n, then n records of 18 fp32: o[3], d[3], p0[3], p1[3], p2[3], then expected
//                                        hit, orient, touch (the float64 restatement's, as floats)
// Prints the records read, the crossings, the touching ones, those leaving through their face, disagreements with lara_raytri's
// acceptance in [0, +inf) (must be 0) and with the restatement (must be 0); exit 1 on a violation.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../lara_amd/csrc/raycross.h"

int main(int argc, char **argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: meshsign_hostcheck <records.bin>\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "meshsign_hostcheck: cannot open %s\n", argv[1]); return 2; }
    int64_t n = 0;
    if (std::fread(&n, sizeof n, 1, f) != 1 || n < 0 || n > (1ll << 28)) { std::fclose(f); return 2; }
    std::vector<float> rows((size_t)n * 18);
    const size_t got = std::fread(rows.data(), sizeof(float), rows.size(), f);
    std::fclose(f);
    if (got != rows.size()) { std::fprintf(stderr, "meshsign_hostcheck: short file\n"); return 2; }
    int64_t hits = 0, touching = 0, leaving = 0, not_raytri = 0, not_restated = 0;
    for (int64_t i = 0; i < n; ++i) {
        const float *r = rows.data() + 18 * (size_t)i;
        const LaraRay ray = lara_ray_setup(r, r + 3);
        int orient = 0, touch = 0;
        const bool hit = lara_raycross(ray, r + 6, r + 9, r + 12, orient, touch);
        double t = 0.0, b[3] = {0.0, 0.0, 0.0};
        if (hit != lara_raytri(ray, 0.0, INFINITY, r + 6, r + 9, r + 12, t, b)) ++not_raytri;
        if (!hit) { orient = 0; touch = 0; }
        if ((float)(hit ? 1 : 0) != r[15] || (float)orient != r[16] || (float)touch != r[17]) ++not_restated;
        hits += hit ? 1 : 0;
        touching += touch;
        leaving += orient == 1 ? 1 : 0;
    }
    std::printf("records %lld, crossings %lld, touching %lld, leaving %lld, not lara_raytri's acceptance %lld, not the restatement's "
                "%lld\n", (long long)n, (long long)hits, (long long)touching, (long long)leaving, (long long)not_raytri,
                (long long)not_restated);
    return not_raytri || not_restated ? 1 : 0;
}
