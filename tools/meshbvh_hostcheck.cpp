// meshbvh_hostcheck.cpp -- csrc/boxbound.h and csrc/tridist.h as plain host C++, over the (query, triangle, box) pairs of
// tests/meshbvh_cases.bound_pairs, for a build with -fsanitize=address,undefined (tools/meshbvh_hostcheck.py writes the pairs,
// compiles this file and runs it; nothing here touches a device or is loaded into python).
//   meshbvh_hostcheck <pairs.bin>      pairs.bin: int64 n, then n records of 18 fp32: q[3], p0[3], p1[3], p2[3], lo[3], hi[3]
// Prints the pairs read, those with bound > d2 (must be 0), non-finite results (must be 0) and the largest bound / d2; exit 1 on a violation.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../lara_amd/csrc/boxbound.h"
#include "../lara_amd/csrc/tridist.h"

int main(int argc, char **argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: meshbvh_hostcheck <pairs.bin>\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "meshbvh_hostcheck: cannot open %s\n", argv[1]); return 2; }
    int64_t n = 0;
    if (std::fread(&n, sizeof n, 1, f) != 1 || n < 0 || n > (1ll << 28)) { std::fclose(f); return 2; }
    std::vector<float> rows((size_t)n * 18);
    const size_t got = std::fread(rows.data(), sizeof(float), rows.size(), f);
    std::fclose(f);
    if (got != rows.size()) { std::fprintf(stderr, "meshbvh_hostcheck: short file\n"); return 2; }
    int64_t above = 0, not_finite = 0, empty_wrong = 0;
    double worst = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        const float *r = rows.data() + 18 * (size_t)i;
        double c[3];
        const double d2 = lara_tridist(r, r + 3, r + 6, r + 9, c);
        const double b = lara_boxbound(r, r + 12, r + 15);
        if (!(b <= d2)) ++above;
        if (!std::isfinite(d2) || !std::isfinite(b) || !std::isfinite(c[0]) || !std::isfinite(c[1]) || !std::isfinite(c[2])) ++not_finite;
        if (d2 > 0.0 && b / d2 > worst) worst = b / d2;
        const float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        if (!(lara_boxbound(r, lo, hi) == INFINITY)) ++empty_wrong;
    }
    std::printf("pairs %lld, bound above d2 %lld, results not finite %lld, empty box not +inf %lld, largest bound / d2 %.12f\n",
                (long long)n, (long long)above, (long long)not_finite, (long long)empty_wrong, worst);
    return above || not_finite || empty_wrong ? 1 : 0;
}
