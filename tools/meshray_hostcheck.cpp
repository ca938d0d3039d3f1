// meshray_hostcheck.cpp -- csrc/raytri.h and csrc/raybox.h as plain host C++, over the (ray, triangle, box) groups of
// tests/meshray_cases.bound_groups, for a build with -fsanitize=address,undefined (tools/meshray_hostcheck.py writes the groups,
// compiles this file and runs it; nothing here touches a device or is loaded into python).
//   meshray_hostcheck <groups.bin>     groups.bin: int64 n, then n records of 23 fp32: o[3], d[3], t_min, t_max, p0[3], p1[3], p2[3], lo[3], hi[3]
// Prints the groups read, the hits, those with an entry that is not finite or above t (must be 0), hits with a result that is not
// finite or weights that do not sum to 1 (must be 0), empty boxes not +inf (must be 0) and the smallest (t - entry) / |t|; exit 1 on
// a violation.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../lara_amd/csrc/raytri.h"
#include "../lara_amd/csrc/raybox.h"

int main(int argc, char **argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: meshray_hostcheck <groups.bin>\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "meshray_hostcheck: cannot open %s\n", argv[1]); return 2; }
    int64_t n = 0;
    if (std::fread(&n, sizeof n, 1, f) != 1 || n < 0 || n > (1ll << 28)) { std::fclose(f); return 2; }
    std::vector<float> rows((size_t)n * 23);
    const size_t got = std::fread(rows.data(), sizeof(float), rows.size(), f);
    std::fclose(f);
    if (got != rows.size()) { std::fprintf(stderr, "meshray_hostcheck: short file\n"); return 2; }
    int64_t hits = 0, above = 0, not_finite = 0, empty_wrong = 0;
    double closest = INFINITY;
    for (int64_t i = 0; i < n; ++i) {
        const float *r = rows.data() + 23 * (size_t)i;
        const LaraRay ray = lara_ray_setup(r, r + 3);
        const double t_min = (double)r[6], t_max = (double)r[7];
        double t = 0.0, b[3] = {0.0, 0.0, 0.0};
        const double entry = lara_raybox(ray, r + 17, r + 20, t_min, t_max);
        const float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        if (!(lara_raybox(ray, lo, hi, t_min, t_max) == INFINITY)) ++empty_wrong;
        if (!lara_raytri(ray, t_min, t_max, r + 8, r + 11, r + 14, t, b)) continue;
        ++hits;
        if (!std::isfinite(entry) || !(entry <= t)) ++above;
        if (!std::isfinite(t) || !(std::fabs((b[0] + b[1]) + b[2] - 1.0) < 1e-9)) ++not_finite;
        const double gap = (t - entry) / (std::fabs(t) > 0.0 ? std::fabs(t) : 1.0);
        if (gap < closest) closest = gap;
    }
    std::printf("groups %lld, hits %lld, entry not finite or above t %lld, results not finite %lld, empty box not +inf %lld, "
                "smallest (t - entry) / |t| %.3e\n", (long long)n, (long long)hits, (long long)above, (long long)not_finite,
                (long long)empty_wrong, closest);
    return above || not_finite || empty_wrong ? 1 : 0;
}
