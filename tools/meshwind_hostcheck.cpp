// meshwind_hostcheck.cpp -- csrc/solidangle.h and the two host entries' loops (csrc/meshwind_host.h) as plain host C++, over the
// (point, triangle) groups of tests/test_meshwind.py and the brute-force cases of tests/meshwind_cases.py, for a build with
// -fsanitize=address,undefined (tools/meshwind_hostcheck.py writes the records, compiles this file and runs it; nothing here
// touches a device or is loaded into python).
//   meshwind_hostcheck <records.bin>     int64 n, n x 12 fp32 (q[3], p0[3], p1[3], p2[3]), n f64 (the float64 restatement's Omega);
//                                        then int64 cases, and per case: int64 N, int64 T, N x 3 fp32 points, T x 9 fp32 triangles,
//                                        N f64 (restated w; NaN: the point is not finite), N f64 (the summation bar on w)
// Prints the pairs, the exact zeros, the worst error of a term in ulp of the restated one (at most 4), the cases, their points and
// the worst ratio of |w - restated w| to its bar (at most 1); exit 1 on a violation.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../lara_amd/csrc/meshwind_host.h"

template <class T>
static bool read_all(std::FILE *f, std::vector<T> &v, const size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char **argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: meshwind_hostcheck <records.bin>\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "meshwind_hostcheck: cannot open %s\n", argv[1]); return 2; }
    int64_t n = 0;
    std::vector<float> rows;
    std::vector<double> want;
    if (std::fread(&n, sizeof n, 1, f) != 1 || n < 0 || n > (1ll << 26) || !read_all(f, rows, (size_t)n * 12) || !read_all(f, want, (size_t)n)) {
        std::fprintf(stderr, "meshwind_hostcheck: short file\n");
        std::fclose(f);
        return 2;
    }
    std::vector<float> q((size_t)n * 3), tri((size_t)n * 9);
    for (int64_t i = 0; i < n; ++i) {
        for (int k = 0; k < 3; ++k) q[3 * (size_t)i + k] = rows[12 * (size_t)i + k];
        for (int k = 0; k < 9; ++k) tri[9 * (size_t)i + k] = rows[12 * (size_t)i + 3 + k];
    }
    std::vector<double> omega((size_t)n);
    lara_meshwind_solid_loop(n, q.data(), tri.data(), omega.data());
    int64_t zeros = 0, bad_zero = 0, bad_term = 0;
    double worst_ulp = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        if (want[i] == 0.0) {
            ++zeros;
            if (omega[i] != 0.0 || std::signbit(omega[i])) ++bad_zero;
            continue;
        }
        const double a = std::fabs(want[i]), ulp = std::nextafter(a, INFINITY) - a;
        const double e = std::fabs(omega[i] - want[i]) / ulp;
        if (!(e <= 4.0)) ++bad_term;
        if (e > worst_ulp) worst_ulp = e;
    }
    int64_t cases = 0, points = 0, bad_w = 0;
    double worst_ratio = 0.0;
    if (std::fread(&cases, sizeof cases, 1, f) != 1 || cases < 0 || cases > 1024) { std::fclose(f); return 2; }
    for (int64_t c = 0; c < cases; ++c) {
        int64_t N = 0, T = 0;
        std::vector<float> P, tr;
        std::vector<double> w_want, bar;
        if (std::fread(&N, sizeof N, 1, f) != 1 || std::fread(&T, sizeof T, 1, f) != 1 || N < 0 || T < 0 || N > (1 << 20) || T > (1 << 20) ||
            !read_all(f, P, (size_t)N * 3) || !read_all(f, tr, (size_t)T * 9) || !read_all(f, w_want, (size_t)N) || !read_all(f, bar, (size_t)N)) {
            std::fprintf(stderr, "meshwind_hostcheck: short file\n");
            std::fclose(f);
            return 2;
        }
        std::vector<double> w((size_t)N);
        lara_meshwind_brute_loop(N, P.data(), T, tr.data(), w.data());
        for (int64_t i = 0; i < N; ++i) {
            if (std::isnan(w_want[i]) || std::isnan(w[i])) {
                if (std::isnan(w_want[i]) != std::isnan(w[i])) ++bad_w;
                continue;
            }
            const double e = std::fabs(w[i] - w_want[i]);
            if (!(e <= bar[i])) ++bad_w;
            if (bar[i] > 0.0 && e / bar[i] > worst_ratio) worst_ratio = e / bar[i];
        }
        points += N;
    }
    std::fclose(f);
    std::printf("pairs %lld, exact zeros %lld (violated %lld), worst term error %.2f ulp (beyond 4 ulp: %lld); brute force: cases %lld, "
                "points %lld, worst ratio to the bar %.3f (beyond it or a NaN misplaced: %lld)\n", (long long)n, (long long)zeros,
                (long long)bad_zero, worst_ulp, (long long)bad_term, (long long)cases, (long long)points, worst_ratio, (long long)bad_w);
    return bad_zero || bad_term || bad_w ? 1 : 0;
}
