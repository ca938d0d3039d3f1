// meshio_exhaustive.cpp -- lara_fmt9g (lara_amd/csrc/fmt9g.h) against the C library's snprintf("%.9g", (double)v) over fp32 bit
// patterns; a stand-alone host program, compiled from fmt9g.h alone:
//     g++ -O2 -std=c++17 -pthread tools/meshio_exhaustive.cpp -o meshio_exhaustive
//     ./meshio_exhaustive [--threads N] [--stride S]
// Without --stride: all 2^32 patterns.  With it: every S-th pattern plus the special values (powers of two, the floats around every
// power of ten, the notation switches, ties), the run for a build with -fsanitize=address,undefined.  A NaN is compared with "nan"
// whatever its sign (glibc prints "-nan" for a negative one).  It also checks that nothing is written beyond the returned length,
// that lara_fmt9g_len agrees, and that the multiplication never carries out of its limbs.  Prints the first mismatches and one
// result line; the exit status is 0 only without a mismatch.
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

static std::atomic<long long> g_overflow{0};
#define LARA_FMT9G_CHECK g_overflow.fetch_add(1)
#include "../lara_amd/csrc/fmt9g.h"

static std::mutex g_print;
static std::atomic<long long> g_bad{0}, g_done{0};
static std::atomic<int> g_longest{0};

static void check(uint32_t bits) {
    float v;
    memcpy(&v, &bits, 4);
    char want[40], got[24];
    if (std::isnan(v))
        strcpy(want, "nan");
    else
        snprintf(want, sizeof want, "%.9g", (double)v);
    memset(got, 0x7f, sizeof got);
    const int n = lara_fmt9g(v, got);
    const int wn = (int)strlen(want);
    bool ok = n == wn && memcmp(got, want, (size_t)wn) == 0 && lara_fmt9g_len(lara_fmt9g_decompose(v)) == n;
    for (int i = n < 0 ? 0 : n; ok && i < (int)sizeof got; ++i) ok = got[i] == 0x7f;
    int prev = g_longest.load();
    while (n > prev && !g_longest.compare_exchange_weak(prev, n)) {
    }
    if (!ok && g_bad.fetch_add(1) < 20) {
        std::lock_guard<std::mutex> lock(g_print);
        printf("mismatch 0x%08x: want %s, got %.*s (length %d)\n", bits, want, n > 0 && n < 24 ? n : 0, got, n);
    }
}

static std::vector<uint32_t> specials() {
    std::vector<uint32_t> s = {0u, 0x80000000u, 1u, 0x007fffffu, 0x00800000u, 0x7f7fffffu, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u,
                               0x7f800001u, 0xffffffffu, 0x4e6e6b28u /* 1e9 */, 0x4e6e6b27u /* 999999936 */};
    auto around = [&](double x) {
        float f = (float)x;
        uint32_t b;
        memcpy(&b, &f, 4);
        for (int d = -2; d <= 2; ++d) s.push_back(b + (uint32_t)d), s.push_back((b + (uint32_t)d) | 0x80000000u);
    };
    for (int e = -149; e <= 127; ++e) around(std::ldexp(1.0, e));
    for (int k = -45; k <= 38; ++k) around(std::pow(10.0, k));
    around(1e-4), around(9.9999e-5), around(123456.789), around(0.000123456789);
    for (uint32_t i = 0; i < 4000; ++i) {      // exact ties m / 8 with a 7-digit integer part
        const float f = (float)(1000000u + 2243u * i) + (i & 1u ? 0.125f : 0.875f) + (i & 2u ? 0.25f : 0.0f);
        uint32_t b;
        memcpy(&b, &f, 4);
        s.push_back(b);
    }
    return s;
}

int main(int argc, char **argv) {
    int threads = (int)std::thread::hardware_concurrency();
    unsigned long long stride = 1;
    for (int i = 1; i + 1 < argc; i += 2) {
        if (!strcmp(argv[i], "--threads")) threads = atoi(argv[i + 1]);
        if (!strcmp(argv[i], "--stride")) stride = strtoull(argv[i + 1], nullptr, 10);
    }
    if (threads < 1) threads = 1;
    if (stride < 1) stride = 1;
    const unsigned long long total = (0x100000000ull + stride - 1) / stride;
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; ++t)
        pool.emplace_back([=] {
            long long n = 0;
            for (unsigned long long j = (unsigned long long)t; j < total; j += (unsigned long long)threads, ++n) check((uint32_t)(j * stride));
            g_done += n;
        });
    for (auto &th : pool) th.join();
    long long extra = 0;
    if (stride > 1) {
        for (uint32_t b : specials()) check(b), ++extra;
    }
    printf("meshio_exhaustive: %lld patterns (stride %llu, %lld special values), %lld mismatches, %lld limb overflows, longest token %d\n",
           g_done.load() + extra, stride, extra, g_bad.load(), g_overflow.load(), g_longest.load());
    return g_bad.load() == 0 && g_overflow.load() == 0 ? 0 : 1;
}
