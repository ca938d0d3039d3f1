// splatadam_hostcheck.cpp -- csrc/splatadam_ops.h (the per-word function and the host entry's loop) as plain host C++, over the cases
// of tests/splatrefine_cases.py, for a build with -fsanitize=address,undefined (tools/splatadam_hostcheck.py writes the cases with the
// float64 restatement's answers, compiles this file and runs it; nothing here touches a device or is loaded into python).
//   splatadam_hostcheck <cases.bin>   int64 cases, then per case: int64 degree, P, zero_grads, has_visible, the expected skipped
//                                     count; the plan, 13 f64; the parameters, gradients, exp_avg and exp_avg_sq, each as centers
//                                     [P][3], shs [P][n][3], opacity [P], scales [P][2], rotations [P][4] in f32; visible, P bytes
//                                     (where has_visible); the expected twenty arrays in the same order and shapes
// Every array is copied into a heap block of exactly its size, so that a read or write beyond it is the sanitizer's to report.
// Prints the cases and words walked, the words that differ from the restatement's bits and the cases whose count differs (both
// must be 0); exit 1 on a difference.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../lara_amd/csrc/splatadam_ops.h"

static bool take(std::FILE *f, std::vector<float> &v, const size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(float), n, f) == n;
}

static int64_t differing(const float *a, const float *b, const size_t n) {
    int64_t bad = 0;
    for (size_t i = 0; i < n; ++i) bad += std::memcmp(a + i, b + i, sizeof(float)) != 0;
    return bad;
}

int main(int argc, char **argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: splatadam_hostcheck <cases.bin>\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "splatadam_hostcheck: cannot open %s\n", argv[1]); return 2; }
    int64_t cases = 0;
    if (std::fread(&cases, sizeof cases, 1, f) != 1 || cases < 0 || cases > 4096) { std::fclose(f); return 2; }
    int64_t walked = 0, bad = 0, miscounted = 0;
    for (int64_t c = 0; c < cases; ++c) {
        int64_t h[5];
        if (std::fread(h, sizeof(int64_t), 5, f) != 5) { std::fclose(f); return 2; }
        const int64_t degree = h[0], P = h[1], zero_grads = h[2], has_visible = h[3], want_skipped = h[4];
        if (degree < 0 || degree > 3 || P < 0 || P > (1 << 24)) { std::fclose(f); return 2; }
        std::vector<double> plan(13);
        std::vector<float> in[20], want[20];
        std::vector<uint8_t> visible((size_t)P);
        bool ok = std::fread(plan.data(), sizeof(double), 13, f) == 13;
        for (int k = 0; ok && k < 20; ++k) ok = take(f, in[k], (size_t)(lara_surfel_width(k % 5, (int)degree) * P));
        if (ok && has_visible && P) ok = std::fread(visible.data(), 1, (size_t)P, f) == (size_t)P;
        for (int k = 0; ok && k < 20; ++k) ok = take(f, want[k], in[k].size());
        if (!ok) { std::fprintf(stderr, "splatadam_hostcheck: short case %lld\n", (long long)c); std::fclose(f); return 2; }
        float *ptrs[20];
        for (int k = 0; k < 20; ++k) ptrs[k] = in[k].data();
        const int64_t skipped = lara_splatadam_host_words(plan.data(), (int)degree, P, ptrs, ptrs + 5, ptrs + 10, ptrs + 15,
                                                          has_visible ? visible.data() : nullptr, (int)zero_grads);
        miscounted += skipped != want_skipped;
        for (int k = 0; k < 20; ++k) {
            bad += differing(in[k].data(), want[k].data(), in[k].size());
            walked += (int64_t)in[k].size();
        }
    }
    std::fclose(f);
    std::printf("cases %lld, words %lld, words off the restatement %lld, cases with another skipped count %lld\n", (long long)cases,
                (long long)walked, (long long)bad, (long long)miscounted);
    return bad || miscounted ? 1 : 0;
}
