// splatxform_hostcheck.cpp -- csrc/splatxform_ops.h (the per-surfel function and the host entry's loop) as plain host C++, over the
// clouds of tests/splatxform_cases.py, for a build with -fsanitize=address,undefined (tools/splatxform_hostcheck.py writes the cases
// with the float64 restatement's answers, compiles this file and runs it; nothing here touches a device or is loaded into python).
//   splatxform_hostcheck <cases.bin>   int64 cases, then per case: int64 degree, P, out_row0, out_rows; the plan, 100 f64; centers
//                                      [P][3], shs [P][n][3], opacity [P], scales [P][2], rotations [P][4] as f32; the expected five
//                                      arrays in the same order and shapes
// Every array is copied into a heap block of exactly its size, so that a read or write beyond a row is the sanitizer's to report.
// Each case runs twice: into fresh outputs of out_rows rows filled with a sentinel (rows outside [out_row0, out_row0 + P) must keep
// it), and in place.  Prints the cases and rows walked and the words that differ from the restatement's bits (must be 0); exit 1 on a
// difference.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../lara_amd/csrc/splatxform_ops.h"

static const uint32_t SENTINEL = 0xDEADBEEFu;

static bool take(std::FILE *f, std::vector<float> &v, const size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(float), n, f) == n;
}

static int64_t differing(const float *a, const float *b, const size_t n) {
    int64_t bad = 0;
    for (size_t i = 0; i < n; ++i) bad += std::memcmp(a + i, b + i, sizeof(float)) != 0;
    return bad;
}

static int64_t not_sentinel(const float *a, const size_t n) {
    int64_t bad = 0;
    for (size_t i = 0; i < n; ++i) bad += std::memcmp(a + i, &SENTINEL, sizeof(float)) != 0;
    return bad;
}

int main(int argc, char **argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: splatxform_hostcheck <cases.bin>\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "splatxform_hostcheck: cannot open %s\n", argv[1]); return 2; }
    int64_t cases = 0;
    if (std::fread(&cases, sizeof cases, 1, f) != 1 || cases < 0 || cases > 4096) { std::fclose(f); return 2; }
    int64_t rows = 0, bad = 0, touched = 0;
    for (int64_t c = 0; c < cases; ++c) {
        int64_t h[4];
        if (std::fread(h, sizeof(int64_t), 4, f) != 4) { std::fclose(f); return 2; }
        const int64_t degree = h[0], P = h[1], row0 = h[2], out_rows = h[3];
        if (degree < 0 || degree > 3 || P < 0 || P > (1 << 24) || row0 < 0 || out_rows > (1 << 24) || row0 + P > out_rows) { std::fclose(f); return 2; }
        const size_t width[5] = {3, (size_t)(3 * (degree + 1) * (degree + 1)), 1, 2, 4};
        std::vector<double> plan(100);
        std::vector<float> in[5], want[5];
        bool ok = std::fread(plan.data(), sizeof(double), 100, f) == 100;
        for (int k = 0; ok && k < 5; ++k) ok = take(f, in[k], width[k] * P);
        for (int k = 0; ok && k < 5; ++k) ok = take(f, want[k], width[k] * P);
        if (!ok) { std::fprintf(stderr, "splatxform_hostcheck: short case %lld\n", (long long)c); std::fclose(f); return 2; }
        std::vector<float> out[5];
        for (int k = 0; k < 5; ++k) {
            out[k].resize(width[k] * out_rows);
            for (float &w : out[k]) std::memcpy(&w, &SENTINEL, sizeof w);
        }
        lara_splatxform_host_rows(plan.data(), (int)degree, P, in[0].data(), in[1].data(), in[2].data(), in[3].data(), in[4].data(),
                                  out[0].data(), out[1].data(), out[2].data(), out[3].data(), out[4].data(), row0);
        for (int k = 0; k < 5; ++k) {
            bad += differing(out[k].data() + width[k] * row0, want[k].data(), width[k] * P);
            touched += not_sentinel(out[k].data(), width[k] * row0);
            touched += not_sentinel(out[k].data() + width[k] * (row0 + P), width[k] * (out_rows - row0 - P));
        }
        lara_splatxform_host_rows(plan.data(), (int)degree, P, in[0].data(), in[1].data(), in[2].data(), in[3].data(), in[4].data(),
                                  in[0].data(), in[1].data(), in[2].data(), in[3].data(), in[4].data(), 0);
        for (int k = 0; k < 5; ++k) bad += differing(in[k].data(), want[k].data(), width[k] * P);
        rows += P;
    }
    std::fclose(f);
    std::printf("cases %lld, rows %lld (each into sentinel-filled outputs at its row offset and again in place), words off the restatement %lld, "
                "sentinel words touched %lld\n", (long long)cases, (long long)rows, (long long)bad, (long long)touched);
    return bad || touched ? 1 : 0;
}
