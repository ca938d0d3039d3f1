// splatpack_hostcheck.cpp -- csrc/splatpack_ops.h (the per-row functions and the host entries' loops) as plain host C++, over the cases of
// tests/splatpack_cases.py, for a build with -fsanitize=address,undefined (tools/splatpack_hostcheck.py writes the cases with the
// float64 restatement's answers, compiles this file and runs it; nothing here touches a device or is loaded into python).
//   splatpack_hostcheck <cases.bin>   int64 cases, then per case six int64: SH degree, P, P_out, 0, 0, 0; the plan, 2 f64; centers [P][3],
//     shs [P][n][3], opacity [P], scales [P][2], rotations [P][4] in f32; near [P] u8 (1: the alpha before its floor lies on a rounding
//     boundary, 2: the importance does); the expected valid [P] u8, box [6] f32, dropped i64, Morton keys [P] i64, importance keys [P] i64,
//     order [P_out] i64, chunks [C][18] f32, words [P_out][4] u32, sh [P_out][W] u8, the .splat order [P_out] i64, rows [P_out][8] u32,
//     and the two decoded clouds (five f32 arrays each, the second of SH degree 0).
// Every array is copied into a heap block of exactly its size, so that a read or write beyond it is the sanitizer's to report.
// Prints the cases and values walked, the values that differ from the restatement outside the rules (must be 0), the alpha bytes and
// importance keys that differ on a boundary, the fp32 words through exp / log beyond one spacing (must be 0) and how many of them differ
// at all; exit 1 on a difference outside the rules.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../lara_amd/csrc/splatpack_ops.h"

template <class T>
static bool take(std::FILE *f, std::vector<T> &v, const size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

template <class T>
static int64_t differing(const std::vector<T> &a, const std::vector<T> &b) {
    int64_t bad = a.size() != b.size();
    for (size_t i = 0; i < a.size() && i < b.size(); ++i) bad += std::memcmp(&a[i], &b[i], sizeof(T)) != 0;
    return bad;
}

static int64_t g_far = 0, g_off = 0, g_words = 0;

// fp32 words that went through exp or log: within one spacing of the restatement's
static void spaced(const float a, const float b) {
    g_words += 1;
    if (std::memcmp(&a, &b, sizeof a) == 0) return;
    g_off += 1;
    const double gap = std::fabs((double)a - (double)b);
    const double spacing = (double)std::nextafter(std::fabs(b), INFINITY) - (double)std::fabs(b);
    g_far += !(gap <= spacing);
}

int main(int argc, char **argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: splatpack_hostcheck <cases.bin>\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "splatpack_hostcheck: cannot open %s\n", argv[1]); return 2; }
    int64_t cases = 0;
    if (std::fread(&cases, sizeof cases, 1, f) != 1 || cases < 0 || cases > 4096) { std::fclose(f); return 2; }
    int64_t walked = 0, bad = 0, alpha_off = 0, keys_off = 0;
    for (int64_t c = 0; c < cases; ++c) {
        int64_t h[6];
        if (std::fread(h, sizeof(int64_t), 6, f) != 6) { std::fclose(f); return 2; }
        const int64_t degree = h[0], P = h[1], P_out = h[2];
        if (degree < 0 || degree > 3 || P < 0 || P > (1 << 24) || P_out < 0 || P_out > P) { std::fclose(f); return 2; }
        const int n = (int)((degree + 1) * (degree + 1)), W = 3 * (n - 1);
        const int64_t C = (P_out + LARA_SPLATPACK_ROWS - 1) / LARA_SPLATPACK_ROWS;
        std::vector<double> plan;
        std::vector<float> in[5], want_box, want_chunks, want_dec[5], want_sdec[5];
        std::vector<uint8_t> near, want_valid, want_sh;
        std::vector<int64_t> want_dropped, want_mk, want_ik, order, sorder;
        std::vector<uint32_t> want_words, want_rows;
        bool ok = take(f, plan, 2);
        for (int k = 0; ok && k < 5; ++k) ok = take(f, in[k], (size_t)(lara_surfel_width(k, (int)degree) * P));
        ok = ok && take(f, near, (size_t)P) && take(f, want_valid, (size_t)P) && take(f, want_box, 6) && take(f, want_dropped, 1) &&
             take(f, want_mk, (size_t)P) && take(f, want_ik, (size_t)P) && take(f, order, (size_t)P_out) &&
             take(f, want_chunks, (size_t)(C * LARA_SPLATPACK_RECORD)) && take(f, want_words, (size_t)(4 * P_out)) &&
             take(f, want_sh, (size_t)(W * P_out)) && take(f, sorder, (size_t)P_out) && take(f, want_rows, (size_t)(8 * P_out));
        for (int k = 0; ok && k < 5; ++k) ok = take(f, want_dec[k], (size_t)(lara_surfel_width(k, (int)degree) * P_out));
        for (int k = 0; ok && k < 5; ++k) ok = take(f, want_sdec[k], (size_t)(lara_surfel_width(k, 0) * P_out));
        if (!ok) { std::fprintf(stderr, "splatpack_hostcheck: short case %lld\n", (long long)c); std::fclose(f); return 2; }
        const float *ins[5];
        for (int k = 0; k < 5; ++k) ins[k] = in[k].data();

        std::vector<uint8_t> valid((size_t)P, 0xEE);
        std::vector<float> box(6, -12345.0f);
        std::vector<int64_t> dropped(1, -1), mk((size_t)P, -1), ik((size_t)P, -1);
        lara_splatpack_host_bounds((int)degree, P, ins, valid.data(), box.data(), dropped.data());
        lara_splatpack_host_morton_keys(P, ins[0], valid.data(), box.data(), mk.data());
        lara_splatpack_host_importance_keys(plan.data(), P, ins[2], ins[3], valid.data(), ik.data());
        bad += differing(valid, want_valid) + differing(box, want_box) + differing(dropped, want_dropped) + differing(mk, want_mk);
        for (int64_t s = 0; s < P; ++s) {
            if (ik[(size_t)s] == want_ik[(size_t)s]) continue;
            const int64_t d = (ik[(size_t)s] >> 31) - (want_ik[(size_t)s] >> 31);
            if ((near[(size_t)s] & 2) && (d == 1 || d == -1)) keys_off += 1; else bad += 1;
        }
        walked += 4 * P + 7;

        std::vector<float> chunks((size_t)(C * LARA_SPLATPACK_RECORD), -12345.0f);
        std::vector<uint32_t> words((size_t)(4 * P_out), 0xEEEEEEEEu), rows((size_t)(8 * P_out), 0xEEEEEEEEu);
        std::vector<uint8_t> sh((size_t)(W * P_out), 0xEE);
        lara_splatpack_host_encode(plan.data(), (int)degree, P, P_out, ins, order.data(), chunks.data(), words.data(), sh.data());
        lara_splatpack_host_splat_encode(plan.data(), (int)degree, P, P_out, ins, sorder.data(), rows.data());
        bad += differing(chunks, want_chunks) + differing(sh, want_sh);
        for (int64_t i = 0; i < P_out; ++i) {
            for (int k = 0; k < 3; ++k) bad += words[(size_t)(4 * i + k)] != want_words[(size_t)(4 * i + k)];
            const uint32_t a = words[(size_t)(4 * i + 3)], b = want_words[(size_t)(4 * i + 3)];
            bad += (a >> 8) != (b >> 8);
            int d = (int)(a & 255u) - (int)(b & 255u);
            if (d != 0) { if ((near[(size_t)order[(size_t)i]] & 1) && (d == 1 || d == -1)) alpha_off += 1; else bad += 1; }
            const uint32_t *r = rows.data() + 8 * i, *w = want_rows.data() + 8 * i;
            bad += (r[0] != w[0]) + (r[1] != w[1]) + (r[2] != w[2]) + (r[5] != w[5]) + (r[7] != w[7]) + ((r[6] & 0xFFFFFFu) != (w[6] & 0xFFFFFFu));
            d = (int)(r[6] >> 24) - (int)(w[6] >> 24);
            if (d != 0) { if ((near[(size_t)sorder[(size_t)i]] & 1) && (d == 1 || d == -1)) alpha_off += 1; else bad += 1; }
            for (int k = 3; k < 5; ++k) {
                float x, y;
                std::memcpy(&x, r + k, 4), std::memcpy(&y, w + k, 4);
                spaced(x, y);
            }
        }
        walked += (int64_t)(chunks.size() + words.size() + sh.size() + rows.size());

        // the decoders, on the restatement's own words
        std::vector<float> dec[5], sdec[5];
        float *outs[5], *souts[5];
        for (int k = 0; k < 5; ++k) {
            dec[k].assign(want_dec[k].size(), -12345.0f), sdec[k].assign(want_sdec[k].size(), -12345.0f);
            outs[k] = dec[k].data(), souts[k] = sdec[k].data();
        }
        lara_splatpack_host_decode((int)degree, P_out, want_chunks.data(), want_words.data(), want_sh.data(), outs);
        lara_splatpack_host_splat_decode(P_out, want_rows.data(), souts);
        for (int k = 0; k < 5; ++k) {
            for (size_t i = 0; i < dec[k].size(); ++i) spaced(dec[k][i], want_dec[k][i]);
            for (size_t i = 0; i < sdec[k].size(); ++i) spaced(sdec[k][i], want_sdec[k][i]);
            walked += (int64_t)(dec[k].size() + sdec[k].size());
        }
    }
    std::fclose(f);
    std::printf("cases %lld, values %lld, values off the restatement outside the rules %lld, alpha bytes one apart on a boundary %lld, importance "
                "keys one apart on a boundary %lld, fp32 words through exp, log or the decoders beyond one spacing %lld, that differ %lld of %lld\n",
                (long long)cases, (long long)walked, (long long)bad, (long long)alpha_off, (long long)keys_off, (long long)g_far, (long long)g_off,
                (long long)g_words);
    return bad || g_far ? 1 : 0;
}
