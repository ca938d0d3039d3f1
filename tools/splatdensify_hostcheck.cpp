// splatdensify_hostcheck.cpp -- csrc/splatdensify_ops.h (the per-row functions and the host entries' loops) as plain host C++, over the
// cases of tests/splatdensify_cases.py, for a build with -fsanitize=address,undefined (tools/splatdensify_hostcheck.py writes the cases
// with the float64 restatement's answers, compiles this file and runs it; nothing here touches a device or is loaded into python).
//   splatdensify_hostcheck <cases.bin>   int64 cases, then per case six int64: kind, a, P, b, c, 0
//     kind 0, an accumulation (a = V): grad_means2D [P][3] f32, radii [V][P] i32, grad_sum [P] f32, seen [P] i32, max_radius [P] i32;
//             the expected grad_sum, seen, max_radius
//     kind 1, a round (a = SH degree, b = P_out, c = survivors): the plan, 8 f64; the parameters, exp_avg and exp_avg_sq, each as
//             centers [P][3], shs [P][n][3], opacity [P], scales [P][2], rotations [P][4] in f32; grad_sum, seen, max_radius; noise
//             [P][N][2] f32; the expected action [P] u8, offset [3 P] i32, counts [5] i64, row_source [P_out] i32, row_child [P_out] u8
//             and the fifteen arrays of P_out rows
// Every array is copied into a heap block of exactly its size, so that a read or write beyond it is the sanitizer's to report.
// Prints the cases and values walked, the values that differ from the restatement (the centre words of split children aside; must be
// 0), those centre words that lie beyond one fp32 spacing (must be 0) and how many of them differ at all; exit 1 on a difference.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../lara_amd/csrc/splatdensify_ops.h"

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

int main(int argc, char **argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: splatdensify_hostcheck <cases.bin>\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "splatdensify_hostcheck: cannot open %s\n", argv[1]); return 2; }
    int64_t cases = 0;
    if (std::fread(&cases, sizeof cases, 1, f) != 1 || cases < 0 || cases > 4096) { std::fclose(f); return 2; }
    int64_t walked = 0, bad = 0, centre_words = 0, centre_off = 0, centre_far = 0;
    for (int64_t c = 0; c < cases; ++c) {
        int64_t h[6];
        if (std::fread(h, sizeof(int64_t), 6, f) != 6) { std::fclose(f); return 2; }
        const int64_t kind = h[0], P = h[2];
        if (P < 0 || P > (1 << 24)) { std::fclose(f); return 2; }
        std::vector<float> grad_sum, want_sum;
        std::vector<int32_t> seen, max_radius, want_seen, want_max;
        if (kind == 0) {
            const int64_t V = h[1];
            std::vector<float> grad;
            std::vector<int32_t> radii;
            bool ok = V >= 1 && V <= 64 && take(f, grad, (size_t)(3 * P)) && take(f, radii, (size_t)(V * P)) && take(f, grad_sum, (size_t)P) &&
                      take(f, seen, (size_t)P) && take(f, max_radius, (size_t)P) && take(f, want_sum, (size_t)P) && take(f, want_seen, (size_t)P) &&
                      take(f, want_max, (size_t)P);
            if (!ok) { std::fprintf(stderr, "splatdensify_hostcheck: short case %lld\n", (long long)c); std::fclose(f); return 2; }
            lara_splatdensify_host_accumulate(P, (int)V, grad.data(), radii.data(), grad_sum.data(), seen.data(), max_radius.data());
            bad += differing(grad_sum, want_sum) + differing(seen, want_seen) + differing(max_radius, want_max);
            walked += 3 * P;
            continue;
        }
        const int64_t degree = h[1], P_out = h[3], survivors = h[4];
        if (kind != 1 || degree < 0 || degree > 3 || P_out < 0 || P_out > 9 * P || survivors < 0 || survivors > P_out) { std::fclose(f); return 2; }
        std::vector<double> plan;
        std::vector<float> in[15], out[15], want[15], noise;
        std::vector<uint8_t> action, want_action, child, want_child;
        std::vector<int32_t> offset, want_offset, source, want_source;
        std::vector<int64_t> counts(5), want_counts;
        bool ok = take(f, plan, 8);
        const int n_split = ok ? lara_splatdensify_children(plan.data()) : 1;
        for (int k = 0; ok && k < 15; ++k) ok = take(f, in[k], (size_t)(lara_surfel_width(k % 5, (int)degree) * P));
        ok = ok && take(f, grad_sum, (size_t)P) && take(f, seen, (size_t)P) && take(f, max_radius, (size_t)P) && take(f, noise, (size_t)(P * n_split * 2));
        ok = ok && take(f, want_action, (size_t)P) && take(f, want_offset, (size_t)(3 * P)) && take(f, want_counts, 5) &&
             take(f, want_source, (size_t)P_out) && take(f, want_child, (size_t)P_out);
        for (int k = 0; ok && k < 15; ++k) ok = take(f, want[k], (size_t)(lara_surfel_width(k % 5, (int)degree) * P_out));
        if (!ok) { std::fprintf(stderr, "splatdensify_hostcheck: short case %lld\n", (long long)c); std::fclose(f); return 2; }
        action.assign((size_t)P, 0xEE);
        offset.assign((size_t)(3 * P), -1);
        lara_splatdensify_host_decide(plan.data(), P, in[2].data(), in[3].data(), grad_sum.data(), seen.data(), max_radius.data(), action.data(),
                                      offset.data(), counts.data());
        bad += differing(action, want_action) + differing(offset, want_offset) + differing(counts, want_counts);
        walked += 4 * P + 5;
        if (counts[4] != P_out || counts[0] + counts[1] != survivors) continue;      // (counted above; the rows would not fit the arrays)
        source.assign((size_t)P_out, -1);
        child.assign((size_t)P_out, 0xEE);
        const float *ins[15];
        float *outs[15];
        for (int k = 0; k < 15; ++k) {
            out[k].assign(want[k].size(), -12345.0f);
            ins[k] = in[k].data(), outs[k] = out[k].data();
        }
        lara_splatdensify_host_apply(plan.data(), (int)degree, P, P_out, survivors, action.data(), offset.data(), noise.data(), ins, outs,
                                     source.data(), child.data());
        bad += differing(source, want_source) + differing(child, want_child);
        walked += 2 * P_out;
        for (int k = 0; k < 15; ++k) {
            walked += (int64_t)out[k].size();
            if (k != 0) { bad += differing(out[k], want[k]); continue; }
            for (int64_t o = 0; o < P_out; ++o)
                for (int r = 0; r < 3; ++r) {
                    const float a = out[0][3 * o + r], b = want[0][3 * o + r];
                    const bool same = std::memcmp(&a, &b, sizeof a) == 0;
                    if (want_child[(size_t)o] == LARA_SPLATDENSIFY_NO_CHILD) { bad += !same; continue; }
                    centre_words += 1;
                    centre_off += !same;
                    const double gap = std::fabs((double)a - (double)b);
                    const double spacing = (double)std::nextafter(std::fabs(b), INFINITY) - (double)std::fabs(b);
                    centre_far += !(gap <= spacing);
                }
        }
    }
    std::fclose(f);
    std::printf("cases %lld, values %lld, values off the restatement %lld, centre words beyond one spacing %lld, split children's centre words "
                "that differ %lld of %lld\n", (long long)cases, (long long)walked, (long long)bad, (long long)centre_far, (long long)centre_off,
                (long long)centre_words);
    return bad || centre_far ? 1 : 0;
}
