// batchfinish_hostcheck.cpp -- csrc/batchfinish_ops.h (the per-pixel function and the host entry's loop) as plain host C++, over the
// raw batches of tests/batchfinish_cases.py, for a build with -fsanitize=address,undefined (tools/batchfinish_hostcheck.py writes the
// cases with the numpy float32 restatement's answers, compiles this file and runs it; nothing here touches a device or is loaded into
// python).
//   batchfinish_hostcheck <cases.bin>   int64 cases, then per case: int64 B, V, H, W, has_normals; rgba u8 [B][V][H][W][4]; bg f32
//                                       [B][V][3]; with normals: n_u8 u8 [B][V][H][W][3], rot f32 [B][3][3]; the expected rgb f32
//                                       [B][V][H][W][3], msk u8 [B][V][H][W] and, with normals, nrm f32 [B][H][V W][3]
// Every array is copied into a heap block of exactly its size, so that a read or write beyond it is the sanitizer's to report; the
// outputs start as a sentinel.  Prints the cases and pixels walked and the words that differ from the restatement's (must be 0);
// exit 1 on a difference.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../lara_amd/csrc/batchfinish_ops.h"

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
    if (argc != 2) { std::fprintf(stderr, "usage: batchfinish_hostcheck <cases.bin>\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "batchfinish_hostcheck: cannot open %s\n", argv[1]); return 2; }
    int64_t cases = 0;
    if (std::fread(&cases, sizeof cases, 1, f) != 1 || cases < 0 || cases > 4096) { std::fclose(f); return 2; }
    int64_t pixels = 0, bad = 0;
    for (int64_t c = 0; c < cases; ++c) {
        int64_t h[5];
        if (std::fread(h, sizeof(int64_t), 5, f) != 5) { std::fclose(f); return 2; }
        const int64_t B = h[0], V = h[1], H = h[2], W = h[3];
        const bool normals = h[4] != 0;
        if (B < 0 || V < 0 || H < 0 || W < 0 || B > 4096 || V > 4096 || H > 4096 || W > 4096 || B * V * H * W > (1 << 24)) { std::fclose(f); return 2; }
        const size_t n = (size_t)(B * V * H * W);
        std::vector<uint8_t> rgba, n_u8, want_msk;
        std::vector<float> bg, rot, want_rgb, want_nrm;
        bool ok = take(f, rgba, 4 * n) && take(f, bg, (size_t)(3 * B * V));
        if (normals) ok = ok && take(f, n_u8, 3 * n) && take(f, rot, (size_t)(9 * B));
        ok = ok && take(f, want_rgb, 3 * n) && take(f, want_msk, n);
        if (normals) ok = ok && take(f, want_nrm, 3 * n);
        if (!ok) { std::fprintf(stderr, "batchfinish_hostcheck: short case %lld\n", (long long)c); std::fclose(f); return 2; }
        std::vector<float> rgb(3 * n, -12345.0f), nrm(normals ? 3 * n : 0, -12345.0f);
        std::vector<uint8_t> msk(n, 0xEE);
        lara_batchfinish_host_pixels(rgba.data(), bg.data(), normals ? n_u8.data() : nullptr, normals ? rot.data() : nullptr, B, V, H, W,
                                     rgb.data(), msk.data(), normals ? nrm.data() : nullptr);
        bad += differing(rgb, want_rgb) + differing(msk, want_msk) + differing(nrm, want_nrm);
        pixels += (int64_t)n;
    }
    std::fclose(f);
    std::printf("cases %lld, pixels %lld, words off the restatement %lld\n", (long long)cases, (long long)pixels, (long long)bad);
    return bad ? 1 : 0;
}
