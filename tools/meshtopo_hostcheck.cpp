// meshtopo_hostcheck.cpp -- csrc/meshtopo_ops.h as plain host C++, over the meshes of tests/meshtopo_cases.py, for a build with
// -fsanitize=address,undefined (tools/meshtopo_hostcheck.py writes the cases with the float64 restatement's answers, compiles this
// file and runs it; nothing here touches a device or is loaded into python).
//   meshtopo_hostcheck <cases.bin>     int64 cases, then per case: int64 Nv, T, n_neighbors, n_faces; vertices [Nv][3] f32; triangles
//                                      [T][3] i32; neighbour offsets [Nv + 1] i64 and neighbours [n_neighbors] i32; face offsets
//                                      [Nv + 1] i64 and faces [n_faces][2] i32; fixed [Nv] i32; the expected normals for the two
//                                      weightings, [Nv][3] f32 each, and their zero counts, int64 each; the steps lam, mu as f64; the
//                                      expected positions after one pass with lam, with mu, and both again with `fixed`, [Nv][3] f32 each
// Every array is copied into a heap block of exactly its size, so that a read beyond a row is the sanitizer's to report.  Prints the
// cases, vertices and rows walked and the words that differ from the restatement's bits (must be 0); exit 1 on a difference.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../lara_amd/csrc/meshtopo_ops.h"

template <class T>
static bool take(std::FILE *f, std::vector<T> &v, const size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

static int64_t differing(const std::vector<float> &a, const std::vector<float> &b) {
    int64_t bad = 0;
    for (size_t i = 0; i < a.size(); ++i) bad += std::memcmp(&a[i], &b[i], sizeof(float)) != 0;
    return bad;
}

int main(int argc, char **argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: meshtopo_hostcheck <cases.bin>\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "meshtopo_hostcheck: cannot open %s\n", argv[1]); return 2; }
    int64_t cases = 0;
    if (std::fread(&cases, sizeof cases, 1, f) != 1 || cases < 0 || cases > 4096) { std::fclose(f); return 2; }
    int64_t vertices = 0, face_rows = 0, neighbor_rows = 0, bad_normals = 0, bad_counts = 0, bad_positions = 0;
    for (int64_t c = 0; c < cases; ++c) {
        int64_t h[4];
        if (std::fread(h, sizeof(int64_t), 4, f) != 4) { std::fclose(f); return 2; }
        const int64_t Nv = h[0], T = h[1], nn = h[2], nf = h[3];
        if (Nv < 0 || T < 0 || nn < 0 || nf < 0 || Nv > (1 << 24) || T > (1 << 24)) { std::fclose(f); return 2; }
        std::vector<float> V, want_n[2], want_x[4];
        std::vector<int32_t> F, nb, fc, fixed;
        std::vector<int64_t> no, fo;
        int64_t want_zero[2];
        double s[2];
        bool ok = take(f, V, 3 * Nv) && take(f, F, 3 * T) && take(f, no, Nv + 1) && take(f, nb, nn) && take(f, fo, Nv + 1) &&
                  take(f, fc, 2 * nf) && take(f, fixed, Nv) && take(f, want_n[0], 3 * Nv) && take(f, want_n[1], 3 * Nv) &&
                  std::fread(want_zero, sizeof(int64_t), 2, f) == 2 && std::fread(s, sizeof(double), 2, f) == 2;
        for (int k = 0; ok && k < 4; ++k) ok = take(f, want_x[k], 3 * Nv);
        if (!ok || no[Nv] != nn || fo[Nv] != nf) { std::fprintf(stderr, "meshtopo_hostcheck: short or inconsistent case %lld\n", (long long)c); std::fclose(f); return 2; }
        for (int w = 0; w < 2; ++w) {
            std::vector<float> got(3 * Nv);
            int64_t zero = 0;
            for (int64_t v = 0; v < Nv; ++v) zero += lara_meshtopo_normal(V.data(), F.data(), fc.data(), fo[v], fo[v + 1], w, got.data() + 3 * v);
            bad_normals += differing(got, want_n[w]);
            bad_counts += zero != want_zero[w];
        }
        for (int k = 0; k < 4; ++k) {
            std::vector<float> got(3 * Nv);
            for (int64_t v = 0; v < Nv; ++v)
                lara_meshtopo_smooth(V.data(), nb.data(), no[v], no[v + 1], s[k & 1], k >= 2 ? fixed[v] : 0, v, got.data() + 3 * v);
            bad_positions += differing(got, want_x[k]);
        }
        vertices += Nv;
        face_rows += nf;
        neighbor_rows += nn;
    }
    std::fclose(f);
    std::printf("cases %lld, vertices %lld, face entries %lld, neighbour entries %lld, normal words off the restatement %lld, zero counts "
                "off %lld, position words off %lld\n", (long long)cases, (long long)vertices, (long long)face_rows, (long long)neighbor_rows,
                (long long)bad_normals, (long long)bad_counts, (long long)bad_positions);
    return bad_normals || bad_counts || bad_positions ? 1 : 0;
}
