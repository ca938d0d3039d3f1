// meshtexture_hostcheck.cpp -- csrc/texatlas.h as plain host C++ over the cases of tests/meshtexture_cases.py, for a build with
// -fsanitize=address,undefined (tools/meshtexture_hostcheck.py writes the records, compiles this file and runs it; nothing here
// touches a device or is loaded into python).
//   meshtexture_hostcheck <records.bin>    int64 cases, and per case a run of blocks, each int64 n followed by n elements:
//       i32 {S, C, T, Nv, V, H, W}, f32 vertices, i32 triangles, f32 images, f32 k, f32 w2c, f32 eyes, f32 colours, i64 mask,
//       i32 face, f32 point, f32 anchor (the restatement's texels), i32 variants, and per variant
//       f32 {near, min_cos, power, two_sided, best, use mask, use colours, fill r, g, b}, u8 texture, f32 weight, i32 view;
//       then i32 sample faces, f32 barycentrics, f32 RGBA (the restatement's samples of the last variant's texture)
// Every output is written into a vector of its exact size and compared with the restatement's as bytes; prints the counts, exit 1 on a
// difference.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../lara_amd/csrc/texatlas.h"

template <class T>
static bool block(std::FILE *f, std::vector<T> &v) {
    int64_t n = 0;
    if (std::fread(&n, sizeof n, 1, f) != 1 || n < 0 || n > (1ll << 28)) return false;
    v.resize((size_t)n);
    return n == 0 || std::fread(v.data(), sizeof(T), (size_t)n, f) == (size_t)n;
}

template <class T>
static int64_t differ(const std::vector<T> &a, const std::vector<T> &b) {
    if (a.size() != b.size()) return (int64_t)(a.size() > b.size() ? a.size() : b.size());
    int64_t n = 0;
    for (size_t i = 0; i < a.size(); ++i) n += std::memcmp(&a[i], &b[i], sizeof(T)) != 0;
    return n;
}

int main(int argc, char **argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: meshtexture_hostcheck <records.bin>\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "meshtexture_hostcheck: cannot open %s\n", argv[1]); return 2; }
    int64_t cases = 0, texels = 0, bakes = 0, samples = 0, bad = 0;
    if (std::fread(&cases, sizeof cases, 1, f) != 1 || cases < 0 || cases > 1024) { std::fclose(f); return 2; }
    for (int64_t c = 0; c < cases; ++c) {
        std::vector<int32_t> dims, tri, face_want, n_variants, sample_face;
        std::vector<float> vert, images, k, w2c, eyes, colours, point_want, anchor_want, bary, rgba_want;
        std::vector<int64_t> mask;
        bool ok = block(f, dims) && dims.size() == 7 && block(f, vert) && block(f, tri) && block(f, images) && block(f, k) && block(f, w2c) &&
                  block(f, eyes) && block(f, colours) && block(f, mask) && block(f, face_want) && block(f, point_want) && block(f, anchor_want) &&
                  block(f, n_variants) && n_variants.size() == 1;
        if (!ok) { std::fprintf(stderr, "meshtexture_hostcheck: short file\n"); std::fclose(f); return 2; }
        const LaraTexAtlas L = lara_texatlas_make(dims[0], dims[1], dims[2]);
        const int64_t n = L.Wa * L.Ha;
        std::vector<int32_t> face((size_t)n);
        std::vector<float> point((size_t)n * 3), anchor((size_t)n * 3);
        for (int64_t i = 0; i < n; ++i) lara_texatlas_texel(L, dims[3], vert.data(), tri.data(), i, face.data(), point.data(), anchor.data());
        bad += differ(face, face_want) + differ(point, point_want) + differ(anchor, anchor_want);
        texels += n;
        std::vector<uint8_t> texture((size_t)n * 4);
        for (int32_t v = 0; v < n_variants[0]; ++v) {
            std::vector<float> p, weight_want;
            std::vector<uint8_t> texture_want;
            std::vector<int32_t> view_want;
            if (!(block(f, p) && p.size() == 10 && block(f, texture_want) && block(f, weight_want) && block(f, view_want))) {
                std::fprintf(stderr, "meshtexture_hostcheck: short file\n");
                std::fclose(f);
                return 2;
            }
            std::vector<float> weight((size_t)n);
            std::vector<int32_t> view((size_t)n);
            LaraTexBake B;
            B.L = L; B.Nv = dims[3]; B.V = dims[4]; B.H = dims[5]; B.W = dims[6];
            B.near = (double)p[0]; B.min_cos = (double)p[1]; B.power = (int32_t)p[2]; B.two_sided = (int32_t)p[3]; B.best = (int32_t)p[4];
            B.fill[0] = p[7]; B.fill[1] = p[8]; B.fill[2] = p[9];
            B.vertices = vert.data(); B.images = images.data(); B.k = k.data(); B.w2c = w2c.data(); B.eyes = eyes.data();
            B.vertex_colors = p[6] != 0.0f ? colours.data() : nullptr;
            B.point = point.data(); B.anchor = anchor.data(); B.triangles = tri.data(); B.face = face.data();
            B.mask = p[5] != 0.0f ? mask.data() : nullptr;
            B.texture = texture.data(); B.weight = weight.data(); B.view = view.data();
            for (int64_t i = 0; i < n; ++i) lara_texatlas_bake_texel(B, i);
            bad += differ(texture, texture_want) + differ(weight, weight_want) + differ(view, view_want);
            bakes += n;
        }
        if (!(block(f, sample_face) && block(f, bary) && block(f, rgba_want) && bary.size() == 3 * sample_face.size())) {
            std::fprintf(stderr, "meshtexture_hostcheck: short file\n");
            std::fclose(f);
            return 2;
        }
        std::vector<float> rgba(sample_face.size() * 4);
        const float bg[3] = {0.1f, 0.2f, 0.3f};
        for (int64_t i = 0; i < (int64_t)sample_face.size(); ++i)
            lara_texatlas_sample(L, texture.data(), sample_face.data(), bary.data(), 4, bg, i, rgba.data());
        bad += differ(rgba, rgba_want);
        samples += (int64_t)sample_face.size();
    }
    std::fclose(f);
    std::printf("cases %lld, texels %lld, baked texels %lld, samples %lld; elements that differ from the restatement: %lld\n", (long long)cases,
                (long long)texels, (long long)bakes, (long long)samples, (long long)bad);
    return bad ? 1 : 0;
}
