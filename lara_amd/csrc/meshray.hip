// meshray.hip -- ray queries on the triangle hierarchy of meshbvh.hip on gfx950: the first triangle a ray meets, whether it meets
// any, and which of E eyes see a point.  The walk of bvhwalk.h over the buffer lara_meshbvh_build wrote (meshbvh_layout.h; its
// records: trimesh.h), with the ray-triangle function of raytri.h per record and the margined entry parameter of raybox.h per
// box.  Interface, the function, the bound's derivation and the tie rule in include/lara_meshray.h.
//
//   mr_cast_kernel<MASKED>        one thread per ray: the walk, then t, face and the barycentrics of the best record
//   mr_occluded_kernel            one thread per ray: the same walk, ended by the first accepted triangle
//   mr_visible_kernel             one thread per point: that walk once per eye, one 64-bit word of `seen` written by its owner
// No LDS, no atomics, no stack: the walk is index arithmetic over the implicit 8-ary tree.  Built with -ffp-contract=off.
#include "common.h"
#include "unigrid.h"
#include "raytri.h"
#include "raybox.h"
#include "bvhwalk.h"
#include "../../include/lara_meshray.h"

#include <cmath>

namespace {

constexpr int64_t MR_MAX_RAYS = 1ll << 30;

struct MrBest { double t; int id, pos; };

// The walk.  A slot is stepped over when it is empty, when the ray has no parameter of its window inside the inflated box, or when
// the entry parameter is strictly greater than the best t so far; at equality it is entered.  MASKED: of eight siblings the
// one at counter c is slot c ^ mask, mask = the signs of d (x -> bit 0, y -> bit 1, z -> bit 2, the order of the Morton code):
// roughly front to back.  Triangle `skip` is ignored (-1: none is).  ANY: ended by the first accepted triangle, and true then.
template <bool ANY, bool MASKED>
__device__ __forceinline__ bool mr_walk(MrBest &best, const LaraRay &ray, const double t_min, const double t_max, const int skip,
                                        const char *__restrict__ bvh) {
    const MbWalk w = mb_walk_open(bvh);
    if (!ray.ok || w.n_valid <= 0 || !w.ok) return false;
    const int mask = MASKED ? (ray.d[0] < 0.0 ? 1 : 0) | (ray.d[1] < 0.0 ? 2 : 0) | (ray.d[2] < 0.0 ? 4 : 0) : 0;
    return lara_bvhwalk(
        w.hdr->L, mask,
        [&](const int level, const int slot) LARA_BVHWALK_INLINE {
            float blo[3], bhi[3];
            mb_load_box((const float2 *)(bvh + w.hdr->L.box[level]), (size_t)slot, blo, bhi);
            const double entry = lara_raybox(ray, blo, bhi, t_min, t_max);
            return entry < (double)INFINITY && !(entry > best.t);
        },
        [&](const int leaf) LARA_BVHWALK_INLINE {
            return mb_leaf_records(w.rec, w.T, leaf, [&](const TriRec &m, const int r) LARA_BVHWALK_INLINE {
                double t, b[3];
                if (m.id == skip || !lara_raytri(ray, t_min, t_max, m.p[0], m.p[1], m.p[2], t, b)) return false;
                if (ANY) return true;
                if (t < best.t || (t == best.t && m.id < best.id)) { best.t = t; best.id = m.id; best.pos = r; }      // (Nearest's rule, on t)
                return false;
            });
        });
}

__device__ __forceinline__ LaraRay mr_ray(const float *__restrict__ o, const float *__restrict__ d, const size_t i) {
    const float of[3] = {o[3 * i], o[3 * i + 1], o[3 * i + 2]}, df[3] = {d[3 * i], d[3 * i + 1], d[3 * i + 2]};
    return lara_ray_setup(of, df);
}

template <bool MASKED>
__global__ void __launch_bounds__(256)
mr_cast_kernel(const int R, const float *__restrict__ o, const float *__restrict__ d, const float *__restrict__ t_min,
               const float *__restrict__ t_max, const char *__restrict__ bvh, float *__restrict__ t, int *__restrict__ face,
               float *__restrict__ bary) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= R) return;
    const LaraRay ray = mr_ray(o, d, (size_t)i);
    const double lo = t_min ? (double)t_min[i] : 0.0, hi = t_max ? (double)t_max[i] : (double)INFINITY;
    MrBest best{INFINITY, NEAREST_NONE, 0};
    mr_walk<false, MASKED>(best, ray, lo, hi, -1, bvh);
    const bool none = best.id == NEAREST_NONE;
    t[i] = none ? INFINITY : (float)best.t;
    face[i] = none ? -1 : best.id;
    if (!bary) return;
    double b[3] = {NAN, NAN, NAN};
    if (!none) {
        const MbHeader *hdr = (const MbHeader *)bvh;
        const TriRec m = tri_load((const float4 *)(bvh + hdr->L.rec), best.pos);
        double tt;
        lara_raytri(ray, lo, hi, m.p[0], m.p[1], m.p[2], tt, b);
    }
#pragma unroll
    for (int j = 0; j < 3; j++) bary[3 * (size_t)i + j] = (float)b[j];
}

__global__ void __launch_bounds__(256)
mr_occluded_kernel(const int R, const float *__restrict__ o, const float *__restrict__ d, const float *__restrict__ t_min,
                   const float *__restrict__ t_max, const char *__restrict__ bvh, unsigned char *__restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= R) return;
    const LaraRay ray = mr_ray(o, d, (size_t)i);
    const double lo = t_min ? (double)t_min[i] : 0.0, hi = t_max ? (double)t_max[i] : (double)INFINITY;
    MrBest best{INFINITY, NEAREST_NONE, 0};
    out[i] = mr_walk<true, true>(best, ray, lo, hi, -1, bvh) ? 1 : 0;
}

// bit e of seen[i]: no triangle but skip[i] meets the ray from eye e to point i within [0, t_hi] (d = fl32(p - eye), t = 1 at p)
__global__ void __launch_bounds__(256)
mr_visible_kernel(const int N, const float *__restrict__ p, const int *__restrict__ skip, const int E, const float *__restrict__ eyes,
                  const float t_hi, const char *__restrict__ bvh, long long *__restrict__ seen) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float pf[3] = {p[3 * (size_t)i], p[3 * (size_t)i + 1], p[3 * (size_t)i + 2]};
    const int ignore = skip ? skip[i] : -1;
    unsigned long long word = 0ull;
    if (tri_point_finite(pf)) {
        for (int e = 0; e < E; e++) {
            const float of[3] = {eyes[3 * e], eyes[3 * e + 1], eyes[3 * e + 2]};
            const float df[3] = {pf[0] - of[0], pf[1] - of[1], pf[2] - of[2]};
            const LaraRay ray = lara_ray_setup(of, df);
            MrBest best{INFINITY, NEAREST_NONE, 0};
            if (!mr_walk<true, true>(best, ray, 0.0, (double)t_hi, ignore, bvh)) word |= 1ull << e;
        }
    }
    seen[i] = (long long)word;
}

template <bool MASKED>
int mr_cast(int32_t R, const float *origins, const float *directions, const float *t_min, const float *t_max, const void *bvh,
            float *t, int32_t *face, float *bary, void *stream) {
    if (R < 0 || R >= MR_MAX_RAYS) return LARA2DGS_E_INVALID;
    if (R == 0) return LARA2DGS_OK;
    if (!origins || !directions || !bvh || !t || !face) return LARA2DGS_E_INVALID;
    L2D_LAUNCH_IN_SCOPE((hipStream_t)stream, mr_cast_kernel<MASKED>, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, R, origins,
                        directions, t_min, t_max, (const char *)bvh, t, face, bary);
    return LARA2DGS_OK;
}

}  // namespace

extern "C" {

int lara_meshray_cast(int32_t R, const float *origins, const float *directions, const float *t_min, const float *t_max,
                      const void *bvh, float *t, int32_t *face, float *bary, void *stream) {
    return mr_cast<LARA_MESHRAY_MASKED_ORDER != 0>(R, origins, directions, t_min, t_max, bvh, t, face, bary, stream);
}

int lara_meshray_cast_other_order(int32_t R, const float *origins, const float *directions, const float *t_min, const float *t_max,
                                  const void *bvh, float *t, int32_t *face, float *bary, void *stream) {
    return mr_cast<LARA_MESHRAY_MASKED_ORDER == 0>(R, origins, directions, t_min, t_max, bvh, t, face, bary, stream);
}

int lara_meshray_occluded(int32_t R, const float *origins, const float *directions, const float *t_min, const float *t_max,
                          const void *bvh, uint8_t *out, void *stream) {
    if (R < 0 || R >= MR_MAX_RAYS) return LARA2DGS_E_INVALID;
    if (R == 0) return LARA2DGS_OK;
    if (!origins || !directions || !bvh || !out) return LARA2DGS_E_INVALID;
    L2D_LAUNCH_IN_SCOPE((hipStream_t)stream, mr_occluded_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, R, origins,
                        directions, t_min, t_max, (const char *)bvh, out);
    return LARA2DGS_OK;
}

int lara_meshray_visible(int32_t N, const float *points, const int32_t *skip_face, int32_t E, const float *eyes, float shrink,
                         const void *bvh, int64_t *seen, void *stream) {
    if (N < 0 || N >= MR_MAX_RAYS || E < 0 || E > LARA_MESHRAY_MAX_EYES || !(shrink >= 0.0f && shrink < 1.0f)) return LARA2DGS_E_INVALID;
    if (N == 0) return LARA2DGS_OK;
    if (!points || !bvh || !seen || (E > 0 && !eyes)) return LARA2DGS_E_INVALID;
    L2D_LAUNCH_IN_SCOPE((hipStream_t)stream, mr_visible_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, N, points, skip_face,
                        E, eyes, 1.0f - shrink, (const char *)bvh, (long long *)seen);
    return LARA2DGS_OK;
}

int lara_meshray_raytri_host(int64_t n, const float *origins, const float *directions, const float *t_min, const float *t_max,
                             const float *triangles9, uint8_t *hit, double *t, double *bary) {
    if (n < 0 || (n > 0 && (!origins || !directions || !triangles9 || !hit || !t))) return LARA2DGS_E_INVALID;
    for (int64_t i = 0; i < n; ++i) {
        const LaraRay ray = lara_ray_setup(origins + 3 * i, directions + 3 * i);
        const float *p = triangles9 + 9 * i;
        double tt = __builtin_inf(), b[3] = {NAN, NAN, NAN};
        const bool h = lara_raytri(ray, t_min ? (double)t_min[i] : 0.0, t_max ? (double)t_max[i] : __builtin_inf(), p, p + 3, p + 6, tt, b);
        hit[i] = h ? 1 : 0;
        t[i] = tt;
        if (bary) { bary[3 * i] = b[0]; bary[3 * i + 1] = b[1]; bary[3 * i + 2] = b[2]; }
    }
    return LARA2DGS_OK;
}

int lara_meshray_box_entry_host(int64_t n, const float *origins, const float *directions, const float *boxes6, const float *t_min,
                                const float *t_max, double *out) {
    if (n < 0 || (n > 0 && (!origins || !directions || !boxes6 || !out))) return LARA2DGS_E_INVALID;
    for (int64_t i = 0; i < n; ++i) {
        const LaraRay ray = lara_ray_setup(origins + 3 * i, directions + 3 * i);
        out[i] = lara_raybox(ray, boxes6 + 6 * i, boxes6 + 6 * i + 3, t_min ? (double)t_min[i] : 0.0,
                             t_max ? (double)t_max[i] : __builtin_inf());
    }
    return LARA2DGS_OK;
}

}  // extern "C"
