// meshsign.hip -- is a point inside a mesh, on the triangle hierarchy of meshbvh.hip on gfx950: the crossings of up to three fixed
// rays per point counted with their orientation, the vote over them with the signed distance, the lattice counts of a volume IoU,
// and the mesh's signed volume.  The walk of bvhwalk.h over the buffer lara_meshbvh_build wrote (meshbvh_layout.h; its records:
// trimesh.h), with the crossing of raycross.h per record and the margined entry parameter of raybox.h per box.
// Interface, the rules and the orders of summation in include/lara_meshsign.h.
//
//   ms_rows_kernel       one thread per (point, ray), blockIdx.y = ray: the walk without a best-so-far, every accepted record counted
//   ms_vote_kernel       one thread per point: the vote, the status bits, the sign on the distance
//   ms_counts_kernel     one thread per point: eight flags, a wave's butterfly, four waves through LDS, one integer atomic each
//   ms_volume_kernel     one workgroup: the records strided over its threads, then rowsum.h's order
// The walk has no LDS, no atomics and no stack.  Built with -ffp-contract=off.
#include "common.h"
#include "unigrid.h"
#include "raytri.h"
#include "raybox.h"
#include "raycross.h"
#include "bvhwalk.h"
#include "rowsum.h"
#include "../../include/lara_meshsign.h"

#include <cmath>

namespace {

constexpr int64_t MS_MAX_ROWS = 1ll << 30;
constexpr int MS_K = LARA_MESHSIGN_MAX_RAYS;

struct MsCount { int cross, wind, touch; };

// The walk, in the stored sibling order: a slot is entered exactly when it is non-empty and the ray has a parameter of [0, +inf)
// inside the inflated box; every accepted crossing of a leaf's records counts.
__device__ __forceinline__ void ms_walk(MsCount &c, const LaraRay &ray, const char *__restrict__ bvh) {
    const MbWalk w = mb_walk_open(bvh);
    if (!ray.ok || w.n_valid <= 0 || !w.ok) return;
    lara_bvhwalk(
        w.hdr->L, 0,
        [&](const int level, const int slot) LARA_BVHWALK_INLINE {
            float blo[3], bhi[3];
            mb_load_box((const float2 *)(bvh + w.hdr->L.box[level]), (size_t)slot, blo, bhi);
            return lara_raybox(ray, blo, bhi, 0.0, (double)INFINITY) < (double)INFINITY;
        },
        [&](const int leaf) LARA_BVHWALK_INLINE {
            return mb_leaf_records(w.rec, w.T, leaf, [&](const TriRec &m, const int) LARA_BVHWALK_INLINE {
                int orient, touch;
                if (lara_raycross(ray, m.p[0], m.p[1], m.p[2], orient, touch)) {
                    c.cross++;
                    c.wind += orient;
                    c.touch |= touch;
                }
                return false;      // (no record ends this walk)
            });
        });
}

__global__ void __launch_bounds__(256)
ms_rows_kernel(const int N, const float *__restrict__ p, const int K, const char *__restrict__ bvh, int *__restrict__ cross,
               int *__restrict__ wind) {
    const int i = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (i >= N) return;
    const float dirs[MS_K][3] = LARA_MESHSIGN_DIRECTIONS;
    const float pf[3] = {p[3 * (size_t)i], p[3 * (size_t)i + 1], p[3 * (size_t)i + 2]};
    const float df[3] = {k == 0 ? dirs[0][0] : (k == 1 ? dirs[1][0] : dirs[2][0]), k == 0 ? dirs[0][1] : (k == 1 ? dirs[1][1] : dirs[2][1]),
                         k == 0 ? dirs[0][2] : (k == 1 ? dirs[1][2] : dirs[2][2])};
    MsCount c{0, 0, 0};
    const bool finite = tri_point_finite(pf);
    if (finite) ms_walk(c, lara_ray_setup(pf, df), bvh);
    const bool usable = finite && !c.touch;
    cross[(size_t)i * K + k] = usable ? c.cross : -1;
    wind[(size_t)i * K + k] = usable ? c.wind : 0;
}

__global__ void __launch_bounds__(256)
ms_vote_kernel(const int N, const int K, const int *__restrict__ cross, const int *__restrict__ wind, const int rule,
               const float *__restrict__ dist, unsigned char *__restrict__ inside, unsigned char *__restrict__ status,
               float *__restrict__ sdf) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    int usable = 0, votes = 0;
    for (int k = 0; k < K; k++) {
        const int c = cross[(size_t)i * K + k], w = wind[(size_t)i * K + k];
        if (c < 0) continue;
        usable++;
        votes += (rule == LARA_MESHSIGN_RULE_WINDING ? w != 0 : (c & 1) != 0) ? 1 : 0;
    }
    const bool in = 2 * votes > usable;
    inside[i] = in ? 1 : 0;
    status[i] = (unsigned char)((votes != 0 && votes != usable ? 1 : 0) | (usable < K ? 2 : 0) | (usable == 0 ? 4 : 0));
    if (sdf) {
        const float d = dist[i];
        sdf[i] = in ? -d : d;
    }
}

constexpr int MS_COUNTS = 8;

__global__ void __launch_bounds__(256)
ms_counts_kernel(const int N, const unsigned char *__restrict__ inside_a, const unsigned char *__restrict__ status_a,
                 const unsigned char *__restrict__ inside_b, const unsigned char *__restrict__ status_b,
                 unsigned long long *__restrict__ out) {
    __shared__ int red[MS_COUNTS][4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    int a = 0, b = 0, sa = 0, sb = 0;
    if (i < N) { a = inside_a[i] != 0; b = inside_b[i] != 0; sa = status_a[i]; sb = status_b[i]; }
    const int flag[MS_COUNTS] = {a, b, a & b, a | b, sa & 1, sb & 1, (sa >> 2) & 1, (sb >> 2) & 1};
#pragma unroll
    for (int q = 0; q < MS_COUNTS; q++) rowsum_wave(red[q], flag[q]);
    __syncthreads();
    if (threadIdx.x < MS_COUNTS) {
        const int q = threadIdx.x;
        const int s = ((red[q][0] + red[q][1]) + red[q][2]) + red[q][3];
        if (s) atomicAdd(out + q, (unsigned long long)s);
    }
}

// out[0] = the signed volume, out[1] = the area, out[2] = the valid records
__global__ void __launch_bounds__(256)
ms_volume_kernel(const char *__restrict__ bvh, double *__restrict__ out) {
    __shared__ double red[2][4];
    __shared__ int redc[4];
    const MbHeader *hdr = (const MbHeader *)bvh;
    const int T = hdr->count[LARA_MESHBVH_HDR_TRIANGLES];
    const int top = hdr->L.levels - 1;
    const float4 *rec = (const float4 *)(bvh + hdr->L.rec);
    double c[3] = {0.0, 0.0, 0.0};
    if (top >= 0 && top < MB_LEVELS) {
        float lo[3], hi[3];
        mb_load_box((const float2 *)(bvh + hdr->L.box[top]), 0, lo, hi);
        if (lo[0] <= hi[0])
#pragma unroll
            for (int j = 0; j < 3; j++) c[j] = 0.5 * (double)lo[j] + 0.5 * (double)hi[j];
    }
    double vol = 0.0, area = 0.0;
    int n = 0;
    for (int r = threadIdx.x; r < T; r += 256) {
        const TriRec m = tri_load(rec, r);
        if (m.id < 0) continue;
        double a[3], b[3], e[3], u[3], v[3];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            a[j] = (double)m.p[0][j] - c[j];
            b[j] = (double)m.p[1][j] - c[j];
            e[j] = (double)m.p[2][j] - c[j];
            u[j] = (double)m.p[1][j] - (double)m.p[0][j];
            v[j] = (double)m.p[2][j] - (double)m.p[0][j];
        }
        vol += (a[0] * (b[1] * e[2] - b[2] * e[1]) + a[1] * (b[2] * e[0] - b[0] * e[2])) + a[2] * (b[0] * e[1] - b[1] * e[0]);
        const double nx = u[1] * v[2] - u[2] * v[1], ny = u[2] * v[0] - u[0] * v[2], nz = u[0] * v[1] - u[1] * v[0];
        area += sqrt((nx * nx + ny * ny) + nz * nz);
        n++;
    }
    rowsum_wave(red[0], vol);
    rowsum_wave(red[1], area);
    rowsum_wave(redc, n);
    __syncthreads();
    if (threadIdx.x == 0) {
        out[0] = (((red[0][0] + red[0][1]) + red[0][2]) + red[0][3]) / 6.0;
        out[1] = (((red[1][0] + red[1][1]) + red[1][2]) + red[1][3]) / 2.0;
        out[2] = (double)(((redc[0] + redc[1]) + redc[2]) + redc[3]);
    }
}

}  // namespace

extern "C" {

int lara_meshsign_rows(int32_t N, const float *points, int32_t K, const void *bvh, int32_t *cross, int32_t *wind, void *stream) {
    if (N < 0 || K < 1 || K > MS_K || (int64_t)N * K >= MS_MAX_ROWS) return LARA2DGS_E_INVALID;
    if (N == 0) return LARA2DGS_OK;
    if (!points || !bvh || !cross || !wind) return LARA2DGS_E_INVALID;
    L2D_LAUNCH_IN_SCOPE((hipStream_t)stream, ms_rows_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)K), dim3(256), 0, N, points, K,
                        (const char *)bvh, cross, wind);
    return LARA2DGS_OK;
}

int lara_meshsign_vote(int32_t N, int32_t K, const int32_t *cross, const int32_t *wind, int32_t rule, const float *dist,
                       uint8_t *inside, uint8_t *status, float *sdf, void *stream) {
    if (N < 0 || N >= MS_MAX_ROWS || K < 1 || K > MS_K || (int64_t)N * K >= MS_MAX_ROWS) return LARA2DGS_E_INVALID;
    if (rule != LARA_MESHSIGN_RULE_PARITY && rule != LARA_MESHSIGN_RULE_WINDING) return LARA2DGS_E_INVALID;
    if (N == 0) return LARA2DGS_OK;
    if (!cross || !wind || !inside || !status || (sdf && !dist)) return LARA2DGS_E_INVALID;
    L2D_LAUNCH_IN_SCOPE((hipStream_t)stream, ms_vote_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, N, K, cross, wind, rule,
                        dist, inside, status, sdf);
    return LARA2DGS_OK;
}

int lara_meshsign_counts(int32_t N, const uint8_t *inside_a, const uint8_t *status_a, const uint8_t *inside_b, const uint8_t *status_b,
                         int64_t *out, void *stream) {
    if (N < 0 || N >= MS_MAX_ROWS || !out) return LARA2DGS_E_INVALID;
    if (N > 0 && (!inside_a || !status_a || !inside_b || !status_b)) return LARA2DGS_E_INVALID;
    L2D_HIP(hipMemsetAsync(out, 0, MS_COUNTS * sizeof(int64_t), (hipStream_t)stream));
    if (N == 0) return LARA2DGS_OK;
    L2D_LAUNCH_IN_SCOPE((hipStream_t)stream, ms_counts_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, N, inside_a, status_a,
                        inside_b, status_b, (unsigned long long *)out);
    return LARA2DGS_OK;
}

int lara_meshsign_volume(const void *bvh, double *out, void *stream) {
    if (!bvh || !out) return LARA2DGS_E_INVALID;
    L2D_LAUNCH_IN_SCOPE((hipStream_t)stream, ms_volume_kernel, dim3(1), dim3(256), 0, (const char *)bvh, out);
    return LARA2DGS_OK;
}

int lara_meshsign_cross_host(int64_t n, const float *origins, const float *directions, const float *triangles9, uint8_t *hit,
                             int8_t *orient, uint8_t *touch) {
    if (n < 0 || (n > 0 && (!origins || !directions || !triangles9 || !hit || !orient || !touch))) return LARA2DGS_E_INVALID;
    for (int64_t i = 0; i < n; ++i) {
        const LaraRay ray = lara_ray_setup(origins + 3 * i, directions + 3 * i);
        const float *p = triangles9 + 9 * i;
        int o = 0, t = 0;
        const bool h = lara_raycross(ray, p, p + 3, p + 6, o, t);
        hit[i] = h ? 1 : 0;
        orient[i] = h ? (int8_t)o : 0;
        touch[i] = h ? (uint8_t)t : 0;
    }
    return LARA2DGS_OK;
}

int lara_meshsign_rows_host(int32_t N, const float *points, int32_t K, int64_t T, const float *triangles9, int32_t *cross,
                            int32_t *wind) {
    if (N < 0 || K < 1 || K > MS_K || (int64_t)N * K >= MS_MAX_ROWS || T < 0) return LARA2DGS_E_INVALID;
    if (N == 0) return LARA2DGS_OK;
    if (!points || !cross || !wind || (T > 0 && !triangles9)) return LARA2DGS_E_INVALID;
    const float dirs[MS_K][3] = LARA_MESHSIGN_DIRECTIONS;
    for (int64_t i = 0; i < N; ++i)
        for (int k = 0; k < K; ++k) {
            const float *pf = points + 3 * i;
            const bool finite = lara_raytri_finite(pf[0]) && lara_raytri_finite(pf[1]) && lara_raytri_finite(pf[2]);
            const LaraRay ray = lara_ray_setup(pf, dirs[k]);
            int c = 0, w = 0, touched = 0;
            for (int64_t j = 0; finite && j < T; ++j) {
                const float *p = triangles9 + 9 * j;
                int o, t;
                if (!lara_raycross(ray, p, p + 3, p + 6, o, t)) continue;
                c++;
                w += o;
                touched |= t;
            }
            const bool usable = finite && !touched;
            cross[i * K + k] = usable ? c : -1;
            wind[i * K + k] = usable ? w : 0;
        }
    return LARA2DGS_OK;
}

}  // extern "C"
