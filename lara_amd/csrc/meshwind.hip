// meshwind.hip -- generalised (solid-angle) winding numbers of a mesh, on the triangle hierarchy of meshbvh.hip on gfx950: per-node
// moments in a buffer of their own, a walk that sums the exact term of solidangle.h near the point and a node's dipole term far
// from it, and the classification of the sums (the two host entries: meshwind_host.h).  The walk of bvhwalk.h over the buffer
// lara_meshbvh_build wrote (meshbvh_layout.h; its records: trimesh.h), and the one walker that needs per-node data beyond boxes:
// its three-way decision on a slot (empty, far, near) is the walk's `enter`.  Interface, the rules and the orders of summation
// in include/lara_meshwind.h.
//
//   mw_leaf_kernel       one thread per stored slot of level 0: the sums over its up-to-8 valid records, in stored order
//   mw_level_kernel      one thread per stored slot of level k: the sums over its 8 children, in slot order; one launch a level
//   mw_rows_kernel       one thread per point: the walk
//   mw_classify_kernel   one thread per point: the threshold, the band, the sign on the distance
// No LDS, no atomics and no stack anywhere.  Built with -ffp-contract=off.
#include "common.h"
#include "unigrid.h"
#include "bvhwalk.h"
#include "solidangle.h"
#include "meshwind_host.h"
#include "../../include/lara_meshwind.h"

#include <cmath>

namespace {

constexpr int64_t MW_MAX_TRIANGLES = 1ll << 26, MW_MAX_POINTS = 1ll << 30;
constexpr double MW_FOUR_PI = 12.566370614359172;

// the first 256 bytes of the moments buffer
struct MwHeader { int64_t off[MB_LEVELS], T; };
static_assert(sizeof(MwHeader) <= LARA_MESHWIND_HEADER_BYTES, "the header's slot");
static_assert(LARA_MESHWIND_SLOT_BYTES == 8 * sizeof(double), "a slot is 8 doubles");

struct MwLayout { MwHeader h; int64_t total; };

MwLayout mw_layout(const MbLayout &L, const int64_t T) {
    MwLayout w = {};
    int64_t o = LARA_MESHWIND_HEADER_BYTES;
    for (int k = 0; k < L.levels; k++) {
        w.h.off[k] = o;
        o += ((int64_t)L.n[k] + 7) / 8 * 8 * LARA_MESHWIND_SLOT_BYTES;
    }
    w.h.T = T;
    w.total = o;
    return w;
}

// the slot's 8 doubles from its sums; A == 0: flagged, all zero
__device__ __forceinline__ void mw_store_slot(double2 *__restrict__ slot, const double N[3], const double A, const double S[3],
                                              const float2 *__restrict__ box, const size_t j) {
    double c[3] = {0.0, 0.0, 0.0}, r2 = 0.0;
    const bool any = A > 0.0;
    if (any) {
        float lo[3], hi[3];
        mb_load_box(box, j, lo, hi);
        double m[3];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            c[a] = S[a] / A;
            const double below = c[a] - (double)lo[a], above = (double)hi[a] - c[a];
            m[a] = fmax(below * below, above * above);
        }
        r2 = (m[0] + m[1]) + m[2];
    }
    slot[0] = make_double2(any ? N[0] : 0.0, any ? N[1] : 0.0);
    slot[1] = make_double2(any ? N[2] : 0.0, any ? A : 0.0);
    slot[2] = make_double2(c[0], c[1]);
    slot[3] = make_double2(c[2], r2);
}

__global__ void __launch_bounds__(256)
mw_leaf_kernel(const int T, const int padded, const char *__restrict__ bvh, const int64_t box_off, char *__restrict__ mom,
               const MwHeader h) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const MbHeader *hdr = (const MbHeader *)bvh;
    if (j >= padded || hdr->count[LARA_MESHBVH_HDR_TRIANGLES] != T) return;
    if (j == 0) *(MwHeader *)mom = h;
    const float4 *rec = (const float4 *)(bvh + hdr->L.rec);
    double N[3] = {0.0, 0.0, 0.0}, A = 0.0, S[3] = {0.0, 0.0, 0.0};
    mb_leaf_records(rec, T, j, [&](const TriRec &m, const int) LARA_BVHWALK_INLINE {
        double u[3], v[3], c[3];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            u[a] = (double)m.p[1][a] - (double)m.p[0][a];
            v[a] = (double)m.p[2][a] - (double)m.p[0][a];
            c[a] = (((double)m.p[0][a] + (double)m.p[1][a]) + (double)m.p[2][a]) / 3.0;
        }
        const double n[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
        const double At = 0.5 * sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
        A += At;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            N[a] += 0.5 * n[a];
            S[a] += At * c[a];
        }
        return false;
    });
    mw_store_slot((double2 *)(mom + h.off[0]) + 4 * (size_t)j, N, A, S, (const float2 *)(bvh + box_off), (size_t)j);
}

__global__ void __launch_bounds__(256)
mw_level_kernel(const int T, const int n_child, const int padded, const char *__restrict__ bvh, const int64_t box_off,
                const double2 *__restrict__ child, double2 *__restrict__ out) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const MbHeader *hdr = (const MbHeader *)bvh;
    if (j >= padded || hdr->count[LARA_MESHBVH_HDR_TRIANGLES] != T) return;
    double N[3] = {0.0, 0.0, 0.0}, A = 0.0, S[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < 8; k++) {
        const long long c = 8ll * j + k;
        if (c >= n_child) break;
        const double2 s0 = child[4 * c], s1 = child[4 * c + 1], s2 = child[4 * c + 2], s3 = child[4 * c + 3];
        N[0] += s0.x; N[1] += s0.y; N[2] += s1.x;
        A += s1.y;
        S[0] += s1.y * s2.x; S[1] += s1.y * s2.y; S[2] += s1.y * s3.x;
    }
    mw_store_slot(out + 4 * (size_t)j, N, A, S, (const float2 *)(bvh + box_off), (size_t)j);
}

// The walk, in the stored sibling order.
__global__ void __launch_bounds__(256)
mw_rows_kernel(const int N, const float *__restrict__ p, const char *__restrict__ bvh, const char *__restrict__ mom, const double bb,
               double *__restrict__ w, int *__restrict__ n_tri, int *__restrict__ n_far) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const MbWalk wk = mb_walk_open(bvh);
    const MwHeader *mh = (const MwHeader *)mom;
    const float pf[3] = {p[3 * (size_t)i], p[3 * (size_t)i + 1], p[3 * (size_t)i + 2]};
    const bool ok = tri_point_finite(pf) && mh->T == (int64_t)wk.T && wk.ok;
    double sum = ok ? 0.0 : (double)NAN;
    int tested = 0, far = 0;
    if (ok) {
        const double q[3] = {(double)pf[0], (double)pf[1], (double)pf[2]};
        lara_bvhwalk(
            wk.hdr->L, 0,
            // an empty slot: nothing; a far one: its dipole term; a near one: entered
            [&](const int level, const int pos) LARA_BVHWALK_INLINE {
                const double2 *slot = (const double2 *)(mom + mh->off[level]) + 4 * (size_t)pos;
                const double2 s1 = slot[1];
                if (!(s1.y > 0.0)) return false;
                const double2 s2 = slot[2], s3 = slot[3];
                const double d[3] = {s2.x - q[0], s2.y - q[1], s3.x - q[2]};
                const double d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
                if (!(d2 > bb * s3.y)) return true;
                const double2 s0 = slot[0];
                sum += ((d[0] * s0.x + d[1] * s0.y) + d[2] * s1.x) / (d2 * sqrt(d2));
                far++;
                return false;
            },
            [&](const int leaf) LARA_BVHWALK_INLINE {
                return mb_leaf_records(wk.rec, wk.T, leaf, [&](const TriRec &m, const int) LARA_BVHWALK_INLINE {
                    sum += lara_solidangle(pf, m.p[0], m.p[1], m.p[2]);
                    tested++;
                    return false;      // (no record ends this walk)
                });
            });
    }
    w[i] = sum / MW_FOUR_PI;
    if (n_tri) n_tri[i] = tested;
    if (n_far) n_far[i] = far;
}

__global__ void __launch_bounds__(256)
mw_classify_kernel(const int N, const double *__restrict__ w, const double threshold, const double band, const float *__restrict__ dist,
                   unsigned char *__restrict__ inside, unsigned char *__restrict__ status, float *__restrict__ sdf) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const double x = w[i];
    const bool in = x > threshold, finite = fabs(x) < (double)INFINITY;
    inside[i] = in ? 1 : 0;
    status[i] = (unsigned char)((fabs(x - threshold) < band ? 1 : 0) | (finite ? 0 : 4));
    if (sdf) {
        const float d = dist[i];
        sdf[i] = in ? -d : d;
    }
}

}  // namespace

extern "C" {

int64_t lara_meshwind_moments_bytes(int32_t T) {
    if (T <= 0 || T >= MW_MAX_TRIANGLES) return LARA2DGS_E_INVALID;
    return mw_layout(mb_layout(T), T).total;
}

int lara_meshwind_moments(int32_t T, const void *bvh, void *moments, void *stream) {
    if (T <= 0 || T >= MW_MAX_TRIANGLES || !bvh || !moments) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const MbLayout L = mb_layout(T);
    const MwLayout W = mw_layout(L, T);
    const char *base = (const char *)bvh;
    char *mom = (char *)moments;
    for (int k = 0; k < L.levels; k++) {
        const int padded = (L.n[k] + 7) / 8 * 8;
        if (k == 0) {
            L2D_LAUNCH_IN_SCOPE(s, mw_leaf_kernel, dim3((unsigned)((padded + 255) / 256)), dim3(256), 0, T, padded, base, L.box[0], mom, W.h);
        } else {
            L2D_LAUNCH_IN_SCOPE(s, mw_level_kernel, dim3((unsigned)((padded + 255) / 256)), dim3(256), 0, T, L.n[k - 1], padded, base,
                                L.box[k], (const double2 *)(mom + W.h.off[k - 1]), (double2 *)(mom + W.h.off[k]));
        }
    }
    return LARA2DGS_OK;
}

int lara_meshwind_rows(int32_t N, const float *points, const void *bvh, const void *moments, double beta, double *w, int32_t *n_tri,
                       int32_t *n_far, void *stream) {
    if (N < 0 || N >= MW_MAX_POINTS || !(beta > 0.0)) return LARA2DGS_E_INVALID;
    if (N == 0) return LARA2DGS_OK;
    if (!points || !bvh || !moments || !w) return LARA2DGS_E_INVALID;
    L2D_LAUNCH_IN_SCOPE((hipStream_t)stream, mw_rows_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, N, points,
                        (const char *)bvh, (const char *)moments, beta * beta, w, n_tri, n_far);
    return LARA2DGS_OK;
}

int lara_meshwind_classify(int32_t N, const double *w, double threshold, double band, const float *dist, uint8_t *inside,
                           uint8_t *status, float *sdf, void *stream) {
    if (N < 0 || N >= MW_MAX_POINTS || !(band >= 0.0) || threshold != threshold) return LARA2DGS_E_INVALID;
    if (N == 0) return LARA2DGS_OK;
    if (!w || !inside || !status || (sdf && !dist)) return LARA2DGS_E_INVALID;
    L2D_LAUNCH_IN_SCOPE((hipStream_t)stream, mw_classify_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, N, w, threshold, band,
                        dist, inside, status, sdf);
    return LARA2DGS_OK;
}

int lara_meshwind_solid_host(int64_t n, const float *points, const float *triangles9, double *omega) {
    if (n < 0 || (n > 0 && (!points || !triangles9 || !omega))) return LARA2DGS_E_INVALID;
    lara_meshwind_solid_loop(n, points, triangles9, omega);
    return LARA2DGS_OK;
}

int lara_meshwind_brute_host(int32_t N, const float *points, int64_t T, const float *triangles9, double *w) {
    if (N < 0 || N >= MW_MAX_POINTS || T < 0) return LARA2DGS_E_INVALID;
    if (N == 0) return LARA2DGS_OK;
    if (!points || !w || (T > 0 && !triangles9)) return LARA2DGS_E_INVALID;
    lara_meshwind_brute_loop(N, points, T, triangles9, w);
    return LARA2DGS_OK;
}

}  // extern "C"
