// meshbvh.hip -- exact point-to-triangle distances at any distance on gfx950: a bounding-volume hierarchy over a mesh's triangles,
// Morton-sorted records under an implicit complete 8-ary tree of boxes, and a stackless walk that prunes with the margined bound of
// boxbound.h.  Interface, the key and box rules, the margin and the tie rule in include/lara_meshbvh.h; the distance is
// tridist.h's, and the validity rule, the record, the tie rule and the result write are trimesh.h's, the functions meshdist.hip runs,
// so the two searches return the same bits.
//
//   mb_bounds_kernel                        the box of the valid triangles (partials per workgroup); the bad and the valid count
//   mb_header_kernel                        the partials -> lo, inv of the cell rule; T, the levels and the layout
//   mb_keys_kernel                          per triangle: Morton code of its box centre -> the 64-bit key            (the caller sorts)
//   mb_records_kernel                       48-byte records {p0, p1, p2, id or -1} in sorted order
//   mb_leaf_kernel / mb_level_kernel        the boxes of level 0 from the records, of level k + 1 from level k: one launch a level
//   mb_query_kernel                         one thread per query: the seed leaf, then the walk
// Every hand-off between workgroups is a launch boundary.  The only atomics are the two integer counters; the query has none.
// Built with -ffp-contract=off.
#include "common.h"
#include "unigrid.h"
#include "tridist.h"
#include "boxbound.h"
#include "bvhwalk.h"      // the walk, and meshbvh_layout.h (MbLayout, MbHeader, mb_layout, mb_load_box): shared by every walker

#include <cmath>

namespace {

constexpr int64_t MB_MAX_TRIANGLES = 1ll << 26, MB_MAX_POINTS = 1ll << 30;
constexpr unsigned long long MB_ID_MASK = (1ull << 26) - 1ull, MB_INVALID = 1ull << 62;

// part[block][6] = min x y z, max x y z of the valid triangles the workgroup strides over; the two counters
__global__ void __launch_bounds__(256)
mb_bounds_kernel(const int Nv, const int T, const float *__restrict__ v, const int *__restrict__ t, float *__restrict__ part,
                 int *__restrict__ count) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    int bad = 0, valid = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < T; i += (long long)gridDim.x * 256) {
        float p[3][3];
        if (!tri_fetch(Nv, v, t, i, p)) { bad++; continue; }
        valid++;
        box_grow(lo, hi, p);
    }
    if (bad) atomicAdd(&count[LARA_MESHBVH_HDR_BAD], bad);
    if (valid) atomicAdd(&count[LARA_MESHBVH_HDR_VALID], valid);
    box_block_partial(lo, hi, part);
}

// one wave: the box of all partials -> lo, inv of the cell rule; T, the levels and the layout
__global__ void __launch_bounds__(64)
mb_header_kernel(const int blocks, const float *__restrict__ part, const int T, const MbLayout L, MbHeader *__restrict__ hdr) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    box_gather_partials(blocks, part, lo, hi);
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const bool any = lo[j] <= hi[j];      // (false: no valid triangle)
        const float ext = any ? hi[j] - lo[j] : 0.0f;
        float inv = ext > 0.0f ? 1024.0f / ext : 0.0f;
        if (!(inv < INFINITY)) inv = 0.0f;
        hdr->lo[j] = any ? lo[j] : 0.0f;
        hdr->inv[j] = inv;
    }
    hdr->count[LARA_MESHBVH_HDR_TRIANGLES] = T;
    hdr->count[LARA_MESHBVH_HDR_LEVELS] = L.levels;
    hdr->L = L;
}

__device__ __forceinline__ unsigned mb_spread(unsigned x) {      // bit b of the low 10 -> bit 3 b
    x &= 0x3ffu;
    x = (x | (x << 16)) & 0x030000ffu;
    x = (x | (x << 8)) & 0x0300f00fu;
    x = (x | (x << 4)) & 0x030c30c3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}

// the 30-bit Morton code of the point c under the header's cell rule
__device__ __forceinline__ unsigned mb_morton(const float c[3], const float lo[3], const float inv[3]) {
    const unsigned x = (unsigned)mm_cell_axis((c[0] - lo[0]) * inv[0], 1024);
    const unsigned y = (unsigned)mm_cell_axis((c[1] - lo[1]) * inv[1], 1024);
    const unsigned z = (unsigned)mm_cell_axis((c[2] - lo[2]) * inv[2], 1024);
    return mb_spread(x) | (mb_spread(y) << 1) | (mb_spread(z) << 2);
}

__global__ void __launch_bounds__(256)
mb_keys_kernel(const int Nv, const int T, const float *__restrict__ v, const int *__restrict__ t, const MbHeader *__restrict__ hdr,
               unsigned long long *__restrict__ keys) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= T) return;
    float p[3][3];
    unsigned long long key = MB_INVALID | (unsigned long long)i;
    if (tri_fetch(Nv, v, t, i, p)) {
        const float lo[3] = {hdr->lo[0], hdr->lo[1], hdr->lo[2]}, inv[3] = {hdr->inv[0], hdr->inv[1], hdr->inv[2]};
        float c[3];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const float mn = fminf(fminf(p[0][j], p[1][j]), p[2][j]), mx = fmaxf(fmaxf(p[0][j], p[1][j]), p[2][j]);
            c[j] = 0.5f * mn + 0.5f * mx;
        }
        key = ((unsigned long long)mb_morton(c, lo, inv) << 26) | (unsigned long long)i;
    }
    keys[i] = key;
}

// rec[j] = the triangle the sorted key j names.  A key that names no triangle of this mesh (the caller sorted something else)
// gives an invalid record, never an index beyond the mesh
__global__ void __launch_bounds__(256)
mb_records_kernel(const int Nv, const int T, const float *__restrict__ v, const int *__restrict__ t,
                  const unsigned long long *__restrict__ keys, float4 *__restrict__ rec) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= T) return;
    const unsigned long long key = keys[j];
    const long long i = (long long)(key & MB_ID_MASK);
    float p[3][3] = {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};
    const bool ok = (key >> 56) == 0ull && i < T && tri_fetch(Nv, v, t, i, p);
    tri_store(rec, (size_t)j, p, ok ? (int)i : -1);
}

__device__ __forceinline__ void mb_store_box(float2 *__restrict__ box, const size_t j, const float lo[3], const float hi[3]) {
    box[3 * j] = make_float2(lo[0], lo[1]);
    box[3 * j + 1] = make_float2(lo[2], hi[0]);
    box[3 * j + 2] = make_float2(hi[1], hi[2]);
}

// level 0: slot j = the box of the valid records 8 j .. 8 j + 7; `padded` slots are written
__global__ void __launch_bounds__(256)
mb_leaf_kernel(const int T, const int padded, const float4 *__restrict__ rec, float2 *__restrict__ box) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= padded) return;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    mb_leaf_records(rec, T, j, [&](const TriRec &m, const int) LARA_BVHWALK_INLINE {
        box_grow(lo, hi, m.p);
        return false;
    });
    mb_store_box(box, (size_t)j, lo, hi);
}

// level k + 1: slot j = the box of the child slots 8 j .. 8 j + 7 below n_child
__global__ void __launch_bounds__(256)
mb_level_kernel(const int n_child, const int padded, const float2 *__restrict__ child, float2 *__restrict__ box) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= padded) return;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int k = 0; k < 8; k++) {
        const long long c = 8ll * j + k;
        if (c >= n_child) break;
        float clo[3], chi[3];
        mb_load_box(child, (size_t)c, clo, chi);
#pragma unroll
        for (int a = 0; a < 3; a++) {
            lo[a] = fminf(lo[a], clo[a]);
            hi[a] = fmaxf(hi[a], chi[a]);
        }
    }
    mb_store_box(box, (size_t)j, lo, hi);
}

// the eight records of leaf `leaf`; pos = the record of the candidate
__device__ __forceinline__ void mb_leaf(Nearest<double> &best, int &pos, const float q[3], const float4 *__restrict__ rec, const int T,
                                        const int leaf) {
    mb_leaf_records(rec, T, leaf, [&](const TriRec &m, const int r) LARA_BVHWALK_INLINE {
        double c[3];
        if (best.take(lara_tridist(q, m.p[0], m.p[1], m.p[2], c), m.id)) pos = r;
        return false;
    });
}

__global__ void __launch_bounds__(256)
mb_query_kernel(const int N, const float *__restrict__ q, const char *__restrict__ bvh, float *__restrict__ dist,
                int *__restrict__ face, float *__restrict__ closest) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const MbWalk w = mb_walk_open(bvh);
    const MbHeader *hdr = w.hdr;
    const float qf[3] = {q[3 * (size_t)i], q[3 * (size_t)i + 1], q[3 * (size_t)i + 2]};
    Nearest<double> best{INFINITY, NEAREST_NONE};
    int pos = 0;      // the candidate's record: the records are in sorted order, not by id
    if (tri_point_finite(qf) && w.n_valid > 0 && w.ok) {
        // the seed: the first valid key not below the query's own code, and the leaf it lies in
        const unsigned long long *keys = (const unsigned long long *)(bvh + hdr->L.keys);
        const float lo[3] = {hdr->lo[0], hdr->lo[1], hdr->lo[2]}, inv[3] = {hdr->inv[0], hdr->inv[1], hdr->inv[2]};
        const unsigned long long want = (unsigned long long)mb_morton(qf, lo, inv) << 26;
        int a = 0, b = w.n_valid;      // the first position in [0, n_valid] whose key is >= want
        for (int step = 0; step < 27 && a < b; step++) {
            const int mid = a + ((b - a) >> 1);
            if (keys[mid] < want) a = mid + 1; else b = mid;
        }
        mb_leaf(best, pos, qf, w.rec, w.T, min(a, w.n_valid - 1) >> 3);
        // the walk, in the stored order: a slot is entered unless it is empty or its bound is strictly above the best so far
        lara_bvhwalk(
            hdr->L, 0,
            [&](const int level, const int slot) LARA_BVHWALK_INLINE {
                float blo[3], bhi[3];
                mb_load_box((const float2 *)(bvh + hdr->L.box[level]), (size_t)slot, blo, bhi);
                const double bound = lara_boxbound(qf, blo, bhi);
                return bound < (double)INFINITY && !(bound > best.d2);
            },
            [&](const int leaf) LARA_BVHWALK_INLINE {
                mb_leaf(best, pos, qf, w.rec, w.T, leaf);
                return false;
            });
    }
    tri_write_result(i, qf, best, w.rec, pos, dist, face, closest);
}

}  // namespace

extern "C" {

int64_t lara_meshbvh_bytes(int32_t T) {
    if (T <= 0 || T >= MB_MAX_TRIANGLES) return LARA2DGS_E_INVALID;
    return mb_layout(T).total;
}

int lara_meshbvh_layout(int32_t T, int64_t *out) {
    if (T <= 0 || T >= MB_MAX_TRIANGLES || !out) return LARA2DGS_E_INVALID;
    const MbLayout L = mb_layout(T);
    out[0] = L.keys; out[1] = L.rec; out[2] = L.levels; out[3] = L.total;
    for (int k = 0; k < MB_LEVELS; k++) {
        out[4 + 2 * k] = k < L.levels ? L.box[k] : 0;
        out[5 + 2 * k] = k < L.levels ? L.n[k] : 0;
    }
    return LARA2DGS_OK;
}

int lara_meshbvh_keys(int32_t Nv, int32_t T, const float *vertices, const int32_t *triangles, void *bvh, void *stream) {
    if (T <= 0 || T >= MB_MAX_TRIANGLES || Nv <= 0 || Nv >= MB_MAX_POINTS) return LARA2DGS_E_INVALID;
    if (!vertices || !triangles || !bvh) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const MbLayout L = mb_layout(T);
    char *base = (char *)bvh;
    MbHeader *hdr = (MbHeader *)base;
    float *part = (float *)(base + L.part);
    const unsigned tb = (unsigned)((T + 255) / 256);
    const int bb = (int)(tb < (unsigned)MM_BOUNDS_BLOCKS ? tb : (unsigned)MM_BOUNDS_BLOCKS);
    L2D_HIP(hipMemsetAsync(hdr, 0, 256, s));
    L2D_LAUNCH_IN_SCOPE(s, mb_bounds_kernel, dim3((unsigned)bb), dim3(256), 0, Nv, T, vertices, triangles, part, hdr->count);
    L2D_LAUNCH_IN_SCOPE(s, mb_header_kernel, dim3(1), dim3(64), 0, bb, (const float *)part, T, L, hdr);
    L2D_LAUNCH_IN_SCOPE(s, mb_keys_kernel, dim3(tb), dim3(256), 0, Nv, T, vertices, triangles, (const MbHeader *)hdr,
                        (unsigned long long *)(base + L.keys));
    return LARA2DGS_OK;
}

int lara_meshbvh_build(int32_t Nv, int32_t T, const float *vertices, const int32_t *triangles, void *bvh, void *stream) {
    if (T <= 0 || T >= MB_MAX_TRIANGLES || Nv <= 0 || Nv >= MB_MAX_POINTS) return LARA2DGS_E_INVALID;
    if (!vertices || !triangles || !bvh) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const MbLayout L = mb_layout(T);
    char *base = (char *)bvh;
    float4 *rec = (float4 *)(base + L.rec);
    L2D_LAUNCH_IN_SCOPE(s, mb_records_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, Nv, T, vertices, triangles,
                        (const unsigned long long *)(base + L.keys), rec);
    for (int k = 0; k < L.levels; k++) {
        const int padded = (L.n[k] + 7) / 8 * 8;
        float2 *box = (float2 *)(base + L.box[k]);
        if (k == 0) {
            L2D_LAUNCH_IN_SCOPE(s, mb_leaf_kernel, dim3((unsigned)((padded + 255) / 256)), dim3(256), 0, T, padded, (const float4 *)rec, box);
        } else {
            L2D_LAUNCH_IN_SCOPE(s, mb_level_kernel, dim3((unsigned)((padded + 255) / 256)), dim3(256), 0, L.n[k - 1], padded,
                                (const float2 *)(base + L.box[k - 1]), box);
        }
    }
    return LARA2DGS_OK;
}

int lara_meshbvh_query(int32_t N, const float *queries, const void *bvh, float *dist, int32_t *face, float *closest, void *stream) {
    if (N < 0 || N >= MB_MAX_POINTS) return LARA2DGS_E_INVALID;
    if (N == 0) return LARA2DGS_OK;
    if (!queries || !bvh || !dist || !face) return LARA2DGS_E_INVALID;
    L2D_LAUNCH_IN_SCOPE((hipStream_t)stream, mb_query_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, N, queries,
                        (const char *)bvh, dist, face, closest);
    return LARA2DGS_OK;
}

int lara_meshbvh_box_bound_host(int64_t n, const float *queries, const float *boxes6, double *out) {
    if (n < 0 || (n > 0 && (!queries || !boxes6 || !out))) return LARA2DGS_E_INVALID;
    for (int64_t i = 0; i < n; ++i) out[i] = lara_boxbound(queries + 3 * i, boxes6 + 6 * i, boxes6 + 6 * i + 3);
    return LARA2DGS_OK;
}

}  // extern "C"
