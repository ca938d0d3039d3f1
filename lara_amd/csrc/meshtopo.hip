// meshtopo.hip -- the connectivity of a triangle mesh on gfx950: half-edge keys, the rows of the unique edges, the report, the two
// CSR adjacency tables, vertex normals and the smoothing pass.  The sorts between the stages are the caller's.  Interface, the
// definitions and the orders of summation in include/lara_meshtopo.h; the two per-vertex functions in meshtopo_ops.h.
//
//   mt_keys_kernel          one thread per triangle: the three undirected edge keys, or the sentinel; bit 0 of err
//   mt_corner_keys_kernel   one thread per triangle: the three (vertex, half-edge) keys, or the sentinel
//   mt_heads_kernel         one thread per sorted position: the first key of a run
//   mt_rows_kernel          one thread per sorted position: the edge's row from the run's first two, integer atomic counts
//   mt_report_*_kernel      triangles, edges, vertices: flags summed by a wave's butterfly, one integer atomic per wave and count
//   mt_boundary_kernel      one thread per edge: the or-flags of the vertices of a boundary edge
//   mt_pair_keys_kernel     one thread per edge: its two directed pairs
//   mt_csr_kernel           one thread per key and per vertex: the values, and the offsets by binary search
//   mt_normals_kernel       one thread per vertex, its row of the face table walked in order
//   mt_smooth_kernel        one thread per vertex, its row of the neighbour table walked in order
// No floating-point atomics and no LDS.  Built with -ffp-contract=off.
#include "common.h"
#include "wave.h"
#include "meshtopo_ops.h"
#include "../../include/lara_meshtopo.h"

namespace {

constexpr int64_t MT_MAX = 1ll << 31;
constexpr long long MT_SENT = LARA_MESHTOPO_SENTINEL;
enum { MT_VERTICES, MT_REFERENCED, MT_TRIANGLES, MT_VALID, MT_DEGENERATE, MT_EDGES, MT_BOUNDARY, MT_MANIFOLD, MT_NONMANIFOLD,
       MT_INCONSISTENT, MT_BOUNDARY_VERTICES, MT_MAX_DEGREE };

inline unsigned mt_blocks(const int64_t n) { return (unsigned)((n + 255) / 256); }

// 2: valid, 1: degenerate, 0: an index outside [0, Nv)
__device__ __forceinline__ int mt_kind(const int a, const int b, const int c, const int Nv) {
    if ((unsigned)a >= (unsigned)Nv || (unsigned)b >= (unsigned)Nv || (unsigned)c >= (unsigned)Nv) return 0;
    return (a != b && b != c && a != c) ? 2 : 1;
}

// the wave's sum of `flag` onto out[slot]: every lane of the wave calls it
__device__ __forceinline__ void mt_count(unsigned long long *__restrict__ out, const int slot, const int flag) {
    const int s = wave_sum(flag);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(out + slot, (unsigned long long)s);
}

__global__ void __launch_bounds__(256)
mt_keys_kernel(const int Nv, const int T, const int *__restrict__ tri, long long *__restrict__ keys, int *__restrict__ err) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const int v[3] = {tri[3 * (size_t)t], tri[3 * (size_t)t + 1], tri[3 * (size_t)t + 2]};
    const int kind = mt_kind(v[0], v[1], v[2], Nv);
    if (kind == 0) atomicOr(err, 1);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int a = v[k], b = v[(k + 1) % 3];
        const long long lo = a < b ? a : b, hi = a < b ? b : a;
        keys[3 * (size_t)t + k] = kind == 2 ? ((lo << 32) | hi) : MT_SENT;
    }
}

__global__ void __launch_bounds__(256)
mt_corner_keys_kernel(const int Nv, const int T, const int *__restrict__ tri, long long *__restrict__ keys) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const int v[3] = {tri[3 * (size_t)t], tri[3 * (size_t)t + 1], tri[3 * (size_t)t + 2]};
    const bool valid = mt_kind(v[0], v[1], v[2], Nv) == 2;
#pragma unroll
    for (int k = 0; k < 3; k++) keys[3 * (size_t)t + k] = valid ? (((long long)v[k] << 32) | (3ll * t + k)) : MT_SENT;
}

__global__ void __launch_bounds__(256)
mt_heads_kernel(const long long n, const long long *__restrict__ keys, int *__restrict__ heads) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long key = keys[i];
    heads[i] = (key != MT_SENT && (i == 0 || keys[i - 1] != key)) ? 1 : 0;
}

__global__ void __launch_bounds__(256)
mt_rows_kernel(const long long n, const long long E, const long long *__restrict__ keys, const long long *__restrict__ order,
               const int *__restrict__ heads, const long long *__restrict__ ends, const int *__restrict__ tri, int *__restrict__ edges,
               int *__restrict__ edge_n, int *__restrict__ edge_fwd, int *__restrict__ edge_face, int *__restrict__ tri_edge) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long key = keys[i];
    if (key == MT_SENT) return;
    const long long e = ends[i] - 1, h = order[i];
    if (e < 0 || e >= E || h < 0 || h >= n) return;      // (never, on what the stages before wrote)
    const int lo = (int)(key >> 32), hi = (int)(key & 0xffffffffll), t = (int)(h / 3);
    tri_edge[h] = (int)e;
    if (heads[i]) {
        edges[2 * e] = lo;
        edges[2 * e + 1] = hi;
        edge_face[2 * e] = t;
    } else if (i > 0 && heads[i - 1]) {
        edge_face[2 * e + 1] = t;
    }
    atomicAdd(edge_n + e, 1);
    if (tri[h] == lo) atomicAdd(edge_fwd + e, 1);
}

__global__ void mt_report_head_kernel(const int Nv, const int T, const long long E, unsigned long long *__restrict__ out) {
    out[MT_VERTICES] = (unsigned long long)Nv;
    out[MT_TRIANGLES] = (unsigned long long)T;
    out[MT_EDGES] = (unsigned long long)E;
}

__global__ void __launch_bounds__(256)
mt_report_triangles_kernel(const int Nv, const int T, const int *__restrict__ tri, int *__restrict__ vflag,
                           unsigned long long *__restrict__ out) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    int kind = 0;
    if (t < T) {
        const int a = tri[3 * (size_t)t], b = tri[3 * (size_t)t + 1], c = tri[3 * (size_t)t + 2];
        kind = mt_kind(a, b, c, Nv);
        if (kind == 2) {
            atomicOr(vflag + a, 1);
            atomicOr(vflag + b, 1);
            atomicOr(vflag + c, 1);
        }
    }
    mt_count(out, MT_VALID, kind == 2);
    mt_count(out, MT_DEGENERATE, kind == 1);
}

// vflag bit 1: on a boundary edge; vdeg: incident edges
__global__ void __launch_bounds__(256)
mt_report_edges_kernel(const int Nv, const long long E, const int *__restrict__ edges, const int *__restrict__ edge_n,
                       const int *__restrict__ edge_fwd, int *__restrict__ vflag, int *__restrict__ vdeg,
                       unsigned long long *__restrict__ out) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    int n = 0, fwd = 0;
    if (e < E) {
        n = edge_n[e];
        fwd = edge_fwd[e];
        const int lo = edges[2 * e], hi = edges[2 * e + 1];
        if ((unsigned)lo < (unsigned)Nv && (unsigned)hi < (unsigned)Nv) {
            if (n == 1) {
                atomicOr(vflag + lo, 2);
                atomicOr(vflag + hi, 2);
            }
            atomicAdd(vdeg + lo, 1);
            atomicAdd(vdeg + hi, 1);
        }
    }
    mt_count(out, MT_BOUNDARY, n == 1);
    mt_count(out, MT_MANIFOLD, n == 2);
    mt_count(out, MT_NONMANIFOLD, n >= 3);
    mt_count(out, MT_INCONSISTENT, n == 2 && fwd != 1);
}

__global__ void __launch_bounds__(256)
mt_report_vertices_kernel(const int Nv, const int *__restrict__ vflag, const int *__restrict__ vdeg,
                          unsigned long long *__restrict__ out) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    int flag = 0, deg = 0;
    if (v < Nv) {
        flag = vflag[v];
        deg = vdeg[v];
    }
    mt_count(out, MT_REFERENCED, flag & 1);
    mt_count(out, MT_BOUNDARY_VERTICES, (flag >> 1) & 1);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) deg = max(deg, __shfl_xor(deg, d, 64));
    if ((threadIdx.x & 63) == 0 && deg) atomicMax(out + MT_MAX_DEGREE, (unsigned long long)deg);
}

__global__ void __launch_bounds__(256)
mt_boundary_kernel(const int Nv, const long long E, const int *__restrict__ edges, const int *__restrict__ edge_n,
                   int *__restrict__ flag) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= E || edge_n[e] != 1) return;
    const int lo = edges[2 * e], hi = edges[2 * e + 1];
    if ((unsigned)lo >= (unsigned)Nv || (unsigned)hi >= (unsigned)Nv) return;
    atomicOr(flag + lo, 1);
    atomicOr(flag + hi, 1);
}

__global__ void __launch_bounds__(256)
mt_pair_keys_kernel(const long long E, const int *__restrict__ edges, long long *__restrict__ keys) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const long long lo = edges[2 * e], hi = edges[2 * e + 1];
    keys[2 * e] = (lo << 32) | hi;
    keys[2 * e + 1] = (hi << 32) | lo;
}

__global__ void __launch_bounds__(256)
mt_csr_kernel(const int Nv, const long long n, const long long *__restrict__ keys, const int mode, long long *__restrict__ offsets,
              int *__restrict__ values) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const int w = (int)(keys[i] & 0xffffffffll);
        if (mode == LARA_MESHTOPO_CSR_FACES) {
            values[2 * i] = w / 3;
            values[2 * i + 1] = w % 3;
        } else {
            values[i] = w;
        }
    }
    if (i <= Nv) {                                   // the number of keys below i << 32
        const long long bound = i << 32;
        long long lo = 0, hi = n;
        while (lo < hi) {
            const long long mid = lo + ((hi - lo) >> 1);
            if (keys[mid] < bound) lo = mid + 1; else hi = mid;
        }
        offsets[i] = lo;
    }
}

__global__ void __launch_bounds__(256)
mt_normals_kernel(const int Nv, const float *__restrict__ V, const int *__restrict__ tri, const long long *__restrict__ offsets,
                  const int *__restrict__ faces, const int weighting, float *__restrict__ normals,
                  unsigned long long *__restrict__ zero_count) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    int zero = 0;
    if (v < Nv) {
        float out[3];
        zero = lara_meshtopo_normal(V, tri, faces, offsets[v], offsets[v + 1], weighting, out);
        normals[3 * (size_t)v] = out[0];
        normals[3 * (size_t)v + 1] = out[1];
        normals[3 * (size_t)v + 2] = out[2];
    }
    mt_count(zero_count, 0, zero);
}

__global__ void __launch_bounds__(256)
mt_smooth_kernel(const int Nv, const float *__restrict__ src, float *__restrict__ dst, const long long *__restrict__ offsets,
                 const int *__restrict__ neighbors, const double s, const int *__restrict__ fixed) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= Nv) return;
    float out[3];
    lara_meshtopo_smooth(src, neighbors, offsets[v], offsets[v + 1], s, fixed ? fixed[v] : 0, v, out);
    dst[3 * (size_t)v] = out[0];
    dst[3 * (size_t)v + 1] = out[1];
    dst[3 * (size_t)v + 2] = out[2];
}

}  // namespace

extern "C" {

int lara_meshtopo_halfedge_keys(int32_t Nv, int32_t T, const int32_t *triangles, int64_t *keys, int32_t *err, void *stream) {
    if (Nv < 0 || T < 0 || 3 * (int64_t)T >= MT_MAX) return LARA2DGS_E_INVALID;
    if (T == 0) return LARA2DGS_OK;
    if (!triangles || !keys || !err) return LARA2DGS_E_INVALID;
    L2D_LAUNCH_IN_SCOPE((hipStream_t)stream, mt_keys_kernel, dim3(mt_blocks(T)), dim3(256), 0, Nv, T, triangles, (long long *)keys, err);
    return LARA2DGS_OK;
}

int lara_meshtopo_corner_keys(int32_t Nv, int32_t T, const int32_t *triangles, int64_t *keys, void *stream) {
    if (Nv < 0 || T < 0 || 3 * (int64_t)T >= MT_MAX) return LARA2DGS_E_INVALID;
    if (T == 0) return LARA2DGS_OK;
    if (!triangles || !keys) return LARA2DGS_E_INVALID;
    L2D_LAUNCH_IN_SCOPE((hipStream_t)stream, mt_corner_keys_kernel, dim3(mt_blocks(T)), dim3(256), 0, Nv, T, triangles,
                        (long long *)keys);
    return LARA2DGS_OK;
}

int lara_meshtopo_edge_heads(int64_t n, const int64_t *keys, int32_t *heads, void *stream) {
    if (n < 0 || n >= MT_MAX) return LARA2DGS_E_INVALID;
    if (n == 0) return LARA2DGS_OK;
    if (!keys || !heads) return LARA2DGS_E_INVALID;
    L2D_LAUNCH_IN_SCOPE((hipStream_t)stream, mt_heads_kernel, dim3(mt_blocks(n)), dim3(256), 0, (long long)n, (const long long *)keys,
                        heads);
    return LARA2DGS_OK;
}

int lara_meshtopo_edge_rows(int64_t n, int64_t E, const int64_t *keys, const int64_t *order, const int32_t *heads, const int64_t *ends,
                            const int32_t *triangles, int32_t *edges, int32_t *edge_n, int32_t *edge_fwd, int32_t *edge_face,
                            int32_t *tri_edge, void *stream) {
    if (n < 0 || n >= MT_MAX || n % 3 != 0 || E < 0 || E > n) return LARA2DGS_E_INVALID;
    if (n == 0) return LARA2DGS_OK;
    if (!keys || !order || !heads || !ends || !triangles || !tri_edge) return LARA2DGS_E_INVALID;
    if (E > 0 && (!edges || !edge_n || !edge_fwd || !edge_face)) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    L2D_HIP(hipMemsetAsync(tri_edge, 0xff, (size_t)n * sizeof(int32_t), s));
    if (E == 0) return LARA2DGS_OK;
    L2D_HIP(hipMemsetAsync(edge_n, 0, (size_t)E * sizeof(int32_t), s));
    L2D_HIP(hipMemsetAsync(edge_fwd, 0, (size_t)E * sizeof(int32_t), s));
    L2D_HIP(hipMemsetAsync(edge_face, 0xff, (size_t)E * 2 * sizeof(int32_t), s));
    L2D_LAUNCH_IN_SCOPE(s, mt_rows_kernel, dim3(mt_blocks(n)), dim3(256), 0, (long long)n, (long long)E, (const long long *)keys,
                        (const long long *)order, heads, (const long long *)ends, triangles, edges, edge_n, edge_fwd, edge_face,
                        tri_edge);
    return LARA2DGS_OK;
}

int lara_meshtopo_report(int32_t Nv, int32_t T, int64_t E, const int32_t *triangles, const int32_t *edges, const int32_t *edge_n,
                         const int32_t *edge_fwd, int32_t *work, int64_t *out, void *stream) {
    if (Nv < 0 || T < 0 || 3 * (int64_t)T >= MT_MAX || E < 0 || E > 3 * (int64_t)T || !out) return LARA2DGS_E_INVALID;
    if ((Nv > 0 && !work) || (T > 0 && !triangles) || (E > 0 && (!edges || !edge_n || !edge_fwd))) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    unsigned long long *o = (unsigned long long *)out;
    L2D_HIP(hipMemsetAsync(out, 0, LARA_MESHTOPO_REPORT * sizeof(int64_t), s));
    L2D_LAUNCH_IN_SCOPE(s, mt_report_head_kernel, dim3(1), dim3(1), 0, Nv, T, (long long)E, o);
    if (Nv == 0) return LARA2DGS_OK;          // (then no triangle is valid and there is no edge)
    L2D_HIP(hipMemsetAsync(work, 0, (size_t)Nv * 2 * sizeof(int32_t), s));
    if (T > 0) L2D_LAUNCH_IN_SCOPE(s, mt_report_triangles_kernel, dim3(mt_blocks(T)), dim3(256), 0, Nv, T, triangles, work, o);
    if (E > 0)
        L2D_LAUNCH_IN_SCOPE(s, mt_report_edges_kernel, dim3(mt_blocks(E)), dim3(256), 0, Nv, (long long)E, edges, edge_n, edge_fwd, work,
                            work + Nv, o);
    L2D_LAUNCH_IN_SCOPE(s, mt_report_vertices_kernel, dim3(mt_blocks(Nv)), dim3(256), 0, Nv, (const int *)work, (const int *)(work + Nv), o);
    return LARA2DGS_OK;
}

int lara_meshtopo_boundary_vertices(int32_t Nv, int64_t E, const int32_t *edges, const int32_t *edge_n, int32_t *flag, void *stream) {
    if (Nv < 0 || E < 0 || E >= MT_MAX) return LARA2DGS_E_INVALID;
    if (Nv == 0) return LARA2DGS_OK;
    if (!flag || (E > 0 && (!edges || !edge_n))) return LARA2DGS_E_INVALID;
    L2D_HIP(hipMemsetAsync(flag, 0, (size_t)Nv * sizeof(int32_t), (hipStream_t)stream));
    if (E == 0) return LARA2DGS_OK;
    L2D_LAUNCH_IN_SCOPE((hipStream_t)stream, mt_boundary_kernel, dim3(mt_blocks(E)), dim3(256), 0, Nv, (long long)E, edges, edge_n, flag);
    return LARA2DGS_OK;
}

int lara_meshtopo_pair_keys(int64_t E, const int32_t *edges, int64_t *keys, void *stream) {
    if (E < 0 || E >= MT_MAX) return LARA2DGS_E_INVALID;
    if (E == 0) return LARA2DGS_OK;
    if (!edges || !keys) return LARA2DGS_E_INVALID;
    L2D_LAUNCH_IN_SCOPE((hipStream_t)stream, mt_pair_keys_kernel, dim3(mt_blocks(E)), dim3(256), 0, (long long)E, edges, (long long *)keys);
    return LARA2DGS_OK;
}

int lara_meshtopo_csr(int32_t Nv, int64_t n, const int64_t *keys, int32_t mode, int64_t *offsets, int32_t *values, void *stream) {
    if (Nv < 0 || n < 0 || n >= 2 * MT_MAX || (mode != LARA_MESHTOPO_CSR_NEIGHBORS && mode != LARA_MESHTOPO_CSR_FACES)) return LARA2DGS_E_INVALID;
    if (!offsets || (n > 0 && (!keys || !values))) return LARA2DGS_E_INVALID;
    if (n == 0) {                             // every row is empty: no launch
        L2D_HIP(hipMemsetAsync(offsets, 0, ((size_t)Nv + 1) * sizeof(int64_t), (hipStream_t)stream));
        return LARA2DGS_OK;
    }
    const int64_t threads = n > (int64_t)Nv + 1 ? n : (int64_t)Nv + 1;
    L2D_LAUNCH_IN_SCOPE((hipStream_t)stream, mt_csr_kernel, dim3(mt_blocks(threads)), dim3(256), 0, Nv, (long long)n, (const long long *)keys,
                        mode, (long long *)offsets, values);
    return LARA2DGS_OK;
}

int lara_meshtopo_vertex_normals(int32_t Nv, const float *vertices, const int32_t *triangles, const int64_t *offsets,
                                 const int32_t *faces, int32_t weighting, float *normals, int64_t *zero_count, void *stream) {
    if (Nv < 0 || (weighting != LARA_MESHTOPO_WEIGHT_AREA && weighting != LARA_MESHTOPO_WEIGHT_UNIFORM) || !zero_count) return LARA2DGS_E_INVALID;
    L2D_HIP(hipMemsetAsync(zero_count, 0, sizeof(int64_t), (hipStream_t)stream));
    if (Nv == 0) return LARA2DGS_OK;
    if (!vertices || !offsets || !normals) return LARA2DGS_E_INVALID;     // (triangles and faces may be null: every row is empty then)
    L2D_LAUNCH_IN_SCOPE((hipStream_t)stream, mt_normals_kernel, dim3(mt_blocks(Nv)), dim3(256), 0, Nv, vertices, triangles,
                        (const long long *)offsets, faces, weighting, normals, (unsigned long long *)zero_count);
    return LARA2DGS_OK;
}

int lara_meshtopo_smooth_pass(int32_t Nv, const float *src, float *dst, const int64_t *offsets, const int32_t *neighbors, double s,
                              const int32_t *fixed, void *stream) {
    if (Nv < 0) return LARA2DGS_E_INVALID;
    if (Nv == 0) return LARA2DGS_OK;
    if (!src || !dst || src == dst || !offsets) return LARA2DGS_E_INVALID;
    L2D_LAUNCH_IN_SCOPE((hipStream_t)stream, mt_smooth_kernel, dim3(mt_blocks(Nv)), dim3(256), 0, Nv, src, dst,
                        (const long long *)offsets, neighbors, s, fixed);
    return LARA2DGS_OK;
}

int lara_meshtopo_normals_host(int32_t Nv, const float *vertices, const int32_t *triangles, const int64_t *offsets,
                               const int32_t *faces, int32_t weighting, float *normals, int64_t *zero_count) {
    if (Nv < 0 || (weighting != LARA_MESHTOPO_WEIGHT_AREA && weighting != LARA_MESHTOPO_WEIGHT_UNIFORM) || !zero_count) return LARA2DGS_E_INVALID;
    *zero_count = 0;
    if (Nv == 0) return LARA2DGS_OK;
    if (!vertices || !offsets || !normals) return LARA2DGS_E_INVALID;
    for (int64_t v = 0; v < Nv; ++v)
        *zero_count += lara_meshtopo_normal(vertices, triangles, faces, offsets[v], offsets[v + 1], weighting, normals + 3 * v);
    return LARA2DGS_OK;
}

int lara_meshtopo_smooth_host(int32_t Nv, const float *src, float *dst, const int64_t *offsets, const int32_t *neighbors, double s,
                              const int32_t *fixed) {
    if (Nv < 0) return LARA2DGS_E_INVALID;
    if (Nv == 0) return LARA2DGS_OK;
    if (!src || !dst || src == dst || !offsets) return LARA2DGS_E_INVALID;
    for (int64_t v = 0; v < Nv; ++v)
        lara_meshtopo_smooth(src, neighbors, offsets[v], offsets[v + 1], s, fixed ? fixed[v] : 0, v, dst + 3 * v);
    return LARA2DGS_OK;
}

}  // extern "C"
