// meshclean.hip -- crop, connected triangle clusters, largest-cluster filter and vertex compaction of an extracted mesh
// (include/lara_meshclean.h).  Thread = triangle (or row); no float atomics, every loop bounded.
#include "common.h"
#include "../../include/lara_meshclean.h"

namespace {

constexpr int MC_BLOCK = 256;
constexpr int FIND_STEPS = 64;                  // root walk of one find / jump (a non-root result only costs another round)
constexpr uint64_t EMPTY_KEY = ~0ull;
constexpr int ERR_INDEX = 1, ERR_PROBE = 2, ERR_AREA = 4;

__device__ __forceinline__ int32_t aload(const int32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void raise_err(int32_t *err, int bit) {
    __hip_atomic_fetch_or(err, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint64_t mix64(uint64_t x) {    // splitmix64 finaliser
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}
__device__ __forceinline__ bool tri_indices(const int32_t *tri, const int64_t t, const int64_t nv, int32_t v[3]) {
    v[0] = tri[3 * t]; v[1] = tri[3 * t + 1]; v[2] = tri[3 * t + 2];
    return (uint64_t)v[0] < (uint64_t)nv && (uint64_t)v[1] < (uint64_t)nv && (uint64_t)v[2] < (uint64_t)nv;
}

__global__ void __launch_bounds__(MC_BLOCK) crop_kernel(const int64_t nv, const int64_t T, const float *vert, const int32_t *tri,
                                                        const double lx, const double ly, const double lz, const double hx,
                                                        const double hy, const double hz, int32_t *keep, int32_t *err) {
    const int64_t t = (int64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
    if (t >= T) return;
    int32_t v[3];
    int32_t in = 0;
    if (tri_indices(tri, t, nv, v)) {
        in = 1;
        for (int k = 0; k < 3; k++) {
            const double x = vert[3 * (int64_t)v[k]], y = vert[3 * (int64_t)v[k] + 1], z = vert[3 * (int64_t)v[k] + 2];
            in &= (lx <= x) & (x <= hx) & (ly <= y) & (y <= hy) & (lz <= z) & (z <= hz);
        }
    } else {
        raise_err(err, ERR_INDEX);
    }
    keep[t] = in;
}

__global__ void __launch_bounds__(MC_BLOCK) compact_kernel(const int64_t n, const int width, const int32_t *src, const int32_t *keep,
                                                           const int64_t *ends, int32_t *dst) {
    const int64_t i = (int64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
    if (i >= n || !keep[i]) return;
    const int64_t o = ends[i] - 1;
    for (int k = 0; k < width; k++) dst[o * width + k] = src[i * width + k];
}

// pass 1: every triangle edge into the open-addressing table; owner[slot] = the smallest triangle on the edge.  adj[3t+e]
// receives the slot (pass 2 turns it into the owner).  A full probe sequence (capacity slots) raises ERR_PROBE.
__global__ void __launch_bounds__(MC_BLOCK) edge_insert_kernel(const int64_t T, const int32_t *tri, const int64_t cap,
                                                               uint64_t *keys, int32_t *owner, int32_t *adj, int32_t *label,
                                                               int32_t *err) {
    const int64_t t = (int64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
    if (t >= T) return;
    label[t] = (int32_t)t;
    const uint64_t mask = (uint64_t)cap - 1;
    for (int e = 0; e < 3; e++) {
        const uint32_t a = (uint32_t)tri[3 * t + e], b = (uint32_t)tri[3 * t + (e + 1) % 3];
        const uint64_t key = ((uint64_t)min(a, b) << 32) | (uint64_t)max(a, b);
        uint64_t slot = mix64(key) & mask;
        int32_t found = -1;
        for (int64_t probe = 0; probe < cap; probe++) {
            uint64_t expected = EMPTY_KEY;
            __hip_atomic_compare_exchange_strong(&keys[slot], &expected, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT);
            if (expected == EMPTY_KEY || expected == key) {      // inserted here, or the key was already here
                found = (int32_t)slot;
                break;
            }
            slot = (slot + 1) & mask;
        }
        if (found < 0) {
            raise_err(err, ERR_PROBE);
            adj[3 * t + e] = -1;
            continue;
        }
        __hip_atomic_fetch_min(&owner[found], (int32_t)t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        adj[3 * t + e] = found;
    }
}

// pass 2 (after the launch boundary: every owner is final): slot -> owner, or -1 where the triangle owns the edge itself
__global__ void __launch_bounds__(MC_BLOCK) edge_owner_kernel(const int64_t n, const int32_t *owner, int32_t *adj) {
    const int64_t i = (int64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int32_t s = adj[i];
    const int32_t o = s < 0 ? -1 : owner[s];
    adj[i] = o == (int32_t)(i / 3) ? -1 : o;
}

// bounded walk to the root (label[x] == x); `done` = the root was reached
__device__ __forceinline__ int32_t find_root(const int32_t *label, int32_t x, bool &done) {
    for (int i = 0; i < FIND_STEPS; i++) {
        const int32_t p = aload(&label[x]);
        if (p == x) { done = true; return x; }
        x = p;
    }
    done = false;
    return x;
}

// min-label hooking: for every edge (t, owner) whose roots differ, the larger root's label drops to the smaller root.
// Labels only decrease and always name a triangle of the same component, so any interleaving is safe; a round in which
// nothing changed (and every walk reached its root) is a fixpoint: one root per component, its smallest triangle.
__global__ void __launch_bounds__(MC_BLOCK) hook_kernel(const int64_t T, const int32_t *adj, int32_t *label, int32_t *work) {
    const int64_t t = (int64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
    if (t >= T) return;
    bool changed = false;
    for (int e = 0; e < 3; e++) {
        const int32_t o = adj[3 * t + e];
        if (o < 0) continue;
        bool da, db;
        const int32_t ra = find_root(label, (int32_t)t, da), rb = find_root(label, o, db);
        changed |= !(da && db);
        if (ra != rb) {
            __hip_atomic_fetch_min(&label[max(ra, rb)], min(ra, rb), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            changed = true;
        }
    }
    if (changed) __hip_atomic_store(&work[0], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// pointer jumping: every label to its root (bounded); a walk that stops short keeps the round loop going
__global__ void __launch_bounds__(MC_BLOCK) jump_kernel(const int64_t T, int32_t *label, int32_t *work) {
    const int64_t t = (int64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
    if (t >= T) return;
    bool done;
    const int32_t r = find_root(label, (int32_t)t, done);
    __hip_atomic_fetch_min(&label[t], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!done) __hip_atomic_store(&work[0], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(MC_BLOCK) stats_kernel(const int64_t nv, const int64_t T, const float *vert, const int32_t *tri,
                                                         const int32_t *label, const int64_t *root_ends, int32_t *clusters,
                                                         unsigned long long *counts, unsigned long long *acc, int32_t *err) {
    const int64_t t = (int64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
    if (t >= T) return;
    const int64_t c = root_ends[label[t]] - 1;
    clusters[t] = (int32_t)c;
    __hip_atomic_fetch_add(&counts[c], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int32_t v[3];
    if (!tri_indices(tri, t, nv, v)) {
        raise_err(err, ERR_INDEX);
        return;
    }
    const float *p0 = vert + 3 * (int64_t)v[0], *p1 = vert + 3 * (int64_t)v[1], *p2 = vert + 3 * (int64_t)v[2];
    const double ax = (double)p1[0] - p0[0], ay = (double)p1[1] - p0[1], az = (double)p1[2] - p0[2];
    const double bx = (double)p2[0] - p0[0], by = (double)p2[1] - p0[1], bz = (double)p2[2] - p0[2];
    const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
    const double area = 0.5 * sqrt(cx * cx + cy * cy + cz * cz);
    if (!(area < 2147483648.0)) {             // (NaN included) outside the fixed-point range
        raise_err(err, ERR_AREA);
        return;
    }
    // area in units of 2^-96 as hi * 2^64 + lo: both conversions are exact splits of the double (truncation < 2^-96)
    const double x = ldexp(area, 32);
    const double xf = floor(x);
    const unsigned long long hi = (unsigned long long)xf;
    const unsigned long long lo = (unsigned long long)ldexp(x - xf, 64);
    const unsigned long long old = __hip_atomic_fetch_add(&acc[2 * c + 1], lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long carry = old + lo < old ? 1ull : 0ull;       // integer sums: the same bits in any order
    __hip_atomic_fetch_add(&acc[2 * c], hi + carry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(MC_BLOCK) area_finish_kernel(const int64_t C, const unsigned long long *acc, double *area) {
    const int64_t c = (int64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
    if (c >= C) return;
    area[c] = ldexp((double)acc[2 * c], -32) + ldexp((double)acc[2 * c + 1], -96);
}

__global__ void __launch_bounds__(MC_BLOCK) keep_kernel(const int64_t nv, const int64_t T, const int32_t *tri, const int32_t *clusters,
                                                        const int64_t *counts, const int64_t *threshold, int32_t *keep,
                                                        int32_t *referenced, int32_t *err) {
    const int64_t t = (int64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
    if (t >= T) return;
    int32_t v[3];
    const bool ok = tri_indices(tri, t, nv, v);
    const int32_t k = ok && counts[clusters[t]] >= threshold[0];
    keep[t] = k;
    if (!ok) raise_err(err, ERR_INDEX);
    if (k) {                                  // (every writer stores the same 1)
        referenced[v[0]] = 1; referenced[v[1]] = 1; referenced[v[2]] = 1;
    }
}

__global__ void __launch_bounds__(MC_BLOCK) remap_kernel(const int64_t nv, const int64_t n, const int32_t *tri, const int64_t *vends,
                                                         int32_t *out, int32_t *err) {
    const int64_t i = (int64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int32_t v = tri[i];
    if ((uint64_t)v >= (uint64_t)nv) {
        raise_err(err, ERR_INDEX);
        out[i] = -1;
        return;
    }
    out[i] = (int32_t)(vends[v] - 1);
}

inline dim3 grid_of(const int64_t n) { return dim3((unsigned)((n + MC_BLOCK - 1) / MC_BLOCK)); }
constexpr int64_t MAX_ROWS = (int64_t)1 << 31;

}  // namespace

extern "C" {

int lara_mesh_crop(int64_t nv, int64_t T, const float *vertices, const int32_t *triangles, const double *box, int32_t *keep,
                   int32_t *err, void *stream) {
    if (nv < 0 || T < 0 || nv >= MAX_ROWS || T >= MAX_ROWS || !box) return LARA2DGS_E_INVALID;
    if (T == 0) return LARA2DGS_OK;
    if (!vertices || !triangles || !keep || !err) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    L2D_LAUNCH("mesh_crop", s, crop_kernel, grid_of(T), dim3(MC_BLOCK), 0, nv, T, vertices, triangles, box[0], box[1], box[2], box[3],
               box[4], box[5], keep, err);
    return LARA2DGS_OK;
}

int lara_mesh_compact_rows(int64_t n, int32_t width, const void *src, const int32_t *keep, const int64_t *ends, void *dst,
                           void *stream) {
    if (n < 0 || width <= 0 || width > 64) return LARA2DGS_E_INVALID;
    if (n == 0) return LARA2DGS_OK;
    if (!src || !keep || !ends || !dst) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    L2D_LAUNCH("mesh_compact_rows", s, compact_kernel, grid_of(n), dim3(MC_BLOCK), 0, n, (int)width, (const int32_t *)src, keep, ends,
               (int32_t *)dst);
    return LARA2DGS_OK;
}

int lara_mesh_cluster_labels(int64_t T, const int32_t *triangles, int64_t capacity, uint64_t *keys, int32_t *owner, int32_t *adj,
                             int32_t *label, int32_t *work, int32_t *rounds, void *stream) {
    if (rounds) *rounds = 0;
    if (T < 0 || T >= MAX_ROWS / 3) return LARA2DGS_E_INVALID;
    if (T == 0) return LARA2DGS_OK;
    if (!triangles || !keys || !owner || !adj || !label || !work) return LARA2DGS_E_INVALID;
    if (capacity < 6 * T || (capacity & (capacity - 1)) || capacity > MAX_ROWS) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    L2D_HIP(hipMemsetAsync(keys, 0xff, (size_t)capacity * sizeof(uint64_t), s));
    L2D_HIP(hipMemsetAsync(owner, 0x7f, (size_t)capacity * sizeof(int32_t), s));     // 0x7f7f7f7f > any triangle
    L2D_HIP(hipMemsetAsync(work, 0, 2 * sizeof(int32_t), s));
    L2D_LAUNCH("mesh_edge_insert", s, edge_insert_kernel, grid_of(T), dim3(MC_BLOCK), 0, T, triangles, capacity, keys, owner, adj, label,
               work + 1);
    L2D_LAUNCH("mesh_edge_owner", s, edge_owner_kernel, grid_of(3 * T), dim3(MC_BLOCK), 0, 3 * T, (const int32_t *)owner, adj);
    int log2t = 0;
    while (((int64_t)1 << log2t) < T) log2t++;
    const int max_rounds = 2 * log2t + 8;
    for (int r = 1; r <= max_rounds; r++) {
        L2D_HIP(hipMemsetAsync(work, 0, sizeof(int32_t), s));
        L2D_LAUNCH("mesh_hook", s, hook_kernel, grid_of(T), dim3(MC_BLOCK), 0, T, (const int32_t *)adj, label, work);
        L2D_LAUNCH("mesh_jump", s, jump_kernel, grid_of(T), dim3(MC_BLOCK), 0, T, label, work);
        int32_t h[2] = {0, 0};          // the round's host read: (changed, error)
        L2D_HIP(hipMemcpyAsync(h, work, sizeof(h), hipMemcpyDeviceToHost, s));
        L2D_HIP(hipStreamSynchronize(s));
        if (rounds) *rounds = r;
        if (h[1]) L2D_FAIL_INTERNAL();            // a probe sequence ran through the whole table
        if (!h[0]) return LARA2DGS_OK;
    }
    L2D_FAIL_INTERNAL();                          // no fixpoint within the round bound
}

int lara_mesh_cluster_stats(int64_t nv, int64_t T, const float *vertices, const int32_t *triangles, const int32_t *label,
                            const int64_t *root_ends, int64_t C, int32_t *clusters, int64_t *counts, uint64_t *area_acc,
                            double *area, int32_t *err, void *stream) {
    if (nv < 0 || T < 0 || C < 0 || C > T || nv >= MAX_ROWS || T >= MAX_ROWS) return LARA2DGS_E_INVALID;
    if (T == 0) return LARA2DGS_OK;
    if (C == 0 || !vertices || !triangles || !label || !root_ends || !clusters || !counts || !area_acc || !area || !err)
        return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    L2D_LAUNCH("mesh_cluster_stats", s, stats_kernel, grid_of(T), dim3(MC_BLOCK), 0, nv, T, vertices, triangles, label, root_ends, clusters,
               (unsigned long long *)counts, (unsigned long long *)area_acc, err);
    L2D_LAUNCH("mesh_area_finish", s, area_finish_kernel, grid_of(C), dim3(MC_BLOCK), 0, C, (const unsigned long long *)area_acc, area);
    return LARA2DGS_OK;
}

int lara_mesh_keep_clusters(int64_t nv, int64_t T, const int32_t *triangles, const int32_t *clusters, const int64_t *counts,
                            const int64_t *threshold, int32_t *keep, int32_t *referenced, int32_t *err, void *stream) {
    if (nv < 0 || T < 0 || nv >= MAX_ROWS || T >= MAX_ROWS) return LARA2DGS_E_INVALID;
    if (T == 0) return LARA2DGS_OK;
    if (!triangles || !clusters || !counts || !threshold || !keep || !referenced || !err) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    L2D_LAUNCH("mesh_keep_clusters", s, keep_kernel, grid_of(T), dim3(MC_BLOCK), 0, nv, T, triangles, clusters, counts, threshold, keep,
               referenced, err);
    return LARA2DGS_OK;
}

int lara_mesh_remap(int64_t nv, int64_t T, const int32_t *triangles, const int64_t *vertex_ends, int32_t *out, int32_t *err,
                    void *stream) {
    if (nv < 0 || T < 0 || nv >= MAX_ROWS || T >= MAX_ROWS / 3) return LARA2DGS_E_INVALID;
    if (T == 0) return LARA2DGS_OK;
    if (!triangles || !vertex_ends || !out || !err) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    L2D_LAUNCH("mesh_remap", s, remap_kernel, grid_of(3 * T), dim3(MC_BLOCK), 0, nv, 3 * T, triangles, vertex_ends, out, err);
    return LARA2DGS_OK;
}

}  // extern "C"
