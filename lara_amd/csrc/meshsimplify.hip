// meshsimplify.hip -- vertex-clustering simplification of a triangle mesh (include/lara_meshsimplify.h): cells and
// clusters through a hash table, triangle survival through a second one, per-cluster buckets in ascending order, fixed-order
// double sums per cluster (a wave each), a closed-form Cholesky solve.  Integer atomics only; every loop bounded; built with -ffp-contract=off.
#include "common.h"
#include "launch.h"
#include "wave.h"
#include "../../include/lara_meshsimplify.h"

namespace {

constexpr int MS_BLOCK = 256;
constexpr uint64_t EMPTY_KEY = ~0ull;
constexpr int64_t MAX_ROWS = (int64_t)1 << 31;
constexpr int ERR_INDEX = LARA_MESHSIMPLIFY_ERR_INDEX, ERR_PROBE = LARA_MESHSIMPLIFY_ERR_PROBE,
              ERR_NONFINITE = LARA_MESHSIMPLIFY_ERR_NONFINITE, ERR_NEGATIVE = LARA_MESHSIMPLIFY_ERR_NEGATIVE,
              ERR_EXTENT = LARA_MESHSIMPLIFY_ERR_EXTENT;

__device__ __forceinline__ void raise_err(int32_t *err, int bit) {
    __hip_atomic_fetch_or(err, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint64_t mix64(uint64_t x) {    // splitmix64 finaliser
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}
// one integer add per wave for the lanes with `flag` (a counter every thread adds to is one contended word)
__device__ __forceinline__ void wave_count_add(int32_t *counter, const bool flag) {
    const unsigned long long m = __ballot(flag);
    if (flag && (int)(threadIdx.x & 63) == __ffsll((long long)m) - 1)
        __hip_atomic_fetch_add(counter, (int32_t)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the cell of a vertex: 0, or the error bits
__device__ __forceinline__ int cell_of(const float *v, const float *origin, const float h, int32_t c[3]) {
    int bits = 0;
    for (int a = 0; a < 3; a++) {
        const float x = v[a];
        c[a] = 0;
        if (!isfinite(x)) { bits |= ERR_NONFINITE; continue; }
        const float f = floorf((x - origin[a]) / h);
        if (!(f >= 0.0f)) { bits |= ERR_NEGATIVE; continue; }
        if (f >= (float)LARA_MESHSIMPLIFY_MAX_CELL) { bits |= ERR_EXTENT; continue; }
        c[a] = (int32_t)f;
    }
    return bits;
}
__device__ __forceinline__ bool tri_indices(const int32_t *tri, const int64_t t, const int64_t nv, int32_t v[3]) {
    v[0] = tri[3 * t]; v[1] = tri[3 * t + 1]; v[2] = tri[3 * t + 2];
    return (uint64_t)v[0] < (uint64_t)nv && (uint64_t)v[1] < (uint64_t)nv && (uint64_t)v[2] < (uint64_t)nv;
}
// c = (p1 - p0) x (p2 - p0) in double; p0 as doubles in q
__device__ __forceinline__ void tri_cross(const float *vert, const int32_t v[3], double q[3], double c[3]) {
    const float *p0 = vert + 3 * (int64_t)v[0], *p1 = vert + 3 * (int64_t)v[1], *p2 = vert + 3 * (int64_t)v[2];
    q[0] = p0[0]; q[1] = p0[1]; q[2] = p0[2];
    const double ax = (double)p1[0] - q[0], ay = (double)p1[1] - q[1], az = (double)p1[2] - q[2];
    const double bx = (double)p2[0] - q[0], by = (double)p2[1] - q[1], bz = (double)p2[2] - q[2];
    c[0] = ay * bz - az * by; c[1] = az * bx - ax * bz; c[2] = ax * by - ay * bx;
}

// ---- cells and clusters -------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MS_BLOCK) cell_insert_kernel(const int64_t nv, const float *vert, const float h, const float *origin,
                                                               const int64_t cap, uint64_t *keys, int32_t *leader, int32_t *slot_of,
                                                               int32_t *err) {
    const int64_t v = (int64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (v >= nv) return;
    int32_t c[3];
    const int bits = cell_of(vert + 3 * v, origin, h, c);
    if (bits) {
        raise_err(err, bits);
        slot_of[v] = -1;
        return;
    }
    const uint64_t key = ((uint64_t)c[0] << 42) | ((uint64_t)c[1] << 21) | (uint64_t)c[2];
    const uint64_t mask = (uint64_t)cap - 1;
    uint64_t slot = mix64(key) & mask;
    int32_t found = -1;
    for (int64_t probe = 0; probe < cap; probe++) {
        uint64_t expected = EMPTY_KEY;
        __hip_atomic_compare_exchange_strong(&keys[slot], &expected, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (expected == EMPTY_KEY || expected == key) {
            found = (int32_t)slot;
            break;
        }
        slot = (slot + 1) & mask;
    }
    slot_of[v] = found;
    if (found < 0) {
        raise_err(err, ERR_PROBE);
        return;
    }
    __hip_atomic_fetch_min(&leader[found], (int32_t)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// (after the launch boundary: every leader is final)
__global__ void __launch_bounds__(MS_BLOCK) leader_flag_kernel(const int64_t nv, const int32_t *slot_of, const int32_t *leader,
                                                               int32_t *is_leader) {
    const int64_t v = (int64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (v >= nv) return;
    const int32_t s = slot_of[v];
    is_leader[v] = s >= 0 && leader[s] == (int32_t)v;
}

__global__ void __launch_bounds__(MS_BLOCK) cluster_kernel(const int64_t nv, const int64_t cap, const int32_t *slot_of,
                                                           const int32_t *leader, const int64_t *leader_ends, int32_t *vertex_cluster,
                                                           int32_t *leader_vertex) {
    const int64_t v = (int64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (v >= nv) return;
    const int32_t s = slot_of[v];
    int32_t g = -1;
    if ((uint64_t)s < (uint64_t)cap) {
        const int32_t l = leader[s];
        if ((uint64_t)l < (uint64_t)nv) {
            g = (int32_t)(leader_ends[l] - 1);
            if (l == (int32_t)v && g >= 0) leader_vertex[g] = l;
        }
    }
    vertex_cluster[v] = g;
}

// ---- triangles ----------------------------------------------------------------------------------------------------------------
// the corners' clusters, the smallest first; tslot = -1 (an index outside the mesh), -2 (two corners in one cluster) or -3 (a candidate)
__global__ void __launch_bounds__(MS_BLOCK) tri_map_kernel(const int64_t nv, const int64_t T, const int64_t n_cells, const int32_t *tri,
                                                           const int32_t *vertex_cluster, int32_t *mapped, int32_t *tslot, int32_t *err) {
    const int64_t t = (int64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (t >= T) return;
    int32_t v[3], g[3] = {-1, -1, -1};
    bool ok = tri_indices(tri, t, nv, v);
    if (ok) {
        for (int k = 0; k < 3; k++) g[k] = vertex_cluster[v[k]];
        ok = (uint64_t)g[0] < (uint64_t)n_cells && (uint64_t)g[1] < (uint64_t)n_cells && (uint64_t)g[2] < (uint64_t)n_cells;
    }
    int32_t state = -1;
    if (!ok) {
        raise_err(err, ERR_INDEX);
        g[0] = g[1] = g[2] = -1;
    } else if (g[0] == g[1] || g[1] == g[2] || g[0] == g[2]) {
        state = -2;
    } else {
        state = -3;
        const int r = g[0] < g[1] ? (g[0] < g[2] ? 0 : 2) : (g[1] < g[2] ? 1 : 2);
        const int32_t a = g[r], b = g[(r + 1) % 3], c = g[(r + 2) % 3];
        g[0] = a; g[1] = b; g[2] = c;
    }
    mapped[3 * t] = g[0]; mapped[3 * t + 1] = g[1]; mapped[3 * t + 2] = g[2];
    tslot[t] = state;
}

// every candidate into the table of triangle indices: a slot's representative is the triangle whose compare-and-swap took it;
// a later triangle with the same mapped triple (written by the launch before) shares the slot.  owner = the smallest of them.
__global__ void __launch_bounds__(MS_BLOCK) tri_insert_kernel(const int64_t T, const int32_t *mapped, const int64_t cap, int32_t *rep,
                                                              int32_t *owner, int32_t *tslot, int32_t *err) {
    const int64_t t = (int64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (t >= T || tslot[t] != -3) return;
    const int32_t a = mapped[3 * t], b = mapped[3 * t + 1], c = mapped[3 * t + 2];
    const uint64_t mask = (uint64_t)cap - 1;
    uint64_t slot = (mix64(((uint64_t)(uint32_t)a << 32) | (uint32_t)b) ^ mix64(0x9e3779b97f4a7c15ull + (uint32_t)c)) & mask;
    int32_t found = -1;
    for (int64_t probe = 0; probe < cap; probe++) {
        int32_t expected = -1;
        __hip_atomic_compare_exchange_strong(&rep[slot], &expected, (int32_t)t, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (expected == -1) {
            found = (int32_t)slot;
            break;
        }
        if ((uint64_t)expected < (uint64_t)T && mapped[3 * (int64_t)expected] == a && mapped[3 * (int64_t)expected + 1] == b &&
            mapped[3 * (int64_t)expected + 2] == c) {
            found = (int32_t)slot;
            break;
        }
        slot = (slot + 1) & mask;
    }
    if (found < 0) {
        raise_err(err, ERR_PROBE);
        tslot[t] = -1;
        return;
    }
    __hip_atomic_fetch_min(&owner[found], (int32_t)t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    tslot[t] = found;
}

__global__ void __launch_bounds__(MS_BLOCK) tri_keep_kernel(const int64_t T, const int64_t cap, const int32_t *mapped, const int32_t *tslot,
                                                            const int32_t *owner, int32_t *keep, int32_t *referenced, int32_t *counters) {
    const int64_t t = (int64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    const int32_t s = t < T ? tslot[t] : -1;
    const bool candidate = (uint64_t)s < (uint64_t)cap;
    const bool kept = candidate && owner[s] == (int32_t)t;
    wave_count_add(counters + LARA_MESHSIMPLIFY_N_DEGENERATE, s == -2);
    wave_count_add(counters + LARA_MESHSIMPLIFY_N_DUPLICATE, candidate && !kept);
    if (t >= T) return;
    keep[t] = kept;
    if (kept) {                               // (every writer stores the same 1)
        referenced[mapped[3 * t]] = 1; referenced[mapped[3 * t + 1]] = 1; referenced[mapped[3 * t + 2]] = 1;
    }
}

// ---- corner keys and buckets ----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MS_BLOCK) corner_key_kernel(const int64_t nv, const int64_t T, const float *vert, const int32_t *tri,
                                                              const int32_t *vertex_cluster, int32_t *corner_key, int32_t *counters) {
    const int64_t t = (int64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    int32_t v[3], g[3] = {-1, -1, -1};
    bool zero = false;
    if (t < T && tri_indices(tri, t, nv, v)) {
        double q[3], c[3];
        tri_cross(vert, v, q, c);
        const double l2 = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
        zero = !(l2 > 0.0 && isfinite(l2));
        if (!zero)
            for (int k = 0; k < 3; k++) g[k] = vertex_cluster[v[k]];
    }
    wave_count_add(counters + LARA_MESHSIMPLIFY_N_ZERO_AREA, zero);
    if (t >= T) return;
    corner_key[3 * t] = g[0]; corner_key[3 * t + 1] = g[1]; corner_key[3 * t + 2] = g[2];
}

__global__ void __launch_bounds__(MS_BLOCK) bucket_count_kernel(const int64_t n, const int64_t n_keys, const int32_t *key, int32_t *count) {
    const int64_t i = (int64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int32_t k = key[i];
    if ((uint64_t)k < (uint64_t)n_keys) __hip_atomic_fetch_add(&count[k], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(MS_BLOCK) bucket_scatter_kernel(const int64_t n, const int64_t n_keys, const int32_t *key,
                                                                  const int64_t *ends, int32_t *cursor, int32_t *unordered) {
    const int64_t i = (int64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int32_t k = key[i];
    if ((uint64_t)k >= (uint64_t)n_keys) return;
    const int64_t start = k ? ends[k - 1] : 0, end = ends[k];
    const int64_t p = start + __hip_atomic_fetch_add(&cursor[k], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p >= start && p < end && p < n) unordered[p] = (int32_t)i;     // (ends that do not belong to these keys write nothing outside)
}

// an item's place in its bucket = the number of smaller items there: the scatter's order does not reach `items`
__global__ void __launch_bounds__(MS_BLOCK) bucket_rank_kernel(const int64_t n, const int64_t n_keys, const int32_t *key,
                                                               const int64_t *ends, const int32_t *unordered, int32_t *items) {
    const int64_t i = (int64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int32_t k = key[i];
    if ((uint64_t)k >= (uint64_t)n_keys) return;
    const int64_t start = k ? ends[k - 1] : 0, end = ends[k];
    if (start < 0 || end > n) return;
    int64_t r = 0;
    for (int64_t j = start; j < end; j++) r += unordered[j] < (int32_t)i;
    if (start + r < end) items[start + r] = (int32_t)i;
}

// ---- sums, solve ----------------------------------------------------------------------------------------------------------------
// one wave per cluster: lane l adds the bucket's items l, l + 64, ... serially, the 64 partials meet in the xor butterfly (the
// same value in every lane).  The order is a function of the bucket alone, not of the launch.
__global__ void __launch_bounds__(MS_BLOCK) sums_kernel(const int64_t nv, const int64_t T, const int64_t n_cells, const float *vert,
                                                        const float *colors, const int32_t *tri, const int64_t *vends,
                                                        const int32_t *vitems, const int64_t *cends, const int32_t *citems,
                                                        const int quadric, double *mean, float *color_out, double *Ab) {
    const int64_t g = ((int64_t)blockIdx.x * MS_BLOCK + threadIdx.x) >> 6;       // (wave-uniform)
    const int lane = threadIdx.x & 63;
    if (g >= n_cells) return;
    const int64_t vs = g ? vends[g - 1] : 0, ve = vends[g];
    double s[3] = {0.0, 0.0, 0.0}, sc[3] = {0.0, 0.0, 0.0};
    for (int64_t j = vs + lane; j < ve; j += 64) {
        const int32_t v = vitems[j];
        if ((uint64_t)v >= (uint64_t)nv) continue;
        for (int a = 0; a < 3; a++) s[a] += (double)vert[3 * (int64_t)v + a];
        if (colors)
            for (int a = 0; a < 3; a++) sc[a] += (double)colors[3 * (int64_t)v + a];
    }
    const double cnt = (double)(ve - vs);
    double m[3];
    for (int a = 0; a < 3; a++) {
        m[a] = wave_sum(s[a]) / cnt;
        if (colors) sc[a] = wave_sum(sc[a]) / cnt;
    }
    if (lane == 0)
        for (int a = 0; a < 3; a++) {
            mean[3 * g + a] = m[a];
            if (colors) color_out[3 * g + a] = (float)sc[a];
        }
    if (!quadric) return;
    double A[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};                  // Axx Axy Axz Ayy Ayz Azz bx by bz
    const int64_t cs = g ? cends[g - 1] : 0, ce = cends[g];
    for (int64_t j = cs + lane; j < ce; j += 64) {
        const int64_t t = (int64_t)citems[j] / 3;
        int32_t v[3];
        if ((uint64_t)t >= (uint64_t)T || !tri_indices(tri, t, nv, v)) continue;
        double q[3], c[3];
        tri_cross(vert, v, q, c);
        const double l = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
        const double nx = c[0] / l, ny = c[1] / l, nz = c[2] / l, w = 0.5 * l;
        const double d = nx * (q[0] - m[0]) + ny * (q[1] - m[1]) + nz * (q[2] - m[2]);
        const double wx = w * nx, wy = w * ny, wz = w * nz, wd = w * d;
        A[0] += wx * nx; A[1] += wx * ny; A[2] += wx * nz; A[3] += wy * ny; A[4] += wy * nz; A[5] += wz * nz;
        A[6] += wd * nx; A[7] += wd * ny; A[8] += wd * nz;
    }
    for (int k = 0; k < 9; k++) A[k] = wave_sum(A[k]);
    if (lane == 0)
        for (int k = 0; k < 9; k++) Ab[9 * g + k] = A[k];
}

__global__ void __launch_bounds__(MS_BLOCK) solve_kernel(const int64_t nv, const int64_t n_cells, const int quadric, const double *mean,
                                                         const double *Ab, const float *vert, const int32_t *leader_vertex, const float h,
                                                         const float *origin, const int32_t *referenced, float *out, int32_t *counters) {
    const int64_t g = (int64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    bool clamped = false;
    if (g < n_cells) {
        double x[3] = {mean[3 * g], mean[3 * g + 1], mean[3 * g + 2]};
        const int32_t lv = leader_vertex[g];
        int32_t cell[3];
        if (quadric && (uint64_t)lv < (uint64_t)nv && cell_of(vert + 3 * (int64_t)lv, origin, h, cell) == 0) {
            const double *A = Ab + 9 * g, *b = A + 6;
            const double tr = A[0] + A[3] + A[5];
            if (tr > 0.0) {
                const double mu = 0.0009765625 * tr;
                const double m00 = A[0] + mu, m11 = A[3] + mu, m22 = A[5] + mu;
                const double l00 = sqrt(m00), l10 = A[1] / l00, l20 = A[2] / l00;
                const double l11 = sqrt(m11 - l10 * l10), l21 = (A[4] - l20 * l10) / l11;
                const double l22 = sqrt(m22 - l20 * l20 - l21 * l21);
                const double z0 = b[0] / l00, z1 = (b[1] - l10 * z0) / l11, z2 = (b[2] - l20 * z0 - l21 * z1) / l22;
                const double y2 = z2 / l22, y1 = (z1 - l21 * y2) / l11, y0 = (z0 - l10 * y1 - l20 * y2) / l00;
                const double y[3] = {y0, y1, y2};
                for (int a = 0; a < 3; a++) {
                    const double lo = (double)origin[a] + (double)cell[a] * (double)h;
                    const double hi = (double)origin[a] + (double)(cell[a] + 1) * (double)h;
                    double xa = x[a] + y[a];
                    if (xa < lo) { xa = lo; clamped = true; }
                    if (xa > hi) { xa = hi; clamped = true; }
                    x[a] = xa;
                }
            }
        }
        for (int a = 0; a < 3; a++) out[3 * g + a] = (float)x[a];
        clamped = clamped && referenced[g] != 0;
    }
    wave_count_add(counters + LARA_MESHSIMPLIFY_N_CLAMPED, clamped);
}

__global__ void __launch_bounds__(MS_BLOCK) vertex_map_kernel(const int64_t nv, const int64_t n_cells, const int32_t *vertex_cluster,
                                                              const int32_t *referenced, const int64_t *cluster_ends, int32_t *out) {
    const int64_t v = (int64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (v >= nv) return;
    const int32_t g = vertex_cluster[v];
    out[v] = (uint64_t)g < (uint64_t)n_cells && referenced[g] ? (int32_t)(cluster_ends[g] - 1) : -1;
}

inline dim3 grid_of(const int64_t n) { return dim3((unsigned)((n + MS_BLOCK - 1) / MS_BLOCK)); }
// a power of two >= 2 n (>= 64)
inline int64_t table_capacity(const int64_t n) {
    int64_t cap = 64;
    while (cap < 2 * n) cap <<= 1;
    return cap;
}
inline int64_t align256(const int64_t n) { return (n + 255) & ~(int64_t)255; }

}  // namespace

extern "C" {

int64_t lara_meshsimplify_cells_workspace_bytes(int64_t Nv) {
    if (Nv < 0 || Nv >= MAX_ROWS) return LARA2DGS_E_INVALID;
    return table_capacity(Nv) * (int64_t)(sizeof(uint64_t) + sizeof(int32_t));
}

int lara_meshsimplify_cells(int64_t Nv, const float *vertices, float h, const float *origin, int32_t *slot, int32_t *is_leader,
                            void *workspace, int32_t *err, void *stream) {
    if (Nv < 0 || Nv >= MAX_ROWS || !(h > 0.0f) || !(h < INFINITY)) return LARA2DGS_E_INVALID;
    if (Nv == 0) return LARA2DGS_OK;
    if (!vertices || !origin || !slot || !is_leader || !workspace || !err) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const int64_t cap = table_capacity(Nv);
    uint64_t *keys = (uint64_t *)workspace;
    int32_t *leader = (int32_t *)(keys + cap);
    L2D_HIP(hipMemsetAsync(keys, 0xff, (size_t)cap * sizeof(uint64_t), s));
    L2D_HIP(hipMemsetAsync(leader, 0x7f, (size_t)cap * sizeof(int32_t), s));         // 0x7f7f7f7f > any vertex
    L2D_LAUNCH_IN_SCOPE(s, cell_insert_kernel, grid_of(Nv), dim3(MS_BLOCK), 0, Nv, vertices, h, origin, cap, keys, leader, slot, err);
    L2D_LAUNCH_IN_SCOPE(s, leader_flag_kernel, grid_of(Nv), dim3(MS_BLOCK), 0, Nv, (const int32_t *)slot, (const int32_t *)leader, is_leader);
    return LARA2DGS_OK;
}

int lara_meshsimplify_clusters(int64_t Nv, const int32_t *slot, const int64_t *leader_ends, const void *workspace,
                               int32_t *vertex_cluster, int32_t *leader_vertex, void *stream) {
    if (Nv < 0 || Nv >= MAX_ROWS) return LARA2DGS_E_INVALID;
    if (Nv == 0) return LARA2DGS_OK;
    if (!slot || !leader_ends || !workspace || !vertex_cluster || !leader_vertex) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const int64_t cap = table_capacity(Nv);
    const int32_t *leader = (const int32_t *)((const uint64_t *)workspace + cap);
    L2D_LAUNCH_IN_SCOPE(s, cluster_kernel, grid_of(Nv), dim3(MS_BLOCK), 0, Nv, cap, slot, leader, leader_ends, vertex_cluster, leader_vertex);
    return LARA2DGS_OK;
}

int64_t lara_meshsimplify_triangles_workspace_bytes(int64_t T) {
    if (T < 0 || T >= MAX_ROWS / 3) return LARA2DGS_E_INVALID;
    return table_capacity(T) * (int64_t)(2 * sizeof(int32_t)) + align256(T * (int64_t)sizeof(int32_t));
}

int lara_meshsimplify_triangles(int64_t Nv, int64_t T, int64_t n_cells, const int32_t *triangles, const int32_t *vertex_cluster,
                                int32_t *mapped, int32_t *keep, int32_t *referenced, int32_t *counters, void *workspace, int32_t *err, void *stream) {
    if (Nv < 0 || T < 0 || n_cells < 0 || Nv >= MAX_ROWS || T >= MAX_ROWS / 3 || n_cells > Nv) return LARA2DGS_E_INVALID;
    if (T == 0) return LARA2DGS_OK;
    if (!triangles || !vertex_cluster || !mapped || !keep || !referenced || !counters || !workspace || !err) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const int64_t cap = table_capacity(T);
    int32_t *rep = (int32_t *)workspace, *owner = rep + cap, *tslot = owner + cap;
    L2D_HIP(hipMemsetAsync(rep, 0xff, (size_t)cap * sizeof(int32_t), s));
    L2D_HIP(hipMemsetAsync(owner, 0x7f, (size_t)cap * sizeof(int32_t), s));
    L2D_LAUNCH_IN_SCOPE(s, tri_map_kernel, grid_of(T), dim3(MS_BLOCK), 0, Nv, T, n_cells, triangles, vertex_cluster, mapped, tslot, err);
    L2D_LAUNCH_IN_SCOPE(s, tri_insert_kernel, grid_of(T), dim3(MS_BLOCK), 0, T, (const int32_t *)mapped, cap, rep, owner, tslot, err);
    L2D_LAUNCH_IN_SCOPE(s, tri_keep_kernel, grid_of(T), dim3(MS_BLOCK), 0, T, cap, (const int32_t *)mapped, (const int32_t *)tslot,
                        (const int32_t *)owner, keep, referenced, counters);
    return LARA2DGS_OK;
}

int lara_meshsimplify_corner_keys(int64_t Nv, int64_t T, const float *vertices, const int32_t *triangles,
                                  const int32_t *vertex_cluster, int32_t *corner_key, int32_t *counters, void *stream) {
    if (Nv < 0 || T < 0 || Nv >= MAX_ROWS || T >= MAX_ROWS / 3) return LARA2DGS_E_INVALID;
    if (T == 0) return LARA2DGS_OK;
    if (!vertices || !triangles || !vertex_cluster || !corner_key || !counters) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    L2D_LAUNCH_IN_SCOPE(s, corner_key_kernel, grid_of(T), dim3(MS_BLOCK), 0, Nv, T, vertices, triangles, vertex_cluster, corner_key, counters);
    return LARA2DGS_OK;
}

int lara_meshsimplify_bucket_count(int64_t n, int64_t n_keys, const int32_t *key, int32_t *count, void *stream) {
    if (n < 0 || n_keys < 0 || n >= MAX_ROWS || n_keys >= MAX_ROWS) return LARA2DGS_E_INVALID;
    if (n_keys == 0) return LARA2DGS_OK;
    if (!count || (n && !key)) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    L2D_HIP(hipMemsetAsync(count, 0, (size_t)n_keys * sizeof(int32_t), s));
    if (n == 0) return LARA2DGS_OK;
    L2D_LAUNCH_IN_SCOPE(s, bucket_count_kernel, grid_of(n), dim3(MS_BLOCK), 0, n, n_keys, key, count);
    return LARA2DGS_OK;
}

int64_t lara_meshsimplify_bucket_workspace_bytes(int64_t n, int64_t n_keys) {
    if (n < 0 || n_keys < 0 || n >= MAX_ROWS || n_keys >= MAX_ROWS) return LARA2DGS_E_INVALID;
    return align256(n_keys * (int64_t)sizeof(int32_t)) + align256(n * (int64_t)sizeof(int32_t));
}

int lara_meshsimplify_bucket_fill(int64_t n, int64_t n_keys, const int32_t *key, const int64_t *ends, int32_t *items,
                                  void *workspace, void *stream) {
    if (n < 0 || n_keys < 0 || n >= MAX_ROWS || n_keys >= MAX_ROWS) return LARA2DGS_E_INVALID;
    if (n == 0 || n_keys == 0) return LARA2DGS_OK;
    if (!key || !ends || !items || !workspace) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    int32_t *cursor = (int32_t *)workspace;
    int32_t *unordered = (int32_t *)((char *)workspace + align256(n_keys * (int64_t)sizeof(int32_t)));
    L2D_HIP(hipMemsetAsync(cursor, 0, (size_t)n_keys * sizeof(int32_t), s));
    L2D_LAUNCH_IN_SCOPE(s, bucket_scatter_kernel, grid_of(n), dim3(MS_BLOCK), 0, n, n_keys, key, ends, cursor, unordered);
    L2D_LAUNCH_IN_SCOPE(s, bucket_rank_kernel, grid_of(n), dim3(MS_BLOCK), 0, n, n_keys, key, ends, (const int32_t *)unordered, items);
    return LARA2DGS_OK;
}

int lara_meshsimplify_sums(int64_t Nv, int64_t T, int64_t n_cells, const float *vertices, const float *colors,
                           const int32_t *triangles, const int64_t *vertex_ends, const int32_t *vertex_items,
                           const int64_t *corner_ends, const int32_t *corner_items, int32_t quadric, double *mean, float *color_out,
                           double *Ab, void *stream) {
    if (Nv < 0 || T < 0 || n_cells < 0 || Nv >= MAX_ROWS || T >= MAX_ROWS / 3 || n_cells > Nv) return LARA2DGS_E_INVALID;
    if (n_cells == 0) return LARA2DGS_OK;
    if (!vertices || !vertex_ends || !vertex_items || !mean || (colors && !color_out)) return LARA2DGS_E_INVALID;
    if (quadric && (!Ab || !corner_ends || (T && (!triangles || !corner_items)))) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    L2D_LAUNCH_IN_SCOPE(s, sums_kernel, grid_of(64 * n_cells), dim3(MS_BLOCK), 0, Nv, T, n_cells, vertices, colors, triangles, vertex_ends,
                        vertex_items, corner_ends, corner_items, (int)quadric, mean, color_out, Ab);
    return LARA2DGS_OK;
}

int lara_meshsimplify_solve(int64_t Nv, int64_t n_cells, int32_t quadric, const double *mean, const double *Ab, const float *vertices,
                            const int32_t *leader_vertex, float h, const float *origin, const int32_t *referenced, float *out,
                            int32_t *counters, void *stream) {
    if (Nv < 0 || n_cells < 0 || Nv >= MAX_ROWS || n_cells > Nv || !(h > 0.0f) || !(h < INFINITY)) return LARA2DGS_E_INVALID;
    if (n_cells == 0) return LARA2DGS_OK;
    if (!mean || !vertices || !leader_vertex || !origin || !referenced || !out || !counters || (quadric && !Ab)) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    L2D_LAUNCH_IN_SCOPE(s, solve_kernel, grid_of(n_cells), dim3(MS_BLOCK), 0, Nv, n_cells, (int)quadric, mean, Ab, vertices, leader_vertex,
                        h, origin, referenced, out, counters);
    return LARA2DGS_OK;
}

int lara_meshsimplify_vertex_map(int64_t Nv, int64_t n_cells, const int32_t *vertex_cluster, const int32_t *referenced,
                                 const int64_t *cluster_ends, int32_t *out, void *stream) {
    if (Nv < 0 || n_cells < 0 || Nv >= MAX_ROWS || n_cells > Nv) return LARA2DGS_E_INVALID;
    if (Nv == 0) return LARA2DGS_OK;
    if (!vertex_cluster || !out || (n_cells && (!referenced || !cluster_ends))) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    L2D_LAUNCH_IN_SCOPE(s, vertex_map_kernel, grid_of(Nv), dim3(MS_BLOCK), 0, Nv, n_cells, vertex_cluster, referenced, cluster_ends, out);
    return LARA2DGS_OK;
}

}  // extern "C"
