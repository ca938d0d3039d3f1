// meshmetrics.hip -- geometry scores between two surfaces on gfx950: surface sampling, exact nearest neighbours over a uniform
// grid, and the reduction behind Chamfer / F-score / normal consistency.  Interface, formulas, the termination rule and its margin
// in include/lara_meshmetrics.h.
//
//   mm_area_kernel / mm_area_total_kernel   double triangle areas; their fixed-order sum and the bad-index count (one workgroup)
//   mm_quantise_kernel                      q = floor(area 2^s)
//   mm_scan_block / _sums / _add            inclusive scan in three launches (int64 prefix of q; uint32 ends of the grid's cells): unigrid.h
//   mm_sample_kernel                        one thread per sample: binary search in the prefix, hashed barycentrics, in double
//   mm_bounds_partial / mm_bounds_finish    the targets' box -> the grid record (the finish and the cell rule: unigrid.h)
//   mm_hist_kernel / mm_scatter_kernel      integer atomic histogram over the cells; cursor scatter of {x, y, z, index} records
//   mm_query_kernel                         one thread per query: mm_rings (unigrid.h) until the bound accepts, else onto the list
//   mm_brute_kernel                         a workgroup per listed query: all targets, tiled through LDS (coalesced loads of the
//                                           [M][3] layout, stride-3 LDS reads)
//   mm_reduce_kernel / mm_reduce_finish     per-workgroup partials, added in a fixed order (rowsum.h)
// Every hand-off between workgroups is a launch boundary.  The only atomics are integer ones (histogram, cursors, list length); no
// result depends on their order.  Built with -ffp-contract=off.
#include "common.h"
#include "unigrid.h"
#include "rowsum.h"
#include "../../include/lara_meshmetrics.h"

#include <cmath>

namespace {

static_assert(MM_MAX_GRID == LARA_MESHMETRICS_MAX_GRID, "unigrid.h and the header agree on the grid limit");
constexpr int MM_RMAX = LARA_MESHMETRICS_RMAX;
constexpr int MM_TILE = 1024;                                              // targets per LDS tile of the brute-force kernel
constexpr int MM_RQ = 3;                                                   // double partials per workgroup of the reduction

// ---- sampler --------------------------------------------------------------------------------------------------------------------

struct MmTri { double p[3][3]; bool ok; };

__device__ __forceinline__ MmTri mm_load_tri(const float *__restrict__ v, const int *__restrict__ t, const int i, const int Nv) {
    MmTri r;
    const int a = t[3 * (size_t)i], b = t[3 * (size_t)i + 1], c = t[3 * (size_t)i + 2];
    r.ok = a >= 0 && a < Nv && b >= 0 && b < Nv && c >= 0 && c < Nv;      // (not tri_fetch's rule: indices only)
    const int id[3] = {r.ok ? a : 0, r.ok ? b : 0, r.ok ? c : 0};
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int j = 0; j < 3; j++) r.p[k][j] = (double)v[3 * (size_t)id[k] + j];
    return r;
}
__device__ __forceinline__ void mm_cross(const MmTri &t, double c[3]) {
    const double e1[3] = {t.p[1][0] - t.p[0][0], t.p[1][1] - t.p[0][1], t.p[1][2] - t.p[0][2]};
    const double e2[3] = {t.p[2][0] - t.p[0][0], t.p[2][1] - t.p[0][1], t.p[2][2] - t.p[0][2]};
    c[0] = e1[1] * e2[2] - e1[2] * e2[1];
    c[1] = e1[2] * e2[0] - e1[0] * e2[2];
    c[2] = e1[0] * e2[1] - e1[1] * e2[0];
}

// area[i]; -1 marks a triangle with an index outside [0, Nv)
__global__ void __launch_bounds__(256)
mm_area_kernel(const int Nv, const int T, const float *__restrict__ v, const int *__restrict__ t, double *__restrict__ area) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= T) return;
    const MmTri tri = mm_load_tri(v, t, i, Nv);
    double c[3];
    mm_cross(tri, c);
    area[i] = tri.ok ? 0.5 * sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]) : -1.0;
}

// rec[0] = sum of the areas (thread t: items t, t + 1024, ...; then a tree), rec[1] = triangles marked bad
__global__ void __launch_bounds__(1024)
mm_area_total_kernel(const int T, const double *__restrict__ area, double *__restrict__ rec) {
    __shared__ double red[1024];
    __shared__ int bad[1024];
    const int tid = threadIdx.x;
    double s = 0.0;
    int b = 0;
    for (int k = tid; k < T; k += 1024) {
        const double a = area[k];
        if (a < 0.0) b++;
        else s += a;
    }
    red[tid] = s;
    bad[tid] = b;
    __syncthreads();
    for (int d = 512; d > 0; d >>= 1) {
        if (tid < d) { red[tid] += red[tid + d]; bad[tid] += bad[tid + d]; }
        __syncthreads();
    }
    if (tid == 0) { rec[0] = red[0]; rec[1] = (double)bad[0]; }
}

__global__ void __launch_bounds__(256)
mm_quantise_kernel(const int T, const double *__restrict__ area, const int s, long long *__restrict__ q) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= T) return;
    const double a = area[i];
    long long r = 0;
    if (a > 0.0 && a < INFINITY) {
        const double f = floor(ldexp(a, s));
        r = f < 9.0e18 ? (long long)f : 0;
    }
    q[i] = r;
}

__device__ __forceinline__ uint32_t mm_mix(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

__global__ void __launch_bounds__(256)
mm_sample_kernel(const int Nv, const int T, const float *__restrict__ v, const int *__restrict__ t,
                 const long long *__restrict__ prefix, const int n, const uint32_t seed, float *__restrict__ points,
                 float *__restrict__ normals, int *__restrict__ face) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const unsigned long long S = (unsigned long long)prefix[T - 1];
    const unsigned long long tk = ((2ull * (unsigned)k + 1ull) * S) / (2ull * (unsigned)n);
    int lo = 0, hi = T - 1;                      // the smallest i with prefix[i] > tk (prefix[T-1] = S > tk)
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if ((unsigned long long)prefix[mid] > tk) hi = mid;
        else lo = mid + 1;
    }
    const MmTri tri = mm_load_tri(v, t, lo, Nv);
    const uint32_t s0 = mm_mix(seed + 0x9e3779b9u);
    const uint32_t h1 = mm_mix(s0 ^ (2u * (uint32_t)k)), h2 = mm_mix(s0 ^ (2u * (uint32_t)k + 1u));
    const double r1 = (double)(h1 >> 8) * (1.0 / 16777216.0), r2 = (double)(h2 >> 8) * (1.0 / 16777216.0);
    const double su = sqrt(r1), b0 = 1.0 - su, b1 = su * (1.0 - r2), b2 = su * r2;
    face[k] = lo;
#pragma unroll
    for (int j = 0; j < 3; j++) points[3 * (size_t)k + j] = (float)((b0 * tri.p[0][j] + b1 * tri.p[1][j]) + b2 * tri.p[2][j]);
    if (normals) {
        double c[3];
        mm_cross(tri, c);
        const double len = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
#pragma unroll
        for (int j = 0; j < 3; j++) normals[3 * (size_t)k + j] = (float)(c[j] / len);
    }
}

// ---- nearest neighbour ----------------------------------------------------------------------------------------------------------

// part[block][6] = min x y z, max x y z of the targets the workgroup strides over (fminf / fmaxf skip a NaN)
__global__ void __launch_bounds__(256)
mm_bounds_partial(const int M, const float *__restrict__ t, float *__restrict__ part) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < M; i += (long long)gridDim.x * 256)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const float x = t[3 * i + j];
            lo[j] = fminf(lo[j], x);
            hi[j] = fmaxf(hi[j], x);
        }
    box_block_partial(lo, hi, part);
}

__device__ __forceinline__ int mm_cell(const MmGrid &g, const float x, const float y, const float z) {
    const int cx = mm_cell_axis((x - g.lo[0]) * g.inv_h, g.R[0]);
    const int cy = mm_cell_axis((y - g.lo[1]) * g.inv_h, g.R[1]);
    const int cz = mm_cell_axis((z - g.lo[2]) * g.inv_h, g.R[2]);
    return (cz * g.R[1] + cy) * g.R[0] + cx;
}

__global__ void __launch_bounds__(256)
mm_hist_kernel(const int M, const float *__restrict__ t, const MmGrid *__restrict__ grid, unsigned *__restrict__ hist) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const MmGrid g = *grid;
    atomicAdd(&hist[mm_cell(g, t[3 * (size_t)i], t[3 * (size_t)i + 1], t[3 * (size_t)i + 2])], 1u);
}

// the histogram counts back down to zero: slot = the cell's start + (count before this target) - 1
__global__ void __launch_bounds__(256)
mm_scatter_kernel(const int M, const float *__restrict__ t, const MmGrid *__restrict__ grid, unsigned *__restrict__ hist,
                  const unsigned *__restrict__ end, float4 *__restrict__ rec) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const MmGrid g = *grid;
    const float x = t[3 * (size_t)i], y = t[3 * (size_t)i + 1], z = t[3 * (size_t)i + 2];
    const int c = mm_cell(g, x, y, z);
    const unsigned start = c ? end[c - 1] : 0u;
    const unsigned pos = start + (atomicSub(&hist[c], 1u) - 1u);
    if (pos < (unsigned)M) rec[pos] = make_float4(x, y, z, __int_as_float(i));
}

__device__ __forceinline__ float mm_d2(const float qx, const float qy, const float qz, const float tx, const float ty, const float tz) {
    const float dx = qx - tx, dy = qy - ty, dz = qz - tz;
    return (dx * dx + dy * dy) + dz * dz;
}

__global__ void __launch_bounds__(256)
mm_query_kernel(const int N, const int M, const float *__restrict__ q, const MmGrid *__restrict__ grid,
                const unsigned *__restrict__ end, const float4 *__restrict__ rec, float *__restrict__ dist,
                int *__restrict__ index, int *__restrict__ list, unsigned *__restrict__ count) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const MmGrid g = *grid;
    const float qx = q[3 * (size_t)i], qy = q[3 * (size_t)i + 1], qz = q[3 * (size_t)i + 2];
    const float u[3] = {qx - g.lo[0], qy - g.lo[1], qz - g.lo[2]};
    int c[3];
    mm_locate(g, u, c);
    Nearest<float> best{INFINITY, NEAREST_NONE};
    // the records of the cells c0 .. c1 of one x row are contiguous; at most M of them (the guard costs nothing)
    const auto visit = [&](const int c0, const int c1) {
        const unsigned s = c0 ? end[c0 - 1] : 0u, e = min(end[c1], (unsigned)M);
        for (unsigned j = s; j < e; j++) {
            const float4 t = rec[j];
            best.take(mm_d2(qx, qy, qz, t.x, t.y, t.z), __float_as_int(t.w));
        }
    };
    const auto accept = [&](const float bound) { return best.d2 < bound * bound; };
    if (mm_rings(g, u, c, MM_RMAX, visit, accept)) {
        dist[i] = sqrtf(best.d2);
        index[i] = best.id;
    } else {
        list[atomicAdd(count, 1u)] = i;
    }
}

// a workgroup per listed query: all M targets in tiles of 1024 (3072 floats, loaded coalesced); a thread meets its targets in
// increasing index, so `<` alone keeps the smaller index inside a thread; across threads the tie rule is explicit
__global__ void __launch_bounds__(256)
mm_brute_kernel(const int M, const float *__restrict__ q, const float *__restrict__ t, const int *__restrict__ list,
                const unsigned *__restrict__ count, float *__restrict__ dist, int *__restrict__ index,
                int *__restrict__ fallback_count) {
    __shared__ float tile[3 * MM_TILE];
    __shared__ float wd[4];
    __shared__ int wi[4];
    const int tid = threadIdx.x;
    const unsigned n_listed = *count;
    if (blockIdx.x == 0 && tid == 0 && fallback_count) *fallback_count = (int)n_listed;
    if (blockIdx.x >= n_listed) return;
    const int qi = list[blockIdx.x];
    const float qx = q[3 * (size_t)qi], qy = q[3 * (size_t)qi + 1], qz = q[3 * (size_t)qi + 2];
    Nearest<float> best{INFINITY, NEAREST_NONE};
    const long long floats = 3ll * M;
    for (int base = 0; base < M; base += MM_TILE) {
        if (base) __syncthreads();
#pragma unroll
        for (int k = 0; k < 3 * MM_TILE / 256; k++) {
            const long long f = 3ll * base + tid + 256 * k;
            tile[tid + 256 * k] = f < floats ? t[f] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < MM_TILE / 256; m++) {
            const int j = tid + 256 * m;
            if (base + j < M) {
                const float d2 = mm_d2(qx, qy, qz, tile[3 * j], tile[3 * j + 1], tile[3 * j + 2]);
                if (d2 < best.d2) { best.d2 = d2; best.id = base + j; }
            }
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) best.take(__shfl_xor(best.d2, d, 64), __shfl_xor(best.id, d, 64));
    if ((tid & 63) == 0) { wd[tid >> 6] = best.d2; wi[tid >> 6] = best.id; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; w++) best.take(wd[w], wi[w]);
        dist[qi] = sqrtf(best.d2);
        index[qi] = best.id == NEAREST_NONE ? -1 : best.id;
    }
}

// ---- reduction ------------------------------------------------------------------------------------------------------------------

struct MmThr { int n; float v[LARA_MESHMETRICS_MAX_THRESHOLDS]; };

// part[block][3] = sum d, sum d^2, sum |nq . nt|; cnt[block][8] = queries with d <= thr[k]
__global__ void __launch_bounds__(256)
mm_reduce_kernel(const int N, const int M, const float *__restrict__ dist, const int *__restrict__ index, const float *__restrict__ nq,
                 const float *__restrict__ nt, const MmThr thr, double *__restrict__ part, unsigned *__restrict__ cnt) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    double s[MM_RQ] = {0.0, 0.0, 0.0};
    int below[LARA_MESHMETRICS_MAX_THRESHOLDS];
#pragma unroll
    for (int k = 0; k < LARA_MESHMETRICS_MAX_THRESHOLDS; k++) below[k] = 0;
    if (i < N) {
        const float d = dist[i];
        s[0] = (double)d;
        s[1] = (double)d * (double)d;
        const int j = index[i];
        if (nq && nt && j >= 0 && j < M) {
            const double a = (double)nq[3 * (size_t)i] * (double)nt[3 * (size_t)j];
            const double b = (double)nq[3 * (size_t)i + 1] * (double)nt[3 * (size_t)j + 1];
            const double c = (double)nq[3 * (size_t)i + 2] * (double)nt[3 * (size_t)j + 2];
            s[2] = fabs((a + b) + c);
        }
#pragma unroll
        for (int k = 0; k < LARA_MESHMETRICS_MAX_THRESHOLDS; k++) below[k] = (k < thr.n && d <= thr.v[k]) ? 1 : 0;
    }
    rowsum_block(s, below, part, cnt);
}

// row = N, the three sums, the counts per threshold
__global__ void __launch_bounds__(256)
mm_reduce_finish(const int N, const int blocks, const double *__restrict__ part, const unsigned *__restrict__ cnt,
                 double *__restrict__ row) {
    rowsum_finish<MM_RQ, LARA_MESHMETRICS_MAX_THRESHOLDS>(blocks, part, cnt, [&](const int q, const double v) { row[1 + q] = v; },
                                                          [&](const int q, const double v) { row[4 + q] = v; });
    if (threadIdx.x == 0) row[0] = (double)N;
}

// ---- workspace layouts ----------------------------------------------------------------------------------------------------------

struct MmSampleWs { int64_t area, prefix, bsum, rec, total; };
MmSampleWs mm_sample_ws(const int64_t T) {
    MmSampleWs w;
    int64_t o = 0;
    w.area = o;    o = align_up(o + T * 8, 256);
    w.prefix = o;  o = align_up(o + T * 8, 256);
    w.bsum = o;    o = align_up(o + ((T + MM_SCAN_BLOCK - 1) / MM_SCAN_BLOCK + 1) * 8, 256);
    w.rec = o;     o = align_up(o + 16, 256);
    w.total = o;
    return w;
}

struct MmNearestWs { int64_t grid, part, hist, end, bsum, rec, list, count, total; };
MmNearestWs mm_nearest_ws(const int64_t N, const int64_t M) {
    const int64_t R = mm_resolution(M), C = R * R * R;
    MmNearestWs w;
    int64_t o = 0;
    w.grid = o;   o = align_up(o + (int64_t)sizeof(MmGrid), 256);
    w.part = o;   o = align_up(o + MM_BOUNDS_BLOCKS * 6 * 4, 256);
    w.hist = o;   o = align_up(o + C * 4, 256);
    w.end = o;    o = align_up(o + C * 4, 256);
    w.bsum = o;   o = align_up(o + ((C + MM_SCAN_BLOCK - 1) / MM_SCAN_BLOCK + 1) * 4, 256);
    w.rec = o;    o = align_up(o + M * 16, 256);
    w.list = o;   o = align_up(o + N * 4, 256);
    w.count = o;  o = align_up(o + 4, 256);
    w.total = o;
    return w;
}

constexpr int64_t MM_MAX_POINTS = 1ll << 30, MM_MAX_TRIANGLES = 1ll << 28;

}  // namespace

extern "C" {

int64_t lara_meshmetrics_sample_workspace_bytes(int32_t T) {
    if (T <= 0 || T >= MM_MAX_TRIANGLES) return LARA2DGS_E_INVALID;
    return mm_sample_ws(T).total;
}

int lara_meshmetrics_sample_surface(int32_t Nv, int32_t T, const float *vertices, const int32_t *triangles, int32_t n,
                                    int32_t seed, int64_t *q, int32_t *scale_exp, float *points, float *normals, int32_t *face,
                                    void *workspace, void *stream) {
    if (T <= 0 || T >= MM_MAX_TRIANGLES || Nv <= 0 || Nv >= MM_MAX_POINTS || n < 0 || n > LARA_MESHMETRICS_MAX_SAMPLES)
        return LARA2DGS_E_INVALID;
    if (!vertices || !triangles || !q || !scale_exp || !workspace || (n > 0 && (!points || !face))) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const MmSampleWs w = mm_sample_ws(T);
    char *ws = (char *)workspace;
    double *area = (double *)(ws + w.area), *rec = (double *)(ws + w.rec);
    long long *prefix = (long long *)(ws + w.prefix), *bsum = (long long *)(ws + w.bsum);
    const unsigned tb = (unsigned)((T + 255) / 256);
    L2D_LAUNCH_IN_SCOPE(s, mm_area_kernel, dim3(tb), dim3(256), 0, Nv, T, vertices, triangles, area);
    L2D_LAUNCH_IN_SCOPE(s, mm_area_total_kernel, dim3(1), dim3(1024), 0, T, (const double *)area, rec);
    double host[2] = {0.0, 0.0};      // the call's one host read
    L2D_HIP(hipMemcpyAsync(host, rec, sizeof(host), hipMemcpyDeviceToHost, s));
    L2D_HIP(hipStreamSynchronize(s));
    if (host[1] != 0.0 || !(host[0] > 0.0) || !(host[0] < INFINITY)) return LARA2DGS_E_INVALID;
    int e = 0;
    std::frexp(host[0], &e);
    const int sc = 39 - e;
    *scale_exp = sc;
    L2D_LAUNCH_IN_SCOPE(s, mm_quantise_kernel, dim3(tb), dim3(256), 0, T, (const double *)area, sc, (long long *)q);
    L2D_TRY(mm_scan<long long>((const long long *)q, prefix, bsum, T, s));
    if (n > 0)
        L2D_LAUNCH_IN_SCOPE(s, mm_sample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, Nv, T, vertices, triangles,
                            (const long long *)prefix, n, (uint32_t)seed, points, normals, face);
    return LARA2DGS_OK;
}

int32_t lara_meshmetrics_grid_resolution(int32_t M) { return M <= 0 ? LARA2DGS_E_INVALID : mm_resolution(M); }

int64_t lara_meshmetrics_nearest_workspace_bytes(int32_t N, int32_t M) {
    if (N < 0 || N >= MM_MAX_POINTS || M <= 0 || M >= MM_MAX_POINTS) return LARA2DGS_E_INVALID;
    return mm_nearest_ws(N, M).total;
}

int lara_meshmetrics_nearest(int32_t N, int32_t M, const float *queries, const float *targets, float *dist, int32_t *index,
                             int32_t *fallback_count, void *workspace, void *stream) {
    if (N < 0 || N >= MM_MAX_POINTS || M <= 0 || M >= MM_MAX_POINTS) return LARA2DGS_E_INVALID;
    if (N == 0) return LARA2DGS_OK;
    if (!queries || !targets || !dist || !index || !workspace) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const MmNearestWs w = mm_nearest_ws(N, M);
    char *ws = (char *)workspace;
    MmGrid *grid = (MmGrid *)(ws + w.grid);
    float *part = (float *)(ws + w.part);
    unsigned *hist = (unsigned *)(ws + w.hist), *end = (unsigned *)(ws + w.end), *bsum = (unsigned *)(ws + w.bsum);
    unsigned *count = (unsigned *)(ws + w.count);
    float4 *rec = (float4 *)(ws + w.rec);
    int *list = (int *)(ws + w.list);
    const int R = mm_resolution(M);
    const long long C = (long long)R * R * R;
    const unsigned mb = (unsigned)((M + 255) / 256), nb = (unsigned)((N + 255) / 256);
    const int bb = (int)(mb < (unsigned)MM_BOUNDS_BLOCKS ? mb : (unsigned)MM_BOUNDS_BLOCKS);
    L2D_HIP(hipMemsetAsync(hist, 0, (size_t)C * 4, s));
    L2D_HIP(hipMemsetAsync(count, 0, 4, s));
    L2D_LAUNCH_IN_SCOPE(s, mm_bounds_partial, dim3((unsigned)bb), dim3(256), 0, M, targets, part);
    L2D_LAUNCH_IN_SCOPE(s, mm_bounds_finish, dim3(1), dim3(64), 0, bb, (const float *)part, R, grid);
    L2D_LAUNCH_IN_SCOPE(s, mm_hist_kernel, dim3(mb), dim3(256), 0, M, targets, (const MmGrid *)grid, hist);
    L2D_TRY(mm_scan<unsigned>((const unsigned *)hist, end, bsum, C, s));
    L2D_LAUNCH_IN_SCOPE(s, mm_scatter_kernel, dim3(mb), dim3(256), 0, M, targets, (const MmGrid *)grid, hist, (const unsigned *)end, rec);
    L2D_LAUNCH_IN_SCOPE(s, mm_query_kernel, dim3(nb), dim3(256), 0, N, M, queries, (const MmGrid *)grid, (const unsigned *)end,
                        (const float4 *)rec, dist, index, list, count);
    L2D_LAUNCH_IN_SCOPE(s, mm_brute_kernel, dim3((unsigned)N), dim3(256), 0, M, queries, targets, (const int *)list,
                        (const unsigned *)count, dist, index, fallback_count);
    return LARA2DGS_OK;
}

int64_t lara_meshmetrics_reduce_workspace_bytes(int32_t N) {
    if (N < 0 || N >= MM_MAX_POINTS) return LARA2DGS_E_INVALID;
    const int64_t blocks = ((int64_t)N + 255) / 256;
    return align_up(blocks * MM_RQ * 8 + 8, 256) + align_up(blocks * LARA_MESHMETRICS_MAX_THRESHOLDS * 4 + 4, 256);
}

int lara_meshmetrics_reduce(int32_t N, int32_t M, const float *dist, const int32_t *index, const float *normals_q, const float *normals_t,
                            int32_t n_thr, const float *thresholds, double *row, void *workspace, void *stream) {
    if (N < 0 || N >= MM_MAX_POINTS || M < 0 || M >= MM_MAX_POINTS || !row || n_thr < 0 || n_thr > LARA_MESHMETRICS_MAX_THRESHOLDS || (n_thr > 0 && !thresholds))
        return LARA2DGS_E_INVALID;
    if ((normals_q == nullptr) != (normals_t == nullptr)) return LARA2DGS_E_INVALID;
    if (N > 0 && (!dist || !index || !workspace)) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const int blocks = (N + 255) / 256;
    double *part = (double *)workspace;
    unsigned *cnt = (unsigned *)((char *)workspace + align_up((int64_t)blocks * MM_RQ * 8 + 8, 256));
    MmThr thr;
    thr.n = n_thr;
    for (int k = 0; k < LARA_MESHMETRICS_MAX_THRESHOLDS; k++) thr.v[k] = k < n_thr ? thresholds[k] : 0.0f;
    if (blocks > 0)
        L2D_LAUNCH_IN_SCOPE(s, mm_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, N, M, dist, index, normals_q, normals_t, thr, part, cnt);
    L2D_LAUNCH_IN_SCOPE(s, mm_reduce_finish, dim3(1), dim3(256), 0, N, blocks, (const double *)part, (const unsigned *)cnt, row);
    return LARA2DGS_OK;
}

}  // extern "C"
