// depthsurface.hip -- a ground-truth surface from depth maps on gfx950: ordered back-projection of the valid pixels, thinning to one
// point per occupied voxel, the per-view observation test, and the masked reduction of one direction's distances.  Interface,
// formulas and the order contract in include/lara_depthsurface.h.
//
//   ds_count_kernel / ds_offsets_kernel / ds_emit_kernel   the ordered compaction, generic over "is item g selected" and "write item g
//                                                          at rank r": 1024 consecutive items per workgroup in four coalesced passes,
//                                                          wave ballots for the ranks, one workgroup for the exclusive offsets
//   DsSelectPixel / DsEmitPixel                            back-projection: validity, the point, the normal (given / from depth, double)
//   ds_thin_lo_kernel / _cmax_kernel / _fill_kernel / _min_kernel / DsSelectWinner / DsEmitRow / ds_thin_finish
//                                                          lo and max cell by integer atomics on ordered images of the floats, the
//                                                          winners by an integer atomicMin per cell word
//   ds_observe_kernel                                      one thread per sample, the views' twenty floats in LDS, a depth gather per view
//   ds_reduce_kernel / ds_reduce_finish                    csrc/meshmetrics.hip's reduction with a keep mask and counted normal pairs (rowsum.h)
// Every hand-off between workgroups is a launch boundary.  The only atomics are integer min / max / add; no result depends on their
// order.  Built with -ffp-contract=off.
#include "common.h"
#include "wave.h"
#include "rowsum.h"
#include "../../include/lara_depthsurface.h"

#include <cmath>

namespace {

constexpr int DS_PASSES = 4, DS_BLOCK = 256 * DS_PASSES;      // items per workgroup of the compaction
constexpr int DS_NONE = 0x7fffffff;
constexpr int DS_CELL_TOP = LARA_DEPTHSURFACE_MAX_CELLS;      // a cell coordinate from here up is out of every admissible grid
constexpr int DS_RQ = 3;                                      // double partials per workgroup of the reduction
constexpr int DS_RC = LARA_DEPTHSURFACE_MAX_THRESHOLDS + 2;   // integer partials: kept, pairs, the thresholds
constexpr int DS_FILL_BLOCKS = 2048;

// ---- the ordered compaction -----------------------------------------------------------------------------------------------------

// cnt[block] = selected items among [1024 block, 1024 (block + 1))
template <class Select>
__global__ void __launch_bounds__(256)
ds_count_kernel(const Select sel, const long long n, unsigned *__restrict__ cnt) {
    __shared__ int wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long base = (long long)blockIdx.x * DS_BLOCK;
    int c = 0;
#pragma unroll
    for (int k = 0; k < DS_PASSES; k++) {
        const long long g = base + k * 256 + tid;
        const bool f = g < n && sel(g);
        c += __popcll(__ballot(f));
    }
    if (lane == 0) wsum[wave] = c;
    __syncthreads();
    if (tid == 0) cnt[blockIdx.x] = (unsigned)(((wsum[0] + wsum[1]) + wsum[2]) + wsum[3]);
}

// in place: cnt[i] <- cnt[0] + ... + cnt[i - 1]; total[0] = the sum of all.  One workgroup, 256 counts at a time with a carry.
__global__ void __launch_bounds__(256)
ds_offsets_kernel(unsigned *__restrict__ cnt, const int nb, long long *__restrict__ total) {
    __shared__ unsigned wtot[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned carry = 0;
    for (int c0 = 0; c0 < nb; c0 += 256) {
        const int i = c0 + tid;
        const unsigned v = i < nb ? cnt[i] : 0u;
        const unsigned incl = wave_inclusive_scan(v, lane);
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        unsigned off = carry;
        for (int w = 0; w < wave; w++) off += wtot[w];
        if (i < nb) cnt[i] = (incl - v) + off;
        carry += ((wtot[0] + wtot[1]) + wtot[2]) + wtot[3];
        __syncthreads();
    }
    if (tid == 0) total[0] = (long long)carry;
}

// item g, when selected, is written at rank off[block] + (selected items of the waves and passes in front) + (ballot bits below the lane)
template <class Select, class Emit>
__global__ void __launch_bounds__(256)
ds_emit_kernel(const Select sel, const Emit emit, const long long n, const unsigned *__restrict__ off) {
    __shared__ int wc[DS_PASSES][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long base = (long long)blockIdx.x * DS_BLOCK;
    bool f[DS_PASSES];
    int below[DS_PASSES];
#pragma unroll
    for (int k = 0; k < DS_PASSES; k++) {
        const long long g = base + k * 256 + tid;
        f[k] = g < n && sel(g);
        const unsigned long long b = __ballot(f[k]);
        below[k] = __popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) wc[k][wave] = __popcll(b);
    }
    __syncthreads();
    unsigned pos = off[blockIdx.x];
#pragma unroll
    for (int k = 0; k < DS_PASSES; k++) {
        unsigned mine = pos;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            if (w < wave) mine += (unsigned)wc[k][w];
            pos += (unsigned)wc[k][w];
        }
        if (f[k]) emit(base + k * 256 + tid, (long long)mine + below[k]);
    }
}

int ds_compaction_blocks(const long long n) { return (int)((n + DS_BLOCK - 1) / DS_BLOCK); }

// ---- back-projection ------------------------------------------------------------------------------------------------------------

struct DsMaps {
    const float *depth;
    const void *mask;
    int mask_bytes, V, H, W;
    float depth_max;
};

__device__ __forceinline__ bool ds_valid(const DsMaps &m, const long long g) {
    if (m.mask) {
        const bool in = m.mask_bytes == 4 ? ((const float *)m.mask)[g] != 0.0f : ((const unsigned char *)m.mask)[g] != 0;
        if (!in) return false;
    }
    const float d = m.depth[g];
    return d > 0.0f && d <= m.depth_max && d < INFINITY;
}

struct DsSelectPixel {
    DsMaps m;
    int stride;
    __device__ __forceinline__ bool operator()(const long long g) const {
        const int x = (int)(g % m.W), y = (int)((g / m.W) % m.H);
        return y % stride == 0 && x % stride == 0 && ds_valid(m, g);
    }
};

__device__ __forceinline__ void ds_point(const float *__restrict__ k4, const float *__restrict__ r, const int y, const int x, const float d,
                                         float p[3]) {
    const float a = ((float)x + 0.5f - k4[2]) / k4[0], b = ((float)y + 0.5f - k4[3]) / k4[1];
    const float px = a * d, py = b * d;
#pragma unroll
    for (int i = 0; i < 3; i++) p[i] = ((r[4 * i] * px + r[4 * i + 1] * py) + r[4 * i + 2] * d) + r[4 * i + 3];
}

__device__ __forceinline__ void ds_store_unit(const double c[3], float *__restrict__ out) {
    const double len = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
    const bool ok = len > 0.0 && len < (double)INFINITY;
#pragma unroll
    for (int j = 0; j < 3; j++) out[j] = ok ? (float)(c[j] / len) : 0.0f;
}

struct DsEmitPixel {
    DsMaps m;
    const float *ixt, *pose, *normal_map;
    int normal_mode;
    float jump;
    float *points, *normals;
    int *pixel;
    __device__ __forceinline__ void operator()(const long long g, const long long r) const {
        const int x = (int)(g % m.W), y = (int)((g / m.W) % m.H), v = (int)(g / ((long long)m.W * m.H));
        const float *k4 = ixt + 4 * v, *rt = pose + 16 * v;
        const float d = m.depth[g];
        float p[3];
        ds_point(k4, rt, y, x, d, p);
#pragma unroll
        for (int j = 0; j < 3; j++) points[3 * r + j] = p[j];
        pixel[r] = (int)g;
        if (normal_mode == LARA_DEPTHSURFACE_NORMALS_GIVEN) {
            const double c[3] = {(double)normal_map[3 * g], (double)normal_map[3 * g + 1], (double)normal_map[3 * g + 2]};
            ds_store_unit(c, normals + 3 * r);
        } else if (normal_mode == LARA_DEPTHSURFACE_NORMALS_DEPTH) {
            double c[3] = {0.0, 0.0, 0.0};
            if (y > 0 && y < m.H - 1 && x > 0 && x < m.W - 1) {
                const long long nb[4] = {g + m.W, g - m.W, g + 1, g - 1};
                const int ny[4] = {y + 1, y - 1, y, y}, nx[4] = {x, x, x + 1, x - 1};
                bool ok = true;
                float q[4][3];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    ok = ok && ds_valid(m, nb[k]);
                    const float dk = ok ? m.depth[nb[k]] : d;
                    ok = ok && fabsf(dk - d) <= jump;
                    ds_point(k4, rt, ny[k], nx[k], dk, q[k]);
                }
                if (ok) {
                    const double a[3] = {(double)q[0][0] - (double)q[1][0], (double)q[0][1] - (double)q[1][1], (double)q[0][2] - (double)q[1][2]};
                    const double b[3] = {(double)q[2][0] - (double)q[3][0], (double)q[2][1] - (double)q[3][1], (double)q[2][2] - (double)q[3][2]};
                    c[0] = a[1] * b[2] - a[2] * b[1];
                    c[1] = a[2] * b[0] - a[0] * b[2];
                    c[2] = a[0] * b[1] - a[1] * b[0];
                }
            }
            ds_store_unit(c, normals + 3 * r);
        }
    }
};

// ---- thinning -------------------------------------------------------------------------------------------------------------------

struct DsGridRec {
    unsigned lo_key[3];      // ordered integer images of the smallest coordinates (all bits set: no point yet)
    int cmax[3];             // the largest cell coordinates (-1: none)
    unsigned dropped;        // points with a non-finite coordinate
    unsigned pad;
};
struct DsGrid { float lo[3]; int R[3]; bool ok; };

__device__ __forceinline__ unsigned ds_key(const float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ds_unkey(const unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

__device__ __forceinline__ bool ds_finite3(const float x, const float y, const float z) {
    return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;
}
__device__ __forceinline__ int ds_cell_axis(const float p, const float lo, const float voxel) {
    const float f = floorf((p - lo) / voxel);
    return f < (float)DS_CELL_TOP ? (int)f : DS_CELL_TOP;      // (p >= lo: f >= 0)
}
__device__ __forceinline__ DsGrid ds_grid(const DsGridRec *__restrict__ rec, const int max_cells) {
    DsGrid g;
    long long prod = 1;
    g.ok = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        g.lo[a] = ds_unkey(rec->lo_key[a]);
        g.R[a] = rec->cmax[a] + 1;
        prod = g.ok ? prod * g.R[a] : 0;
        g.ok = g.ok && prod > 0 && prod <= (long long)max_cells;      // (each factor <= 2^27 + 1 and the running product <= 2^27: no overflow)
    }
    return g;
}
__device__ __forceinline__ int ds_cell(const DsGrid &g, const float x, const float y, const float z, const float voxel) {
    const int cx = ds_cell_axis(x, g.lo[0], voxel), cy = ds_cell_axis(y, g.lo[1], voxel), cz = ds_cell_axis(z, g.lo[2], voxel);
    return (cz * g.R[1] + cy) * g.R[0] + cx;
}

__global__ void __launch_bounds__(256)
ds_thin_lo_kernel(const int N, const float *__restrict__ p, DsGridRec *__restrict__ rec) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    unsigned k[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu};
    int bad = 0;
    if (i < N) {
        const float x = p[3 * (size_t)i], y = p[3 * (size_t)i + 1], z = p[3 * (size_t)i + 2];
        if (ds_finite3(x, y, z)) { k[0] = ds_key(x); k[1] = ds_key(y); k[2] = ds_key(z); }
        else bad = 1;
    }
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) k[a] = min(k[a], (unsigned)__shfl_xor((int)k[a], d, 64));
    bad = wave_sum(bad);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 3; a++)
            if (k[a] != 0xffffffffu) atomicMin(&rec->lo_key[a], k[a]);
        if (bad) atomicAdd(&rec->dropped, (unsigned)bad);
    }
}

__global__ void __launch_bounds__(256)
ds_thin_cmax_kernel(const int N, const float *__restrict__ p, const float voxel, DsGridRec *__restrict__ rec) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    int c[3] = {-1, -1, -1};
    if (i < N) {
        const float q[3] = {p[3 * (size_t)i], p[3 * (size_t)i + 1], p[3 * (size_t)i + 2]};
        if (ds_finite3(q[0], q[1], q[2]))
#pragma unroll
            for (int a = 0; a < 3; a++) c[a] = ds_cell_axis(q[a], ds_unkey(rec->lo_key[a]), voxel);
    }
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) c[a] = max(c[a], __shfl_xor(c[a], d, 64));
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int a = 0; a < 3; a++)
            if (c[a] >= 0) atomicMax(&rec->cmax[a], c[a]);
}

__global__ void __launch_bounds__(256)
ds_thin_fill_kernel(const DsGridRec *__restrict__ rec, const int max_cells, int *__restrict__ cells) {
    const DsGrid g = ds_grid(rec, max_cells);
    if (!g.ok) return;
    const long long C = (long long)g.R[0] * g.R[1] * g.R[2];
    for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < C; c += (long long)gridDim.x * 256) cells[c] = DS_NONE;
}

__global__ void __launch_bounds__(256)
ds_thin_min_kernel(const int N, const float *__restrict__ p, const float voxel, const DsGridRec *__restrict__ rec, const int max_cells,
                   int *__restrict__ cells) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const DsGrid g = ds_grid(rec, max_cells);
    const float x = p[3 * (size_t)i], y = p[3 * (size_t)i + 1], z = p[3 * (size_t)i + 2];
    if (!g.ok || !ds_finite3(x, y, z)) return;
    atomicMin(&cells[ds_cell(g, x, y, z, voxel)], i);
}

struct DsSelectWinner {
    const float *p;
    float voxel;
    const DsGridRec *rec;
    int max_cells;
    const int *cells;
    __device__ __forceinline__ bool operator()(const long long i) const {
        const DsGrid g = ds_grid(rec, max_cells);
        const float x = p[3 * i], y = p[3 * i + 1], z = p[3 * i + 2];
        if (!g.ok || !ds_finite3(x, y, z)) return false;
        return cells[ds_cell(g, x, y, z, voxel)] == (int)i;
    }
};

struct DsEmitRow {
    const float *p, *nrm;
    int *kept;
    float *out_p, *out_n;
    __device__ __forceinline__ void operator()(const long long i, const long long r) const {
        kept[r] = (int)i;
#pragma unroll
        for (int j = 0; j < 3; j++) out_p[3 * r + j] = p[3 * i + j];
        if (nrm)
#pragma unroll
            for (int j = 0; j < 3; j++) out_n[3 * r + j] = nrm[3 * i + j];
    }
};

// res[0] = N' (the offsets kernel wrote it), res[1] = dropped, res[2] = 1 where the grid does not fit max_cells
__global__ void ds_thin_finish(const DsGridRec *__restrict__ rec, const int max_cells, long long *__restrict__ res) {
    const DsGrid g = ds_grid(rec, max_cells);
    const bool any = rec->cmax[0] >= 0;
    res[1] = (long long)rec->dropped;
    res[2] = (any && !g.ok) ? 1 : 0;
}

// ---- observation ----------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256)
ds_observe_kernel(const int N, const float *__restrict__ p, const DsMaps m, const float *__restrict__ ixt, const float *__restrict__ pose,
                  const float tau, const int background_is_free, long long *__restrict__ seen) {
    __shared__ float cam[LARA_DEPTHSURFACE_MAX_VIEWS * 20];
    for (int k = threadIdx.x; k < m.V * 20; k += 256) {
        const int v = k / 20, j = k % 20;
        cam[k] = j < 4 ? ixt[4 * v + j] : pose[16 * v + (j - 4)];
    }
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float x = p[3 * (size_t)i], y = p[3 * (size_t)i + 1], z = p[3 * (size_t)i + 2];
    unsigned long long bits = 0;
    if (ds_finite3(x, y, z)) {
        const float fw = (float)m.W, fh = (float)m.H;
        const long long HW = (long long)m.H * m.W;
        for (int v = 0; v < m.V; v++) {
            const float *c = cam + 20 * v, *w = c + 4;
            float q[3];
#pragma unroll
            for (int a = 0; a < 3; a++) q[a] = ((w[4 * a] * x + w[4 * a + 1] * y) + w[4 * a + 2] * z) + w[4 * a + 3];
            const float zc = q[2];
            if (!(zc > 0.0f)) continue;
            const float u = (q[0] * c[0]) / zc + c[2], t = (q[1] * c[1]) / zc + c[3];
            if (!(u >= 0.0f && u < fw && t >= 0.0f && t < fh)) continue;
            const long long g = v * HW + (long long)((int)floorf(t)) * m.W + (int)floorf(u);
            const bool obs = ds_valid(m, g) ? zc <= m.depth[g] + tau : background_is_free != 0;
            if (obs) bits |= 1ull << v;
        }
    }
    seen[i] = (long long)bits;
}

// ---- reduction ------------------------------------------------------------------------------------------------------------------

struct DsThr { int n; float v[LARA_DEPTHSURFACE_MAX_THRESHOLDS]; };

__device__ __forceinline__ bool ds_nonzero3(const float *__restrict__ n) { return n[0] != 0.0f || n[1] != 0.0f || n[2] != 0.0f; }

// part[block][3] = sum d, sum d^2, sum |nq . nt|; cnt[block][10] = kept, counted pairs, queries with d <= thr[k]
__global__ void __launch_bounds__(256)
ds_reduce_kernel(const int N, const int M, const float *__restrict__ dist, const int *__restrict__ index, const unsigned char *__restrict__ keep,
                 const float *__restrict__ nq, const float *__restrict__ nt, const DsThr thr, double *__restrict__ part,
                 unsigned *__restrict__ cnt) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    double s[DS_RQ] = {0.0, 0.0, 0.0};
    int c[DS_RC];
#pragma unroll
    for (int k = 0; k < DS_RC; k++) c[k] = 0;
    if (i < N && (!keep || keep[i])) {
        const float d = dist[i];
        c[0] = 1;
        s[0] = (double)d;
        s[1] = (double)d * (double)d;
        const int j = index[i];
        if (nq && nt && j >= 0 && j < M && ds_nonzero3(nq + 3 * (size_t)i) && ds_nonzero3(nt + 3 * (size_t)j)) {
            const double a = (double)nq[3 * (size_t)i] * (double)nt[3 * (size_t)j];
            const double b = (double)nq[3 * (size_t)i + 1] * (double)nt[3 * (size_t)j + 1];
            const double e = (double)nq[3 * (size_t)i + 2] * (double)nt[3 * (size_t)j + 2];
            s[2] = fabs((a + b) + e);
            c[1] = 1;
        }
#pragma unroll
        for (int k = 0; k < LARA_DEPTHSURFACE_MAX_THRESHOLDS; k++) c[2 + k] = (k < thr.n && d <= thr.v[k]) ? 1 : 0;
    }
    rowsum_block(s, c, part, cnt);
}

// row: the sums -> [1 .. 3]; kept -> [0], pairs -> [4], threshold k -> [5 + k]
__global__ void __launch_bounds__(256)
ds_reduce_finish(const int blocks, const double *__restrict__ part, const unsigned *__restrict__ cnt, double *__restrict__ row) {
    rowsum_finish<DS_RQ, DS_RC>(blocks, part, cnt, [&](const int q, const double v) { row[1 + q] = v; },
                                [&](const int q, const double v) { row[q == 0 ? 0 : 3 + q] = v; });
}

// ---- host -----------------------------------------------------------------------------------------------------------------------

bool ds_maps_ok(const int V, const int H, const int W) {
    return V >= 1 && V <= LARA_DEPTHSURFACE_MAX_VIEWS && H >= 1 && W >= 1 && (long long)V * H * W < (1ll << 31) &&
           (long long)H * W < (1ll << 31);
}
bool ds_mask_ok(const void *mask, const int bytes) { return !mask || bytes == 1 || bytes == 4; }

struct DsThinWs { int64_t rec, res, cnt, cells, total; };
DsThinWs ds_thin_ws(const int64_t N, const int64_t max_cells) {
    DsThinWs w;
    int64_t o = 0;
    w.rec = o;    o = align_up(o + (int64_t)sizeof(DsGridRec), 256);
    w.res = o;    o = align_up(o + 3 * 8, 256);
    w.cnt = o;    o = align_up(o + (ds_compaction_blocks(N) + 1) * 4, 256);
    w.cells = o;  o = align_up(o + max_cells * 4, 256);
    w.total = o;
    return w;
}

}  // namespace

extern "C" {

int64_t lara_depthsurface_backproject_workspace_bytes(int32_t V, int32_t H, int32_t W) {
    if (!ds_maps_ok(V, H, W)) return LARA2DGS_E_INVALID;
    return 256 + align_up(((int64_t)ds_compaction_blocks((long long)V * H * W) + 1) * 4, 256);
}

int lara_depthsurface_backproject_count(int32_t V, int32_t H, int32_t W, const float *depth, const void *mask, int32_t mask_elem_bytes,
                                        int32_t stride, float depth_max, int64_t *n_points, void *workspace, void *stream) {
    if (!ds_maps_ok(V, H, W) || !ds_mask_ok(mask, mask_elem_bytes) || stride < 1 || std::isnan(depth_max)) return LARA2DGS_E_INVALID;
    if (!depth || !n_points || !workspace) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const long long n = (long long)V * H * W;
    const int nb = ds_compaction_blocks(n);
    long long *total = (long long *)workspace;
    unsigned *cnt = (unsigned *)((char *)workspace + 256);
    const DsSelectPixel sel{{depth, mask, mask_elem_bytes, V, H, W, depth_max}, stride};
    L2D_LAUNCH_IN_SCOPE(s, ds_count_kernel<DsSelectPixel>, dim3((unsigned)nb), dim3(256), 0, sel, n, cnt);
    L2D_LAUNCH_IN_SCOPE(s, ds_offsets_kernel, dim3(1), dim3(256), 0, cnt, nb, total);
    long long host = 0;      // the call's one host read
    L2D_HIP(hipMemcpyAsync(&host, total, sizeof(host), hipMemcpyDeviceToHost, s));
    L2D_HIP(hipStreamSynchronize(s));
    *n_points = host;
    return LARA2DGS_OK;
}

int lara_depthsurface_backproject_emit(int32_t V, int32_t H, int32_t W, const float *depth, const void *mask, int32_t mask_elem_bytes,
                                       int32_t stride, float depth_max, const float *ixt, const float *pose, int32_t normal_mode,
                                       const float *normal_map, float jump, float *points, float *normals, int32_t *pixel,
                                       void *workspace, void *stream) {
    if (!ds_maps_ok(V, H, W) || !ds_mask_ok(mask, mask_elem_bytes) || stride < 1 || std::isnan(depth_max)) return LARA2DGS_E_INVALID;
    if (normal_mode < LARA_DEPTHSURFACE_NORMALS_NONE || normal_mode > LARA_DEPTHSURFACE_NORMALS_DEPTH) return LARA2DGS_E_INVALID;
    if (!depth || !ixt || !pose || !points || !pixel || !workspace) return LARA2DGS_E_INVALID;
    if (normal_mode != LARA_DEPTHSURFACE_NORMALS_NONE && !normals) return LARA2DGS_E_INVALID;
    if (normal_mode == LARA_DEPTHSURFACE_NORMALS_GIVEN && !normal_map) return LARA2DGS_E_INVALID;
    if (normal_mode == LARA_DEPTHSURFACE_NORMALS_DEPTH && !(jump >= 0.0f)) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const long long n = (long long)V * H * W;
    const DsMaps m{depth, mask, mask_elem_bytes, V, H, W, depth_max};
    const DsSelectPixel sel{m, stride};
    const DsEmitPixel emit{m, ixt, pose, normal_map, normal_mode, jump, points, normals, pixel};
    L2D_LAUNCH_IN_SCOPE(s, (ds_emit_kernel<DsSelectPixel, DsEmitPixel>), dim3((unsigned)ds_compaction_blocks(n)), dim3(256), 0, sel, emit, n,
                        (const unsigned *)((char *)workspace + 256));
    return LARA2DGS_OK;
}

int64_t lara_depthsurface_thin_workspace_bytes(int32_t N, int32_t max_cells) {
    if (N < 0 || max_cells < 1 || max_cells > LARA_DEPTHSURFACE_MAX_CELLS) return LARA2DGS_E_INVALID;
    return ds_thin_ws(N, max_cells).total;
}

int lara_depthsurface_thin(int32_t N, const float *points, const float *normals, float voxel, int32_t max_cells, int32_t *kept_index,
                           float *out_points, float *out_normals, int64_t *counts, void *workspace, void *stream) {
    if (N < 0 || max_cells < 1 || max_cells > LARA_DEPTHSURFACE_MAX_CELLS || !(voxel > 0.0f) || !(voxel < INFINITY) || !counts)
        return LARA2DGS_E_INVALID;
    counts[0] = counts[1] = 0;
    if (N == 0) return LARA2DGS_OK;
    if (!points || !kept_index || !out_points || !workspace || (normals && !out_normals)) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const DsThinWs w = ds_thin_ws(N, max_cells);
    char *ws = (char *)workspace;
    DsGridRec *rec = (DsGridRec *)(ws + w.rec);
    long long *res = (long long *)(ws + w.res);
    unsigned *cnt = (unsigned *)(ws + w.cnt);
    int *cells = (int *)(ws + w.cells);
    const unsigned pb = (unsigned)((N + 255) / 256);
    const int nb = ds_compaction_blocks(N);
    L2D_HIP(hipMemsetAsync(rec, 0xff, 24, s));                                  // keys: all bits; max cells: -1
    L2D_HIP(hipMemsetAsync((char *)rec + 24, 0, sizeof(DsGridRec) - 24, s));    // dropped
    L2D_LAUNCH_IN_SCOPE(s, ds_thin_lo_kernel, dim3(pb), dim3(256), 0, N, points, rec);
    L2D_LAUNCH_IN_SCOPE(s, ds_thin_cmax_kernel, dim3(pb), dim3(256), 0, N, points, voxel, rec);
    L2D_LAUNCH_IN_SCOPE(s, ds_thin_fill_kernel, dim3(DS_FILL_BLOCKS), dim3(256), 0, (const DsGridRec *)rec, max_cells, cells);
    L2D_LAUNCH_IN_SCOPE(s, ds_thin_min_kernel, dim3(pb), dim3(256), 0, N, points, voxel, (const DsGridRec *)rec, max_cells, cells);
    const DsSelectWinner sel{points, voxel, rec, max_cells, cells};
    const DsEmitRow emit{points, normals, kept_index, out_points, out_normals};
    L2D_LAUNCH_IN_SCOPE(s, ds_count_kernel<DsSelectWinner>, dim3((unsigned)nb), dim3(256), 0, sel, (long long)N, cnt);
    L2D_LAUNCH_IN_SCOPE(s, ds_offsets_kernel, dim3(1), dim3(256), 0, cnt, nb, res);
    L2D_LAUNCH_IN_SCOPE(s, (ds_emit_kernel<DsSelectWinner, DsEmitRow>), dim3((unsigned)nb), dim3(256), 0, sel, emit, (long long)N,
                        (const unsigned *)cnt);
    L2D_LAUNCH_IN_SCOPE(s, ds_thin_finish, dim3(1), dim3(1), 0, (const DsGridRec *)rec, max_cells, res);
    long long host[3] = {0, 0, 0};      // the call's one host read
    L2D_HIP(hipMemcpyAsync(host, res, sizeof(host), hipMemcpyDeviceToHost, s));
    L2D_HIP(hipStreamSynchronize(s));
    if (host[2] != 0) return LARA2DGS_E_INVALID;
    counts[0] = host[0];
    counts[1] = host[1];
    return LARA2DGS_OK;
}

int lara_depthsurface_observe(int32_t N, const float *points, int32_t V, int32_t H, int32_t W, const float *depth, const void *mask,
                              int32_t mask_elem_bytes, float depth_max, const float *ixt, const float *pose, float tau,
                              int32_t background_is_free, int64_t *seen, void *stream) {
    if (N < 0 || !ds_maps_ok(V, H, W) || !ds_mask_ok(mask, mask_elem_bytes) || std::isnan(depth_max) || !(tau >= 0.0f)) return LARA2DGS_E_INVALID;
    if (N == 0) return LARA2DGS_OK;
    if (!points || !depth || !ixt || !pose || !seen) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const DsMaps m{depth, mask, mask_elem_bytes, V, H, W, depth_max};
    L2D_LAUNCH_IN_SCOPE(s, ds_observe_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, N, points, m, ixt, pose, tau,
                        background_is_free, (long long *)seen);
    return LARA2DGS_OK;
}

int64_t lara_depthsurface_reduce_workspace_bytes(int32_t N) {
    if (N < 0) return LARA2DGS_E_INVALID;
    const int64_t blocks = ((int64_t)N + 255) / 256;
    return align_up(blocks * DS_RQ * 8 + 8, 256) + align_up(blocks * DS_RC * 4 + 4, 256);
}

int lara_depthsurface_reduce(int32_t N, int32_t M, const float *dist, const int32_t *index, const uint8_t *keep, const float *normals_q,
                             const float *normals_t, int32_t n_thr, const float *thresholds, double *row, void *workspace,
                             void *stream) {
    if (N < 0 || M < 0 || !row || n_thr < 0 || n_thr > LARA_DEPTHSURFACE_MAX_THRESHOLDS || (n_thr > 0 && !thresholds)) return LARA2DGS_E_INVALID;
    if ((normals_q == nullptr) != (normals_t == nullptr)) return LARA2DGS_E_INVALID;
    if (N > 0 && (!dist || !index || !workspace)) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const int blocks = (N + 255) / 256;
    double *part = (double *)workspace;
    unsigned *cnt = (unsigned *)((char *)workspace + align_up((int64_t)blocks * DS_RQ * 8 + 8, 256));
    DsThr thr;
    thr.n = n_thr;
    for (int k = 0; k < LARA_DEPTHSURFACE_MAX_THRESHOLDS; k++) thr.v[k] = k < n_thr ? thresholds[k] : 0.0f;
    if (blocks > 0)
        L2D_LAUNCH_IN_SCOPE(s, ds_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, N, M, dist, index, (const unsigned char *)keep, normals_q,
                            normals_t, thr, part, cnt);
    L2D_LAUNCH_IN_SCOPE(s, ds_reduce_finish, dim3(1), dim3(256), 0, blocks, (const double *)part, (const unsigned *)cnt, row);
    return LARA2DGS_OK;
}

}  // extern "C"
