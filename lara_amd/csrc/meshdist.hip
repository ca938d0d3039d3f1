// meshdist.hip -- exact point-to-triangle distances on gfx950: a uniform grid over a mesh's triangles, the ring search of
// meshmetrics.hip carried over from points to triangles, and a brute-force kernel for the queries the rings do not settle.
// Interface, the grid rule, the cover argument and the tie rule in include/lara_meshdist.h; the distance itself in tridist.h;
// the record, the validity rule, the box reduction, the candidate and the result write in trimesh.h, shared with meshbvh.hip.
//
//   md_pack_kernel                          48-byte records {p0, p1, p2, id or -1}; the box of the valid triangles; the bad count
//   mm_bounds_finish (unigrid.h)            the box -> the grid record
//   md_count_kernel                         per triangle: the cells its box overlaps -> integer atomic histogram, or the large flag
//   mm_scan (unigrid.h)                     the cells' ends; the large triangles' positions (an ordered compaction)
//   md_scatter_kernel / md_finish_kernel    cursor scatter of the triangle ids; the large list; the header's counts
//   md_query_kernel                         one thread per query: the large list, then mm_rings (unigrid.h) until the bound accepts
//   md_brute_kernel                         a workgroup per listed query: all records, tiled through LDS
//   md_normals_kernel                       unit face normals
// Every hand-off between workgroups is a launch boundary.  The only atomics are integer ones (histogram, cursors, list length, bad
// count); no result depends on their order.  Built with -ffp-contract=off.
#include "common.h"
#include "unigrid.h"
#include "tridist.h"
#include "../../include/lara_meshdist.h"

#include <cmath>

namespace {

constexpr int MD_RMAX = LARA_MESHDIST_RMAX, MD_SPAN = LARA_MESHDIST_MAX_SPAN;
constexpr int MD_PAIRS = MD_SPAN * MD_SPAN * MD_SPAN;      // (triangle, cell) pairs of a triangle outside the large list, at most
constexpr int MD_TILE = 256;                               // records per LDS tile of the brute-force kernel
constexpr int64_t MD_MAX_TRIANGLES = 1ll << 26, MD_MAX_POINTS = 1ll << 30;      // (64 T pairs stay below 2^32)

// byte offsets into the caller's grid buffer: functions of T alone
struct MdLayout { int64_t rec, part, hist, end, bsum, flag, lpos, bsum_l, large, pairs, total; };

struct MdHeader {
    int count[LARA_MESHDIST_HEADER_INTS];      // LARA_MESHDIST_HDR_*
    MmGrid g;
    MdLayout L;
};
static_assert(sizeof(MdHeader) <= 256, "the header's slot");

MdLayout md_layout(const int64_t T) {
    const int64_t R = mm_resolution(T), C = R * R * R;
    MdLayout w;
    int64_t o = 256;
    w.rec = o;     o = align_up(o + T * 48, 256);
    w.part = o;    o = align_up(o + MM_BOUNDS_BLOCKS * 6 * 4, 256);
    w.hist = o;    o = align_up(o + C * 4, 256);
    w.end = o;     o = align_up(o + C * 4, 256);
    w.bsum = o;    o = align_up(o + ((C + MM_SCAN_BLOCK - 1) / MM_SCAN_BLOCK + 1) * 4, 256);
    w.flag = o;    o = align_up(o + T * 4, 256);
    w.lpos = o;    o = align_up(o + T * 4, 256);
    w.bsum_l = o;  o = align_up(o + ((T + MM_SCAN_BLOCK - 1) / MM_SCAN_BLOCK + 1) * 4, 256);
    w.large = o;   o = align_up(o + T * 4, 256);
    w.pairs = o;   o = align_up(o + T * MD_PAIRS * 4, 256);
    w.total = o;
    return w;
}

// rec[i] and part[block][6] = min x y z, max x y z of the valid triangles the workgroup strides over.  Valid: tri_fetch's rule;
// the others get id = -1, zero coordinates, and are counted
__global__ void __launch_bounds__(256)
md_pack_kernel(const int Nv, const int T, const float *__restrict__ v, const int *__restrict__ t, float4 *__restrict__ rec,
               float *__restrict__ part, int *__restrict__ bad) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < T; i += (long long)gridDim.x * 256) {
        float p[3][3];
        const bool ok = tri_fetch(Nv, v, t, i, p);
        if (!ok) atomicAdd(bad, 1);
        else box_grow(lo, hi, p);
        tri_store(rec, (size_t)i, p, ok ? (int)i : -1);
    }
    box_block_partial(lo, hi, part);
}

// the cells c0 .. c1 (per axis) between the cell of the box's minimum corner and the cell of its maximum corner: the cell rule is
// monotone, so every point of the triangle falls into one of them.  true: the box spans more than MD_SPAN cells on some axis
__device__ __forceinline__ bool md_cells(const MmGrid &g, const TriRec &r, int c0[3], int c1[3]) {
    bool large = false;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float mn = fminf(fminf(r.p[0][a], r.p[1][a]), r.p[2][a]), mx = fmaxf(fmaxf(r.p[0][a], r.p[1][a]), r.p[2][a]);
        c0[a] = mm_cell_axis((mn - g.lo[a]) * g.inv_h, g.R[a]);
        c1[a] = mm_cell_axis((mx - g.lo[a]) * g.inv_h, g.R[a]);
        large = large || c1[a] - c0[a] + 1 > MD_SPAN;
    }
    return large;
}

__global__ void __launch_bounds__(256)
md_count_kernel(const int T, const float4 *__restrict__ rec, const MdHeader *__restrict__ hdr, unsigned *__restrict__ hist,
                unsigned *__restrict__ flag) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= T) return;
    const TriRec r = tri_load(rec, i);
    unsigned f = 0u;
    if (r.id >= 0) {
        const MmGrid g = hdr->g;
        int c0[3], c1[3];
        if (md_cells(g, r, c0, c1)) f = 1u;
        else
            for (int z = c0[2]; z <= c1[2]; z++)
                for (int y = c0[1]; y <= c1[1]; y++)
                    for (int x = c0[0]; x <= c1[0]; x++) atomicAdd(&hist[(z * g.R[1] + y) * g.R[0] + x], 1u);
    }
    flag[i] = f;
}

// the histogram counts back down to zero: slot = the cell's start + (count before this pair) - 1; a large triangle goes to the slot
// the scan of the flags gives it, so the large list is in increasing triangle order
__global__ void __launch_bounds__(256)
md_scatter_kernel(const int T, const float4 *__restrict__ rec, const MdHeader *__restrict__ hdr, unsigned *__restrict__ hist,
                  const unsigned *__restrict__ end, const unsigned *__restrict__ flag, const unsigned *__restrict__ lpos,
                  int *__restrict__ large, int *__restrict__ pairs) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= T) return;
    if (flag[i]) {
        const unsigned pos = lpos[i] - 1u;
        if (pos < (unsigned)T) large[pos] = i;
        return;
    }
    const TriRec r = tri_load(rec, i);
    if (r.id < 0) return;
    const MmGrid g = hdr->g;
    int c0[3], c1[3];
    md_cells(g, r, c0, c1);
    const unsigned long long cap = (unsigned long long)T * MD_PAIRS;
    for (int z = c0[2]; z <= c1[2]; z++)
        for (int y = c0[1]; y <= c1[1]; y++)
            for (int x = c0[0]; x <= c1[0]; x++) {
                const int c = (z * g.R[1] + y) * g.R[0] + x;
                const unsigned start = c ? end[c - 1] : 0u;
                const unsigned pos = start + (atomicSub(&hist[c], 1u) - 1u);
                if (pos < cap) pairs[pos] = i;
            }
}

__global__ void md_finish_kernel(MdHeader *__restrict__ hdr, const MdLayout L, const int T, const long long C,
                                 const unsigned *__restrict__ lpos, const unsigned *__restrict__ end) {
    hdr->count[LARA_MESHDIST_HDR_LARGE] = (int)lpos[T - 1];
    hdr->count[LARA_MESHDIST_HDR_PAIRS] = (int)end[C - 1];
    hdr->count[LARA_MESHDIST_HDR_TRIANGLES] = T;
    hdr->L = L;
}

__device__ __forceinline__ double md_d2(const float q[3], const TriRec &r, double c[3]) { return lara_tridist(q, r.p[0], r.p[1], r.p[2], c); }

__global__ void __launch_bounds__(256)
md_query_kernel(const int N, const float *__restrict__ q, const char *__restrict__ grid, float *__restrict__ dist,
                int *__restrict__ face, float *__restrict__ closest, int *__restrict__ list, unsigned *__restrict__ count) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const MdHeader *hdr = (const MdHeader *)grid;
    const MmGrid g = hdr->g;
    const int T = hdr->count[LARA_MESHDIST_HDR_TRIANGLES], n_large = min(hdr->count[LARA_MESHDIST_HDR_LARGE], T);
    const float4 *rec = (const float4 *)(grid + hdr->L.rec);
    const unsigned *end = (const unsigned *)(grid + hdr->L.end);
    const int *large = (const int *)(grid + hdr->L.large), *pairs = (const int *)(grid + hdr->L.pairs);
    const unsigned long long cap = (unsigned long long)T * MD_PAIRS;
    const float qf[3] = {q[3 * (size_t)i], q[3 * (size_t)i + 1], q[3 * (size_t)i + 2]};
    Nearest<double> best{INFINITY, NEAREST_NONE};
    if (!(fabsf(qf[0]) < INFINITY && fabsf(qf[1]) < INFINITY && fabsf(qf[2]) < INFINITY)) {      // a non-finite query: no candidate
        tri_write_result(i, qf, best, rec, best.id, dist, face, closest);
        return;
    }
    const auto test = [&](const int id) {
        if ((unsigned)id >= (unsigned)T) return;
        double c[3];
        best.take(md_d2(qf, tri_load(rec, id), c), id);
    };
    for (int j = 0; j < n_large; j++) test(large[j]);
    const float u[3] = {qf[0] - g.lo[0], qf[1] - g.lo[1], qf[2] - g.lo[2]};
    int c[3];
    mm_locate(g, u, c);
    // the pairs of the cells c0 .. c1 of one x row are contiguous; at most 64 T of them (the guard costs nothing)
    const auto visit = [&](const int c0, const int c1) {
        const unsigned s = c0 ? end[c0 - 1] : 0u;
        const unsigned e = (unsigned)min((unsigned long long)end[c1], cap);
        for (unsigned j = s; j < e; j++) test(pairs[j]);
    };
    const auto accept = [&](const float bound) { return best.d2 < (double)bound * (double)bound; };
    // a record's position in the grid's buffer is its id
    if (mm_rings(g, u, c, MD_RMAX, visit, accept)) tri_write_result(i, qf, best, rec, best.id, dist, face, closest);
    else list[atomicAdd(count, 1u)] = i;
}

// a workgroup per listed query: all T records in tiles of 256 (768 float4, loaded coalesced); a thread meets its triangles in
// increasing id, so `<` alone keeps the smaller id inside a thread; across threads the tie rule is explicit
__global__ void __launch_bounds__(256)
md_brute_kernel(const float *__restrict__ q, const char *__restrict__ grid, const int *__restrict__ list,
                const unsigned *__restrict__ count, float *__restrict__ dist, int *__restrict__ face, float *__restrict__ closest,
                int *__restrict__ fallback_count) {
    __shared__ float4 tile[3 * MD_TILE];
    __shared__ double wd[4];
    __shared__ int wi[4];
    const int tid = threadIdx.x;
    const unsigned n_listed = *count;
    if (blockIdx.x == 0 && tid == 0 && fallback_count) *fallback_count = (int)n_listed;
    if (blockIdx.x >= n_listed) return;
    const MdHeader *hdr = (const MdHeader *)grid;
    const int T = hdr->count[LARA_MESHDIST_HDR_TRIANGLES];
    const float4 *rec = (const float4 *)(grid + hdr->L.rec);
    const int qi = list[blockIdx.x];
    const float qf[3] = {q[3 * (size_t)qi], q[3 * (size_t)qi + 1], q[3 * (size_t)qi + 2]};
    Nearest<double> best{INFINITY, NEAREST_NONE};
    const long long words = 3ll * T;
    for (int base = 0; base < T; base += MD_TILE) {
        if (base) __syncthreads();
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const long long f = 3ll * base + tid + 256 * k;
            tile[tid + 256 * k] = f < words ? rec[f] : make_float4(0.0f, __int_as_float(-1), 0.0f, 0.0f);
        }
        __syncthreads();
        if (base + tid < T) {
            const TriRec r = tri_unpack(tile[3 * tid], tile[3 * tid + 1], tile[3 * tid + 2]);
            if (r.id >= 0) {
                double c[3];
                const double d2 = md_d2(qf, r, c);
                if (d2 < best.d2) { best.d2 = d2; best.id = base + tid; }
            }
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) best.take(__shfl_xor(best.d2, d, 64), __shfl_xor(best.id, d, 64));
    if ((tid & 63) == 0) { wd[tid >> 6] = best.d2; wi[tid >> 6] = best.id; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; w++) best.take(wd[w], wi[w]);
        tri_write_result(qi, qf, best, rec, best.id, dist, face, closest);
    }
}

// c / |c| for c = (p1 - p0) x (p2 - p0) in double, stored as fp32; zero where the area is 0 (or not finite) or an index is bad
__global__ void __launch_bounds__(256)
md_normals_kernel(const int Nv, const int T, const float *__restrict__ v, const int *__restrict__ t, float *__restrict__ normals) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= T) return;
    const int id[3] = {t[3 * (size_t)i], t[3 * (size_t)i + 1], t[3 * (size_t)i + 2]};
    double n[3] = {0.0, 0.0, 0.0};
    if (id[0] >= 0 && id[0] < Nv && id[1] >= 0 && id[1] < Nv && id[2] >= 0 && id[2] < Nv) {      // (not tri_fetch's rule: indices only)
        double p[3][3];
#pragma unroll
        for (int k = 0; k < 3; k++)
#pragma unroll
            for (int j = 0; j < 3; j++) p[k][j] = (double)v[3 * (size_t)id[k] + j];
        const double e1[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
        const double e2[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
        const double c[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        const double len = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
        if (len > 0.0 && len < INFINITY) { n[0] = c[0] / len; n[1] = c[1] / len; n[2] = c[2] / len; }
    }
#pragma unroll
    for (int j = 0; j < 3; j++) normals[3 * (size_t)i + j] = (float)n[j];
}

}  // namespace

extern "C" {

int32_t lara_meshdist_grid_resolution(int32_t T) { return T <= 0 ? LARA2DGS_E_INVALID : mm_resolution(T); }

int64_t lara_meshdist_grid_bytes(int32_t T) {
    if (T <= 0 || T >= MD_MAX_TRIANGLES) return LARA2DGS_E_INVALID;
    return md_layout(T).total;
}

int lara_meshdist_build(int32_t Nv, int32_t T, const float *vertices, const int32_t *triangles, void *grid, void *stream) {
    if (T <= 0 || T >= MD_MAX_TRIANGLES || Nv <= 0 || Nv >= MD_MAX_POINTS) return LARA2DGS_E_INVALID;
    if (!vertices || !triangles || !grid) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const MdLayout L = md_layout(T);
    char *base = (char *)grid;
    MdHeader *hdr = (MdHeader *)base;
    float4 *rec = (float4 *)(base + L.rec);
    float *part = (float *)(base + L.part);
    unsigned *hist = (unsigned *)(base + L.hist), *end = (unsigned *)(base + L.end), *bsum = (unsigned *)(base + L.bsum);
    unsigned *flag = (unsigned *)(base + L.flag), *lpos = (unsigned *)(base + L.lpos), *bsum_l = (unsigned *)(base + L.bsum_l);
    int *large = (int *)(base + L.large), *pairs = (int *)(base + L.pairs);
    const int R = mm_resolution(T);
    const long long C = (long long)R * R * R;
    const unsigned tb = (unsigned)((T + 255) / 256);
    const int bb = (int)(tb < (unsigned)MM_BOUNDS_BLOCKS ? tb : (unsigned)MM_BOUNDS_BLOCKS);
    L2D_HIP(hipMemsetAsync(hdr, 0, 256, s));
    L2D_HIP(hipMemsetAsync(hist, 0, (size_t)C * 4, s));
    L2D_LAUNCH_IN_SCOPE(s, md_pack_kernel, dim3((unsigned)bb), dim3(256), 0, Nv, T, vertices, triangles, rec, part,
                        &hdr->count[LARA_MESHDIST_HDR_BAD]);
    L2D_LAUNCH_IN_SCOPE(s, mm_bounds_finish, dim3(1), dim3(64), 0, bb, (const float *)part, R, &hdr->g);
    L2D_LAUNCH_IN_SCOPE(s, md_count_kernel, dim3(tb), dim3(256), 0, T, (const float4 *)rec, (const MdHeader *)hdr, hist, flag);
    L2D_TRY(mm_scan<unsigned>((const unsigned *)hist, end, bsum, C, s));
    L2D_TRY(mm_scan<unsigned>((const unsigned *)flag, lpos, bsum_l, T, s));
    L2D_LAUNCH_IN_SCOPE(s, md_scatter_kernel, dim3(tb), dim3(256), 0, T, (const float4 *)rec, (const MdHeader *)hdr, hist,
                        (const unsigned *)end, (const unsigned *)flag, (const unsigned *)lpos, large, pairs);
    L2D_LAUNCH_IN_SCOPE(s, md_finish_kernel, dim3(1), dim3(1), 0, hdr, L, T, C, (const unsigned *)lpos, (const unsigned *)end);
    return LARA2DGS_OK;
}

int64_t lara_meshdist_query_workspace_bytes(int32_t N) {
    if (N < 0 || N >= MD_MAX_POINTS) return LARA2DGS_E_INVALID;
    return align_up((int64_t)N * 4 + 4, 256) + 256;
}

int lara_meshdist_query(int32_t N, const float *queries, const void *grid, float *dist, int32_t *face, float *closest,
                        int32_t *fallback_count, void *workspace, void *stream) {
    if (N < 0 || N >= MD_MAX_POINTS) return LARA2DGS_E_INVALID;
    if (N == 0) return LARA2DGS_OK;
    if (!queries || !grid || !dist || !face || !workspace) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    int *list = (int *)workspace;
    unsigned *count = (unsigned *)((char *)workspace + align_up((int64_t)N * 4 + 4, 256));
    L2D_HIP(hipMemsetAsync(count, 0, 4, s));
    L2D_LAUNCH_IN_SCOPE(s, md_query_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, N, queries, (const char *)grid, dist, face,
                        closest, list, count);
    L2D_LAUNCH_IN_SCOPE(s, md_brute_kernel, dim3((unsigned)N), dim3(256), 0, queries, (const char *)grid, (const int *)list,
                        (const unsigned *)count, dist, face, closest, fallback_count);
    return LARA2DGS_OK;
}

int lara_meshdist_face_normals(int32_t Nv, int32_t T, const float *vertices, const int32_t *triangles, float *normals, void *stream) {
    if (T <= 0 || T >= MD_MAX_TRIANGLES || Nv <= 0 || Nv >= MD_MAX_POINTS) return LARA2DGS_E_INVALID;
    if (!vertices || !triangles || !normals) return LARA2DGS_E_INVALID;
    L2D_LAUNCH_IN_SCOPE((hipStream_t)stream, md_normals_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, Nv, T, vertices,
                        triangles, normals);
    return LARA2DGS_OK;
}

int lara_meshdist_point_triangle_host(int64_t n, const float *queries, const float *triangles9, double *d2, double *closest) {
    if (n < 0 || (n > 0 && (!queries || !triangles9 || !d2))) return LARA2DGS_E_INVALID;
    for (int64_t i = 0; i < n; ++i) {
        const float *t = triangles9 + 9 * i;
        double c[3];
        d2[i] = lara_tridist(queries + 3 * i, t, t + 3, t + 6, c);
        if (closest) { closest[3 * i] = c[0]; closest[3 * i + 1] = c[1]; closest[3 * i + 2] = c[2]; }
    }
    return LARA2DGS_OK;
}

}  // extern "C"
