// unigrid.h -- what the two uniform-grid searches share (meshmetrics.hip: nearest point; meshdist.hip: nearest triangle): the grid
// record and the wave that derives it from a bounding box, the cell rule, the Chebyshev ring walk with its bound (mm_rings), the
// resolution rule and the three-launch inclusive scan.  The box reduction and the candidate are trimesh.h's.  The rules are stated
// in include/lara_meshmetrics.h.  Everything sits in an unnamed namespace: each unit that includes this header owns
// its copies.  Include it from units built with -ffp-contract=off only.
#pragma once
#include "common.h"
#include "wave.h"
#include "trimesh.h"

#include <cmath>

namespace {

constexpr int MM_SCAN_ITEMS = 4, MM_SCAN_BLOCK = 256 * MM_SCAN_ITEMS;      // elements per workgroup of the scan
constexpr int MM_BOUNDS_BLOCKS = 1024;
constexpr float MM_MARGIN = 3.814697265625e-06f;                           // 2^-18
constexpr int MM_MAX_GRID = 256;

struct MmGrid {
    float lo[3];
    float h, inv_h, ext;      // cell edge, its reciprocal, R h
    int R[3];
};

// inclusive scan of 1024 elements per workgroup; bsum[block] = the workgroup's total
template <class T>
__global__ void __launch_bounds__(256)
mm_scan_block(const T *__restrict__ in, T *__restrict__ out, T *__restrict__ bsum, const long long n) {
    __shared__ T wtot[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long base = ((long long)blockIdx.x * 256 + tid) * MM_SCAN_ITEMS;
    T v[MM_SCAN_ITEMS];
#pragma unroll
    for (int k = 0; k < MM_SCAN_ITEMS; k++) v[k] = base + k < n ? in[base + k] : (T)0;
#pragma unroll
    for (int k = 1; k < MM_SCAN_ITEMS; k++) v[k] += v[k - 1];
    const T incl = wave_inclusive_scan(v[MM_SCAN_ITEMS - 1], lane);
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    T off = incl - v[MM_SCAN_ITEMS - 1];
    for (int w = 0; w < wave; w++) off += wtot[w];
#pragma unroll
    for (int k = 0; k < MM_SCAN_ITEMS; k++)
        if (base + k < n) out[base + k] = v[k] + off;
    if (tid == 255) bsum[blockIdx.x] = v[MM_SCAN_ITEMS - 1] + off;
}

// in place: bsum[i] <- bsum[0] + ... + bsum[i]; one workgroup, 256 sums at a time with a carry
template <class T>
__global__ void __launch_bounds__(256)
mm_scan_sums(T *__restrict__ bsum, const int nb) {
    __shared__ T wtot[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    T carry = (T)0;
    for (int c0 = 0; c0 < nb; c0 += 256) {
        const int i = c0 + tid;
        const T v = i < nb ? bsum[i] : (T)0;
        const T incl = wave_inclusive_scan(v, lane);
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        T off = carry;
        for (int w = 0; w < wave; w++) off += wtot[w];
        if (i < nb) bsum[i] = incl + off;
        carry += ((wtot[0] + wtot[1]) + wtot[2]) + wtot[3];
        __syncthreads();
    }
}

template <class T>
__global__ void __launch_bounds__(256)
mm_scan_add(T *__restrict__ out, const T *__restrict__ bsum, const long long n) {
    if (blockIdx.x == 0) return;
    const T off = bsum[blockIdx.x - 1];
    const long long base = ((long long)blockIdx.x * 256 + threadIdx.x) * MM_SCAN_ITEMS;
#pragma unroll
    for (int k = 0; k < MM_SCAN_ITEMS; k++)
        if (base + k < n) out[base + k] += off;
}

template <class T>
int mm_scan(const T *in, T *out, T *bsum, const long long n, hipStream_t s) {
    const int nb = (int)((n + MM_SCAN_BLOCK - 1) / MM_SCAN_BLOCK);
    L2D_LAUNCH_IN_SCOPE(s, mm_scan_block<T>, dim3((unsigned)nb), dim3(256), 0, in, out, bsum, n);
    if (nb > 1) {
        L2D_LAUNCH_IN_SCOPE(s, mm_scan_sums<T>, dim3(1), dim3(256), 0, bsum, nb);
        L2D_LAUNCH_IN_SCOPE(s, mm_scan_add<T>, dim3((unsigned)nb), dim3(256), 0, out, (const T *)bsum, n);
    }
    return LARA2DGS_OK;
}

// one wave: the box of all partials (part[block][6] = min x y z, max x y z) -> the grid record
__global__ void __launch_bounds__(64)
mm_bounds_finish(const int blocks, const float *__restrict__ part, const int R, MmGrid *__restrict__ grid) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    box_gather_partials(blocks, part, lo, hi);
    if (threadIdx.x != 0) return;
    MmGrid g;
    float ext[3], emax = 0.0f;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const bool fin = fabsf(lo[j]) < INFINITY && fabsf(hi[j]) < INFINITY;      // (false: every coordinate of the axis is a NaN or infinite)
        g.lo[j] = fin ? lo[j] : 0.0f;
        ext[j] = fin ? hi[j] - lo[j] : 0.0f;
        emax = fmaxf(emax, ext[j]);
    }
    float h = 1.0f, inv_h = 1.0f;
    if (emax > 0.0f && emax < INFINITY) {
        const float hh = emax / (float)R, ii = 1.0f / hh;
        if (hh > 0.0f && ii < INFINITY) { h = hh; inv_h = ii; }
    }
    g.h = h;
    g.inv_h = inv_h;
    g.ext = (float)R * h;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const float f = ext[j] * inv_h;
        g.R[j] = (f >= 0.0f && f < (float)R) ? min((int)f + 1, R) : (f >= (float)R ? R : 1);
    }
    *grid = g;
}

__device__ __forceinline__ int mm_cell_axis(const float u_scaled, const int Ra) {      // clamp(floor(u), 0, Ra - 1); a NaN -> 0
    const float f = floorf(u_scaled);
    return f >= 0.0f ? (f < (float)Ra ? (int)f : Ra - 1) : 0;
}

// of a query at u = q - g.lo: its cell, and the margin its bound gives away to the rounding of u and of the cells' faces
__device__ __forceinline__ void mm_locate(const MmGrid &g, const float u[3], int c[3]) {
#pragma unroll
    for (int a = 0; a < 3; a++) c[a] = mm_cell_axis(u[a] * g.inv_h, g.R[a]);
}
__device__ __forceinline__ float mm_margin(const MmGrid &g, const float u[3]) {
    return fmaxf(fmaxf(fabsf(u[0]), fabsf(u[1])), fmaxf(fabsf(u[2]), g.ext)) * MM_MARGIN;
}

// The Chebyshev ring search around cell c: ring r = the cells at Chebyshev distance r, as contiguous runs of one x row handed to
// visit(c0, c1); after each ring accept(bound) says whether the caller's candidate is nearer than `bound`, the distance from the
// query to the nearest face of the cube of rings 0 .. r that is not a face of the grid, less the margin.  true: accepted within
// rings 0 .. rmax
template <class Visit, class Accept>
__device__ __forceinline__ bool mm_rings(const MmGrid &g, const float u[3], const int c[3], const int rmax, Visit visit, Accept accept) {
    const float margin = mm_margin(g, u);
    bool done = false;
    for (int r = 0; r <= rmax && !done; r++) {
        const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, g.R[2] - 1), y0 = max(c[1] - r, 0), y1 = min(c[1] + r, g.R[1] - 1);
        const int xa = max(c[0] - r, 0), xb = min(c[0] + r, g.R[0] - 1);
        for (int z = z0; z <= z1; z++)
            for (int y = y0; y <= y1; y++) {
                const int row = (z * g.R[1] + y) * g.R[0];
                if (z == c[2] - r || z == c[2] + r || y == c[1] - r || y == c[1] + r) visit(row + xa, row + xb);
                else {      // (r > 0 here) the ring's two cells of an inner row
                    if (c[0] - r >= 0) visit(row + c[0] - r, row + c[0] - r);
                    if (c[0] + r < g.R[0]) visit(row + c[0] + r, row + c[0] + r);
                }
            }
        float gap = INFINITY;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            if (c[a] - r > 0) gap = fminf(gap, u[a] - (float)(c[a] - r) * g.h);
            if (c[a] + r + 1 < g.R[a]) gap = fminf(gap, (float)(c[a] + r + 1) * g.h - u[a]);
        }
        done = accept(fmaxf(0.0f, gap - margin));
    }
    return done;
}

int mm_resolution(const int64_t M) {
    int R = (int)std::ceil(std::sqrt((double)M / 4.0));
    return R < 1 ? 1 : (R > MM_MAX_GRID ? MM_MAX_GRID : R);
}

}  // namespace
