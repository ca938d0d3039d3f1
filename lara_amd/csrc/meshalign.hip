// meshalign.hip -- the device side of ICP on gfx950: the transform of a point set by a 3x4 similarity and the one-pass reduction
// of N correspondences to the 48-double row the host solves one iteration from.  Interface, the sequences and the summation order
// in include/lara_meshalign.h.
//
//   ma_transform_kernel     one thread per row: points and (optionally) normals, in double, one rounding to fp32
//   ma_accumulate_kernel    one pair per lane; every one of the 46 sums is butterflied as soon as its term exists, so a lane never
//                           holds the row: the live state is p, q, n, J (18 doubles), not 46 sums
//   ma_accumulate_finish    one workgroup: the partials in a fixed order, the counts as integers (rowsum.h, like the wave and
//                           workgroup steps of ma_accumulate_kernel)
// Every hand-off between workgroups is a launch boundary.  No atomics.  Built with -ffp-contract=off.
#include "common.h"
#include "wave.h"
#include "rowsum.h"
#include "../../include/lara_meshalign.h"

#include <cmath>

namespace {

constexpr int MA_SUMS = LARA_MESHALIGN_ROW - 2;                            // double partials per workgroup: row entries 1 .. 46
constexpr int64_t MA_MAX_POINTS = 1ll << 30;

struct MaAffine { double a[12]; double inv_scale; };
struct MaOrigin { double o[3]; };

__global__ void __launch_bounds__(256)
ma_transform_kernel(const int N, const float *points, const float *normals, const MaAffine A, float *out_points, float *out_normals) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const size_t o = 3 * (size_t)i;
    const double x = (double)points[o], y = (double)points[o + 1], z = (double)points[o + 2];
    double nx = 0.0, ny = 0.0, nz = 0.0;
    if (normals) { nx = (double)normals[o]; ny = (double)normals[o + 1]; nz = (double)normals[o + 2]; }
#pragma unroll
    for (int k = 0; k < 3; k++) out_points[o + k] = (float)(((A.a[4 * k] * x + A.a[4 * k + 1] * y) + A.a[4 * k + 2] * z) + A.a[4 * k + 3]);
    if (normals) {
#pragma unroll
        for (int k = 0; k < 3; k++) out_normals[o + k] = (float)(((A.a[4 * k] * nx + A.a[4 * k + 1] * ny) + A.a[4 * k + 2] * nz) * A.inv_scale);
    }
}

// part[block][46] = the workgroup's sums of row entries 1 .. 46; cnt[block][2] = pairs kept, kept pairs with a normal
__global__ void __launch_bounds__(256)
ma_accumulate_kernel(const int N, const int M, const int K, const float *__restrict__ src, const float *__restrict__ tgt,
                     const int *__restrict__ index, const float *__restrict__ normals, const int *__restrict__ nindex,
                     const float *__restrict__ dist, const float max_dist, const MaOrigin org, double *__restrict__ part,
                     unsigned *__restrict__ cnt) {
    __shared__ double red[MA_SUMS][4];
    __shared__ int redc[2][4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool keep = false, has_n = false;
    double p[3] = {0.0, 0.0, 0.0}, q[3] = {0.0, 0.0, 0.0}, n[3] = {0.0, 0.0, 0.0};
    if (i < N) {
        const int j = index ? index[i] : i;
        const float d = dist[i];
        keep = j >= 0 && j < M && fabsf(d) < INFINITY && d <= max_dist;
        if (keep) {
#pragma unroll
            for (int a = 0; a < 3; a++) {
                p[a] = (double)src[3 * (size_t)i + a] - org.o[a];
                q[a] = (double)tgt[3 * (size_t)j + a] - org.o[a];
            }
            if (normals) {
                const int k = nindex[i];
                if (k >= 0 && k < K) {
                    const float f0 = normals[3 * (size_t)k], f1 = normals[3 * (size_t)k + 1], f2 = normals[3 * (size_t)k + 2];
                    has_n = fabsf(f0) < INFINITY && fabsf(f1) < INFINITY && fabsf(f2) < INFINITY && (f0 != 0.0f || f1 != 0.0f || f2 != 0.0f);
                    if (has_n) { n[0] = (double)f0; n[1] = (double)f1; n[2] = (double)f2; }
                }
            }
        }
    }
    // a term of row entry `entry`: +0 from a lane that does not contribute, the butterfly, the wave's slot
    const auto emit = [&](const int entry, const bool on, const double term) { rowsum_wave(red[entry - 1], on ? term : 0.0); };
    const double d[3] = {p[0] - q[0], p[1] - q[1], p[2] - q[2]};
    emit(1, keep, (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
#pragma unroll
    for (int a = 0; a < 3; a++) {
        emit(2 + a, keep, p[a]);
        emit(5 + a, keep, q[a]);
#pragma unroll
        for (int b = 0; b < 3; b++) emit(8 + 3 * a + b, keep, p[a] * q[b]);
    }
    emit(17, keep, (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]);
    emit(18, keep, (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
    const double J[6] = {p[1] * n[2] - p[2] * n[1], p[2] * n[0] - p[0] * n[2], p[0] * n[1] - p[1] * n[0], n[0], n[1], n[2]};
    const double r = (d[0] * n[0] + d[1] * n[1]) + d[2] * n[2];
    int e = 19;
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int b = a; b < 6; b++) emit(e++, has_n, J[a] * J[b]);
#pragma unroll
    for (int a = 0; a < 6; a++) emit(40 + a, has_n, J[a] * r);
    emit(46, has_n, r * r);
    rowsum_wave(redc[0], keep ? 1 : 0);
    rowsum_wave(redc[1], has_n ? 1 : 0);
    rowsum_block_partial(red, redc, part, cnt);
}

// row: the sums -> [1 .. 46]; pairs kept -> [0], kept pairs with a normal -> [47]
__global__ void __launch_bounds__(256)
ma_accumulate_finish(const int blocks, const double *__restrict__ part, const unsigned *__restrict__ cnt, double *__restrict__ row) {
    rowsum_finish<MA_SUMS, 2>(blocks, part, cnt, [&](const int q, const double v) { row[1 + q] = v; },
                              [&](const int q, const double v) { row[q == 0 ? 0 : LARA_MESHALIGN_ROW - 1] = v; });
}

int64_t ma_part_bytes(const int64_t blocks) { return align_up(blocks * MA_SUMS * 8 + 8, 256); }

}  // namespace

extern "C" {

int lara_meshalign_transform(int32_t N, const float *points, const float *normals, const double *A, double inv_scale,
                             float *out_points, float *out_normals, void *stream) {
    if (N < 0 || N >= MA_MAX_POINTS || !A) return LARA2DGS_E_INVALID;
    if (N == 0) return LARA2DGS_OK;
    if (!points || !out_points || (normals && !out_normals)) return LARA2DGS_E_INVALID;
    MaAffine a;
    for (int k = 0; k < 12; k++) a.a[k] = A[k];
    a.inv_scale = inv_scale;
    L2D_LAUNCH_IN_SCOPE((hipStream_t)stream, ma_transform_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, N, points, normals, a,
                        out_points, out_normals);
    return LARA2DGS_OK;
}

int64_t lara_meshalign_accumulate_workspace_bytes(int32_t N) {
    if (N < 0 || N >= MA_MAX_POINTS) return LARA2DGS_E_INVALID;
    const int64_t blocks = ((int64_t)N + 255) / 256;
    return ma_part_bytes(blocks) + align_up(blocks * 2 * 4 + 4, 256);
}

int lara_meshalign_accumulate(int32_t N, int32_t M, int32_t K, const float *src, const float *tgt, const int32_t *index,
                              const float *normals, const int32_t *nindex, const float *dist, float max_dist, const double *origin,
                              double *row, void *workspace, void *stream) {
    if (N < 0 || N >= MA_MAX_POINTS || M < 0 || M >= MA_MAX_POINTS || K < 0 || K >= MA_MAX_POINTS || !row || !origin) return LARA2DGS_E_INVALID;
    if ((normals == nullptr) != (nindex == nullptr)) return LARA2DGS_E_INVALID;
    if (!index && M != N) return LARA2DGS_E_INVALID;
    if (N > 0 && (!src || !tgt || !dist || !workspace)) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const int blocks = (N + 255) / 256;
    double *part = (double *)workspace;
    unsigned *cnt = (unsigned *)((char *)workspace + ma_part_bytes(blocks));
    MaOrigin org;
    for (int a = 0; a < 3; a++) org.o[a] = origin[a];
    if (blocks > 0)
        L2D_LAUNCH_IN_SCOPE(s, ma_accumulate_kernel, dim3((unsigned)blocks), dim3(256), 0, N, M, K, src, tgt, index, normals, nindex, dist,
                            max_dist, org, part, cnt);
    L2D_LAUNCH_IN_SCOPE(s, ma_accumulate_finish, dim3(1), dim3(256), 0, blocks, (const double *)part, (const unsigned *)cnt, row);
    return LARA2DGS_OK;
}

}  // extern "C"
