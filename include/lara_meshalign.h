/*
 * meshalign/lara_meshalign.h -- the device side of rigid / similarity registration (ICP) of two surfaces: the transform of a point
 * set and the one-pass reduction of N correspondences to the normal equations of one iteration (part of liblara2dgs.so; opt-in,
 * python side: lara_amd/meshalign.py, which owns the correspondences' search -- meshmetrics / meshdist --, the 3x3 and 6x6 solves on
 * the host and the loop; kernels: csrc/meshalign.hip).  All pointers are device pointers unless a parameter says HOST.  Returns 0 or
 * a negative LARA2DGS_E_* code.  Work is enqueued on `stream`; no entry point reads anything back to the host.  Built with
 * -ffp-contract=off: the sequences written here are the instructions.  fp32 inputs, every operation in double.
 *
 * ---- lara_meshalign_transform ---------------------------------------------------------------------------------------------------------
 * points [N][3] f32, normals [N][3] f32 (may be NULL, then out_normals is not used), A: HOST double [12], the row-major 3x4 matrix
 * [sR | t], inv_scale = 1 / s.  For every row (x, y, z) of points and (nx, ny, nz) of normals, k = 0, 1, 2:
 *     out_points[k]  = (float)(((A[4k] x + A[4k+1] y) + A[4k+2] z) + A[4k+3])
 *     out_normals[k] = (float)(((A[4k] nx + A[4k+1] ny) + A[4k+2] nz) inv_scale)
 * one rounding to fp32 each.  A is read before the call returns.  out_points may be points and out_normals may be normals (a thread
 * reads its row before it writes it).  N == 0 is a no-op.  Limit: 0 <= N < 2^30.
 *
 * ---- lara_meshalign_accumulate: N correspondences -> one row of LARA_MESHALIGN_ROW doubles ----------------------------------------------
 * src [N][3] f32; tgt [M][3] f32 with index [N] i32 (index NULL: pair i is (src[i], tgt[i]), which requires M == N); normals [K][3]
 * f32 with nindex [N] i32 (both NULL or both given); dist [N] f32; max_dist; origin: HOST double [3], read before the call returns.
 * Pair i with j = index[i] (or i) is KEPT iff 0 <= j < M, dist[i] is finite and dist[i] <= max_dist (fp32 comparison).  A kept pair
 * HAS A NORMAL iff normals is given, 0 <= nindex[i] < K, and n = normals[nindex[i]] has three finite components that are not all 0.
 * tgt and normals are read for kept pairs only.  Per kept pair, a, b = 0, 1, 2:
 *     p_a = (double)src[i][a] - origin[a],   q_a = (double)tgt[j][a] - origin[a],   d_a = p_a - q_a
 *     [1]  += (d0 d0 + d1 d1) + d2 d2           [2 + a] += p_a            [5 + a] += q_a            [8 + 3a + b] += p_a q_b
 *     [17] += (p0 p0 + p1 p1) + p2 p2           [18]    += (q0 q0 + q1 q1) + q2 q2
 * and, where the pair has a normal, with c = p x n = (p1 n2 - p2 n1, p2 n0 - p0 n2, p0 n1 - p1 n0), J = (c0, c1, c2, n0, n1, n2) and
 * r = (d0 n0 + d1 n1) + d2 n2:
 *     [19 ..39] += J_a J_b for a <= b, row-major (00 01 .. 05 11 12 .. 55)         [40 + a] += J_a r         [46] += r r
 * [0] = the kept pairs, [47] = the kept pairs that have a normal: integer counts, exact as doubles.  A pair that is not kept adds +0
 * to every sum, one without a normal adds +0 to 19..46.
 * Summation as in lara_meshmetrics_reduce (meshmetrics/lara_meshmetrics.h): workgroup w takes pairs 256 w .. 256 w + 255, one per
 * lane; each of the 46 sums goes through the 64-lane xor butterfly (32, 16, .., 1), then ((w0 + w1) + w2) + w3 over the four waves:
 * one partial per workgroup.  A finishing workgroup adds the partials in a fixed order (thread t of 256: partials t, t + 256, ...;
 * then a tree 128, 64, .., 1); the two counts are added as integers.  No floating-point atomics: two calls give the same bits, on
 * any stream.  Lanes beyond N and pairs not kept add +0, so appending pairs that are not kept changes no bit.  N == 0 writes a row of
 * zeros.  Limits: 0 <= N < 2^30, 0 <= M, K < 2^30.
 * Workspace (lara_meshalign_accumulate_workspace_bytes(N)): the partials, 46 doubles and 2 counts per workgroup.
 */
#ifndef LARA_MESHALIGN_H
#define LARA_MESHALIGN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LARA_MESHALIGN_ROW 48

int lara_meshalign_transform(int32_t N, const float *points, const float *normals, const double *A, double inv_scale,
                             float *out_points, float *out_normals, void *stream);

int64_t lara_meshalign_accumulate_workspace_bytes(int32_t N);

int lara_meshalign_accumulate(int32_t N, int32_t M, int32_t K, const float *src, const float *tgt, const int32_t *index,
                              const float *normals, const int32_t *nindex, const float *dist, float max_dist, const double *origin,
                              double *row, void *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif
