/*
 * meshmetrics/lara_meshmetrics.h -- geometry scores between two surfaces on the device: an area-weighted surface sampler, an
 * exact nearest-neighbour search over a uniform grid, and the reduction behind accuracy / completeness / Chamfer / F-score /
 * normal consistency (part of liblara2dgs.so; opt-in, python side: lara_amd/meshmetrics.py; kernels: csrc/meshmetrics.hip).
 * All pointers are device pointers unless a parameter says HOST.  Returns 0 or a negative LARA2DGS_E_* code.  Work is enqueued
 * on `stream`; lara_meshmetrics_sample_surface alone waits for the stream once (below).  Built with -ffp-contract=off: the
 * sequences written here are the instructions.
 *
 * ---- lara_meshmetrics_sample_surface: n points on a triangle mesh, area-weighted, stratified, deterministic ----------------------
 * vertices [Nv][3] f32, triangles [T][3] i32.
 *   1. area_i = 0.5 |(p1 - p0) x (p2 - p0)| in double from the fp32 vertices; a triangle with an index outside [0, Nv) has
 *      area 0 and is counted.  The areas are added in a fixed order (thread t of 1024: items t, t + 1024, ...; then a tree).
 *   2. THE ONE HOST READ: 16 bytes {total area, bad-index count}; the call waits for `stream` here.  A bad index, or a total
 *      that is not a positive finite number, returns LARA2DGS_E_INVALID.  With total = m 2^e, 0.5 <= m < 1 (frexp), the scale
 *      exponent is s = 39 - e (so that sum q < 2^40 with a factor of two to spare), written to the HOST int32 *scale_exp.
 *   3. q_i = floor(area_i 2^s) as int64 (0 where the area is not a positive finite number) -> q [T], an output.
 *   4. inclusive prefix sum of q over int64 (exact, independent of association): a three-launch device scan.  S = prefix[T-1].
 *   5. sample k in [0, n): t_k = ((2k + 1) S) / (2n) in unsigned 64-bit integers (floor); the face is the smallest i with
 *      prefix[i] > t_k (binary search), so a face with q_i = 0 is never chosen (S >= 2^38 - T > 0 by the choice of s).
 *      mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16        (uint32, wrapping)
 *      s0 = mix(seed + 0x9e3779b9),  h1 = mix(s0 ^ (2k)),  h2 = mix(s0 ^ (2k + 1)),  r1 = (h1 >> 8) 2^-24,  r2 = (h2 >> 8) 2^-24
 *      su = sqrt(r1),  b = (1 - su, su (1 - r2), su r2), point = (b0 p0 + b1 p1) + b2 p2, normal = c / |c| for
 *      c = (p1 - p0) x (p2 - p0): all in double, stored as fp32.
 *      points [n][3] f32, normals [n][3] f32 (may be NULL), face [n] i32.
 * Limits: 0 < T < 2^28, 0 < Nv < 2^30, 0 <= n <= LARA_MESHMETRICS_MAX_SAMPLES (2^22: (2k + 1) S stays below 2^63).
 * Workspace (lara_meshmetrics_sample_workspace_bytes(T)): areas, the prefix, the scan's block sums, the 16-byte record.
 *
 * ---- lara_meshmetrics_nearest: for every query the nearest target, exactly --------------------------------------------------------
 * queries [N][3] f32, targets [M][3] f32 -> dist [N] f32, index [N] i32.
 *     d2(q, t) = ((qx - tx)^2 + (qy - ty)^2) + (qz - tz)^2 in fp32;  index = argmin d2, an exact tie goes to the SMALLER index;
 *     dist = sqrt(d2).  A target with a NaN coordinate is never chosen; with no candidate at all index = -1, dist = +inf.
 * Grid.  lo, hi = the targets' bounding box (a min/max reduction).  R = clamp(ceil(sqrt(M / 4)), 1, 256): a surface crosses about
 * R^2 of a grid's cells, so this aims at a few targets per occupied cell.  Cubic cells: h = max_a(hi_a - lo_a) / R, inv_h = 1 / h
 * (h = inv_h = 1 where that extent is 0 or not finite), R_a = clamp(int((hi_a - lo_a) inv_h) + 1, 1, R) cells along axis a.
 *     cell_a(p) = clamp(floor((p_a - lo_a) inv_h), 0, R_a - 1)   in fp32; a NaN goes to cell 0
 * Build: an integer atomicAdd histogram over the R^3 cell words, an inclusive scan, a cursor scatter of {x, y, z, index}
 * records.  The order inside a cell is not reproducible; the result is, by the tie rule.
 * Query, one thread each: Chebyshev rings r = 0 .. LARA_MESHMETRICS_RMAX around the query's (clamped) cell c.  After ring r the
 * searched block is [c_a - r, c_a + r] on every axis, clipped to the grid.  Every target outside it lies beyond one of the block's
 * faces that the grid boundary did not clip: with u_a = q_a - lo_a,
 *     gap = min over axes of { u_a - (c_a - r) h  if c_a - r > 0 ;  (c_a + r + 1) h - u_a  if c_a + r + 1 < R_a }   (+inf if none)
 *     margin = 2^-18 max(|u_x|, |u_y|, |u_z|, R h),   bound = max(0, gap - margin)
 * and the best candidate so far is accepted when d2 < bound^2.  The margin is conservative: a target's cell comes from two fp32
 * roundings (it may sit an ulp across a face: 2^-22 R h), gap from three more, d2 from a few ulps; together below 2^-21 of the
 * magnitudes involved.  A query not accepted after ring RMAX is appended to a list (integer atomic cursor) and a second kernel
 * resolves it by brute force over all M targets: a workgroup per query, the targets tiled through LDS, same d2, same tie rule.
 * No loop runs longer than RMAX rings or M targets.  fallback_count (may be NULL): one int32, the number of queries that took the
 * brute-force route.  M <= 0 returns LARA2DGS_E_INVALID; N == 0 is a no-op.  Limits: N, M < 2^30.
 * Workspace (lara_meshmetrics_nearest_workspace_bytes(N, M)): grid record, bounds partials, cell words, scan, records, list.
 *
 * ---- lara_meshmetrics_reduce: the sums of one direction ---------------------------------------------------------------------------
 * dist [N] f32, index [N] i32 as lara_meshmetrics_nearest wrote them for M targets; normals_q [N][3], normals_t [M][3] f32 or both NULL;
 * thresholds: HOST float [n_thr], n_thr <= LARA_MESHMETRICS_MAX_THRESHOLDS.  row [LARA_MESHMETRICS_ROW] doubles:
 *     row[0] = N, row[1] = sum d, row[2] = sum d^2 (d as double), row[3] = sum |nq . nt[index]| (in double; 0 without normals;
 *     a query whose index lies outside [0, M) adds 0), row[4 + k] = #{d <= thresholds[k]} (fp32 comparison; integer counts, exact as doubles).
 * Per-workgroup partials (256 queries each: a wave butterfly, then the four waves in order), added in a fixed order by a
 * finishing workgroup (thread t of 256: partials t, t + 256, ...; then a tree); counts are added as integers.  No floating-point
 * atomics: a call is bit-reproducible.  N == 0 writes a row of zeros.
 * Workspace (lara_meshmetrics_reduce_workspace_bytes(N)): the partials.
 */
#ifndef LARA_MESHMETRICS_H
#define LARA_MESHMETRICS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LARA_MESHMETRICS_MAX_SAMPLES (1 << 22)
#define LARA_MESHMETRICS_RMAX 4
#define LARA_MESHMETRICS_MAX_GRID 256
#define LARA_MESHMETRICS_MAX_THRESHOLDS 8
#define LARA_MESHMETRICS_ROW 12

int64_t lara_meshmetrics_sample_workspace_bytes(int32_t T);

int lara_meshmetrics_sample_surface(int32_t Nv, int32_t T, const float *vertices, const int32_t *triangles, int32_t n,
                                    int32_t seed, int64_t *q, int32_t *scale_exp, float *points, float *normals, int32_t *face,
                                    void *workspace, void *stream);

int32_t lara_meshmetrics_grid_resolution(int32_t M);

int64_t lara_meshmetrics_nearest_workspace_bytes(int32_t N, int32_t M);

int lara_meshmetrics_nearest(int32_t N, int32_t M, const float *queries, const float *targets, float *dist, int32_t *index,
                             int32_t *fallback_count, void *workspace, void *stream);

int64_t lara_meshmetrics_reduce_workspace_bytes(int32_t N);

int lara_meshmetrics_reduce(int32_t N, int32_t M, const float *dist, const int32_t *index, const float *normals_q, const float *normals_t,
                            int32_t n_thr, const float *thresholds, double *row, void *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif
