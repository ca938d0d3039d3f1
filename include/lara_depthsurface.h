/*
 * depthsurface/lara_depthsurface.h -- a ground-truth surface from depth maps, on the device: back-projection of the valid pixels
 * of V depth maps into an ordered world-space point set with normals, thinning to one point per occupied voxel, the test of which
 * views observed a sample, and the reduction of one direction's distances under a keep mask (part of liblara2dgs.so; opt-in,
 * python side: lara_amd/depthsurface.py; kernels: csrc/depthsurface.hip).  All pointers are device pointers unless a parameter
 * says HOST.  Returns 0 or a negative LARA2DGS_E_* code.  Work is enqueued on `stream`; lara_depthsurface_backproject_count and
 * lara_depthsurface_thin wait for the stream once each (below), nothing else does.  Built with -ffp-contract=off: all arithmetic is
 * fp32 in the written order unless a line says double.
 *
 * ---- conventions ------------------------------------------------------------------------------------------------------------------
 * depth [V][H][W] f32: view-space z.  Pixel (y, x) looks through (x + 0.5, y + 0.5).  ixt [V][4] f32 = fx, fy, cx, cy.
 * pose [V][16] f32, row-major 4 x 4: camera to world (c2w) for the back-projection, world to camera (w2c) for the observation test.
 * mask [V][H][W] or NULL; `mask_elem_bytes` is 1 (uint8 / bool) or 4 (float32); an element counts when it is nonzero, as `.bool()`
 * does (a float is compared with 0: -0 does not count, a NaN does).  depth_max: +inf means none.
 *     valid(v, y, x)  <=>  mask nonzero  and  d finite  and  0 < d <= depth_max                 (d = depth[v][y][x])
 *     P(v, y, x):  a = ((float)x + 0.5f - cx) / fx,  b = ((float)y + 0.5f - cy) / fy,  p = (a d, b d, d),
 *                  world_i = ((R_i0 p.x + R_i1 p.y) + R_i2 p.z) + t_i        (R_ij = pose[4 i + j], t_i = pose[4 i + 3])
 * Limits: 1 <= V <= LARA_DEPTHSURFACE_MAX_VIEWS, H, W >= 1, V H W < 2^31.
 *
 * ---- lara_depthsurface_backproject_count / _emit: valid pixels to an ordered point set -------------------------------------------
 * A pixel is SELECTED when it is valid and y % stride == 0 and x % stride == 0 (stride >= 1).  The selected pixels are numbered
 * in the order (v, y, x) ascending, i.e. by g = (v H + y) W + x.  An ordered compaction in three launches: a workgroup counts the
 * selected pixels of its 1024 consecutive g (wave ballots), one workgroup turns the counts into exclusive offsets, and the emitting
 * launch ranks a pixel by offset + the counts of the waves in front of it + the ballot bits below its lane.  No atomic cursor: two
 * calls give the same bits.
 *   _count: launches the first two, then THE ONE HOST READ: 8 bytes, the number N of selected pixels, written to the HOST int64
 *           *n_points; the call waits for `stream` here.  The offsets stay in `workspace`.
 *   _emit:  with the same V, H, W, depth, mask, stride, depth_max and the workspace _count left: points [N][3] f32 = P, pixel [N]
 *           i32 = g, and normals [N][3] f32 by `normal_mode`:
 *     LARA_DEPTHSURFACE_NORMALS_NONE   `normals` is not written (may be NULL).
 *     LARA_DEPTHSURFACE_NORMALS_GIVEN  normal_map [V][H][W][3] f32, world space: n / |n| with |n| = sqrt((nx^2 + ny^2) + nz^2), in
 *                                      double, stored as fp32; a zero or non-finite vector (or length) gives (0, 0, 0).
 *     LARA_DEPTHSURFACE_NORMALS_DEPTH  c = (P(y+1, x) - P(y-1, x)) x (P(y, x+1) - P(y, x-1)), n = c / |c|: the fp32 points P of the
 *                                      full-resolution map (whatever `stride` is) taken to double, differences, cross product
 *                                      (c_0 = a_1 b_2 - a_2 b_1, ...), length and quotient in double, stored as fp32.  It applies
 *                                      where all four neighbours lie inside the image, are valid (without the stride condition) and
 *                                      |d_neighbour - d| <= jump in fp32 (+inf: no limit).  Everywhere else, and where |c| is 0 or
 *                                      not finite: (0, 0, 0).
 * Workspace (lara_depthsurface_backproject_workspace_bytes(V, H, W)): the block counts / offsets and the 8-byte total.
 *
 * ---- lara_depthsurface_thin: one point per occupied voxel ------------------------------------------------------------------------
 * points [N][3] f32, normals [N][3] f32 or NULL, voxel > 0 (finite).  A point with a non-finite coordinate is DROPPED and counted.
 *     lo_a = min over the other points;  cell_a = (int)floor((p_a - lo_a) / voxel)  (fp32; anything from 2^27 up counts as 2^27);
 *     R_a = max cell_a + 1.  The cell words are (cell_z R_y + cell_y) R_x + cell_x.
 * Each occupied cell keeps its point with the SMALLEST input index: an integer atomicMin over cell words initialised to INT32_MAX;
 * lo and max cell come from integer atomicMin / atomicMax too (on order-preserving integer images of the floats), so nothing
 * depends on scheduling.  The survivors are emitted in input order by the compaction above: kept_index [N'] i32, out_points [N'][3]
 * and (with normals) out_normals [N'][3], bit copies of their rows.  The outputs have room for N rows.
 * THE ONE HOST READ: counts, HOST int64 [2] = {N', dropped}; the call waits for `stream`.  `max_cells` (1 .. 2^27) is the room for
 * cell words in the workspace: R_x R_y R_z > max_cells returns LARA2DGS_E_INVALID (found on the device, reported through the same
 * read; no cell word is touched).  N == 0 writes {0, 0}.  Limits: 0 <= N < 2^31.
 * Workspace (lara_depthsurface_thin_workspace_bytes(N, max_cells)): the grid record, block counts / offsets, the cell words.
 *
 * ---- lara_depthsurface_observe: which views saw each sample -----------------------------------------------------------------------
 * points [N][3] f32 (e.g. samples of the extracted mesh), depth / mask / ixt as above, pose = w2c, tau >= 0, background_is_free 0 / 1
 * -> seen [N] i64: bit v is set when view v observed the sample.  One thread per sample; the views' twenty floats are staged in LDS.
 *     p_i = ((W_i0 x + W_i1 y) + W_i2 z) + W_i3 (i = 0, 1, 2),  z_c = p_2;  not observed unless z_c > 0;
 *     u = (p_0 fx) / z_c + cx,  w = (p_1 fy) / z_c + cy;  not observed unless 0 <= u < (float)W and 0 <= w < (float)H;
 *     the pixel is ((int)floor(w), (int)floor(u)), tested with valid() above (depth_max applies);
 *     on a valid pixel: observed iff z_c <= d + tau (on the seen surface or in front of it; further behind it than tau: occluded);
 *     on any other pixel: observed iff background_is_free (an object dataset's masked background is seen free space).
 * A sample with a non-finite coordinate has seen = 0.  No host read.  N == 0 is a no-op.
 *
 * ---- lara_depthsurface_reduce: one direction's sums under a keep mask -------------------------------------------------------------
 * lara_meshmetrics_reduce (meshmetrics/lara_meshmetrics.h) with two differences: keep [N] u8 or NULL -- a query with keep == 0
 * takes no part --, and a normal pair is counted only where the query's index lies inside [0, M) and both normals are non-zero
 * (any component != 0).  row [LARA_DEPTHSURFACE_ROW] doubles:
 *     row[0] = queries kept, row[1] = sum d, row[2] = sum d^2 (d as double), row[3] = sum |nq . nt[index]| over the counted pairs
 *     (products and sums in double), row[4] = counted pairs, row[5 + k] = #{kept, d <= thresholds[k]} (fp32 comparison).
 * The same decomposition: per-workgroup partials of 256 queries (a wave butterfly, then the four waves in order), added in a fixed
 * order by a finishing workgroup (thread t of 256: partials t, t + 256, ...; then a tree); counts are integers.  No floating-point
 * atomics.  With keep all ones and all normals non-zero, rows [1], [2], [3] and [5 + k] are lara_meshmetrics_reduce's [1], [2], [3]
 * and [4 + k], bit for bit.  thresholds: HOST float [n_thr], n_thr <= LARA_DEPTHSURFACE_MAX_THRESHOLDS.  N == 0 writes zeros.
 * Workspace (lara_depthsurface_reduce_workspace_bytes(N)): the partials.
 */
#ifndef LARA_DEPTHSURFACE_H
#define LARA_DEPTHSURFACE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LARA_DEPTHSURFACE_MAX_VIEWS 64
#define LARA_DEPTHSURFACE_MAX_CELLS (1 << 27)
#define LARA_DEPTHSURFACE_MAX_THRESHOLDS 8
#define LARA_DEPTHSURFACE_ROW 13
#define LARA_DEPTHSURFACE_NORMALS_NONE 0
#define LARA_DEPTHSURFACE_NORMALS_GIVEN 1
#define LARA_DEPTHSURFACE_NORMALS_DEPTH 2

int64_t lara_depthsurface_backproject_workspace_bytes(int32_t V, int32_t H, int32_t W);

int lara_depthsurface_backproject_count(int32_t V, int32_t H, int32_t W, const float *depth, const void *mask, int32_t mask_elem_bytes,
                                        int32_t stride, float depth_max, int64_t *n_points, void *workspace, void *stream);

int lara_depthsurface_backproject_emit(int32_t V, int32_t H, int32_t W, const float *depth, const void *mask, int32_t mask_elem_bytes,
                                       int32_t stride, float depth_max, const float *ixt, const float *pose, int32_t normal_mode,
                                       const float *normal_map, float jump, float *points, float *normals, int32_t *pixel,
                                       void *workspace, void *stream);

int64_t lara_depthsurface_thin_workspace_bytes(int32_t N, int32_t max_cells);

int lara_depthsurface_thin(int32_t N, const float *points, const float *normals, float voxel, int32_t max_cells, int32_t *kept_index,
                           float *out_points, float *out_normals, int64_t *counts, void *workspace, void *stream);

int lara_depthsurface_observe(int32_t N, const float *points, int32_t V, int32_t H, int32_t W, const float *depth, const void *mask,
                              int32_t mask_elem_bytes, float depth_max, const float *ixt, const float *pose, float tau,
                              int32_t background_is_free, int64_t *seen, void *stream);

int64_t lara_depthsurface_reduce_workspace_bytes(int32_t N);

int lara_depthsurface_reduce(int32_t N, int32_t M, const float *dist, const int32_t *index, const uint8_t *keep, const float *normals_q,
                             const float *normals_t, int32_t n_thr, const float *thresholds, double *row, void *workspace,
                             void *stream);

#ifdef __cplusplus
}
#endif
#endif
