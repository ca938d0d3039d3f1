/*
 * meshdist/lara_meshdist.h -- exact distances from points to a triangle mesh on the device: a uniform grid over the triangles, the
 * ring search of lara_meshmetrics_nearest carried over from points to triangles, a brute-force kernel for what the rings do not
 * settle (part of liblara2dgs.so; opt-in, python side: lara_amd/meshdist.py; kernels: csrc/meshdist.hip; the distance function,
 * shared by host and device: csrc/tridist.h).  All pointers are device pointers unless a parameter says HOST.  Returns 0 or a
 * negative LARA2DGS_E_* code.  Work is enqueued on `stream`; no entry point reads anything back to the host.  Built with
 * -ffp-contract=off: the sequences written here are the instructions.
 *
 * ---- the distance: d2(q, p0 p1 p2) and the closest point c ------------------------------------------------------------------------
 * fp32 inputs, every operation in double.  Dot products and squared lengths are (x x' + y y') + z z'; a cross product a x b is
 * (ay bz - az by, az bx - ax bz, ax by - ay bx).
 *     e0 = p1 - p0,  e2 = p2 - p0,  n = e0 x e2,  nn = n . n
 *     if nn > 0:  f0 = (e0 x (q - p0)) . n,  f1 = ((p2 - p1) x (q - p1)) . n,  f2 = ((p0 - p2) x (q - p2)) . n
 *         if f0 >= 0 and f1 >= 0 and f2 >= 0:  s = n . (q - p0),  d2 = (s s) / nn,  c = q - (s / nn) n
 *     otherwise, over the sides (a, b) = (p0, p1), (p1, p2), (p2, p0) in this order:
 *         ab = b - a,  den = ab . ab,  t = clamp(((q - a) . ab) / den, 0, 1)  (t = 0 where den = 0),  c' = a + t ab,  d2' = |q - c'|^2
 *         d2 = the smallest d2', c its c'; a later side replaces an earlier one only when strictly smaller.
 * A triangle without area is therefore its sides, or its point.  With finite fp32 inputs every intermediate stays finite.
 * lara_meshdist_point_triangle_host runs exactly this function on the CPU over n (query, triangle) pairs: queries HOST [n][3] f32,
 * triangles9 HOST [n][9] f32 (p0, p1, p2) -> d2 HOST [n] double, closest HOST [n][3] double (may be NULL).  No device is touched.
 *
 * ---- lara_meshdist_build: the grid of a mesh, built once for any number of query sets -----------------------------------------------
 * vertices [Nv][3] f32, triangles [T][3] i32 -> grid: lara_meshdist_grid_bytes(T) bytes, a function of T alone.
 * A triangle with an index outside [0, Nv) or a coordinate that is not finite is never a candidate; such triangles are counted.
 * Records: every triangle is packed once into 48 bytes {p0, p1, p2, id, -, -} so that a candidate costs three 16-byte loads.
 * Grid: lo, hi = the bounding box of the valid triangles' vertices.  R = clamp(ceil(sqrt(T / 4)), 1, 256), cubic cells, h, inv_h,
 * R_a and the cell rule
 *     cell_a(p) = clamp(floor((p_a - lo_a) inv_h), 0, R_a - 1)   in fp32; a NaN goes to cell 0
 * exactly as lara_meshmetrics_nearest states them (meshmetrics/lara_meshmetrics.h).  The rule is monotone in p_a, so a triangle
 * registered in every cell of the block [cell(min corner), cell(max corner)] of its bounding box is registered in the cell of each
 * of its points: the block covers it.  A triangle whose block spans more than LARA_MESHDIST_MAX_SPAN cells on some axis goes to the
 * LARGE LIST instead, in increasing triangle id (a scan of flags, not an atomic cursor); every other triangle contributes at most
 * MAX_SPAN^3 = 64 (triangle, cell) pairs, which is what makes the grid's size a function of T.  Sequence: pack + box, the grid
 * record, an integer atomicAdd histogram over the cells, two inclusive scans, a cursor scatter of the ids.  The order inside a cell
 * is not reproducible; the result is, by the tie rule.
 * The grid's first LARA_MESHDIST_HEADER_INTS int32 may be read by the caller: [LARA_MESHDIST_HDR_BAD] triangles refused as above,
 * [_HDR_LARGE] the large list's length, [_HDR_PAIRS] (triangle, cell) pairs (uint32), [_HDR_TRIANGLES] T.
 * Size: 316 bytes per triangle (the record, 64 pair slots, the flags, their scan, the large list) and 8 bytes per cell: at the
 * bench mesh of tools/meshdist_bench.py (556 516 triangles, R = 256) 176 MB + 134 MB = 310 MB.
 * Limits: 0 < T < 2^26 (64 T pairs are counted in 32 bits), 0 < Nv < 2^30.
 *
 * ---- lara_meshdist_query: for every query the nearest triangle, exactly -------------------------------------------------------------
 * queries [N][3] f32, grid as built -> dist [N] f32 = (float)sqrt(d2), face [N] i32, closest [N][3] f32 (may be NULL): c rounded.
 *     face = argmin d2 over the valid triangles; an exact tie of d2 goes to the SMALLER triangle id, so the result does not depend
 *     on the scatter's order and two calls give the same bits.  With no valid triangle face = -1, dist = +inf, closest = NaN.
 *     A query with a coordinate that is not finite gets the same: face = -1, dist = +inf, closest = NaN, at once.
 * One thread per query: the large list first, then Chebyshev rings r = 0 .. LARA_MESHDIST_RMAX around the query's (clamped) cell
 * with the gap, margin and bound of lara_meshmetrics_nearest:
 *     gap = min over axes of { u_a - (c_a - r) h  if c_a - r > 0 ;  (c_a + r + 1) h - u_a  if c_a + r + 1 < R_a }   (+inf if none)
 *     margin = 2^-18 max(|u_x|, |u_y|, |u_z|, R h),   bound = max(0, gap - margin),   accept when d2 < (double)bound^2
 * A triangle not met so far is registered in no cell of the searched block, so its own block lies beyond one of the searched
 * block's unclipped faces on some axis, and with it its bounding box and all of its points: farther than gap.  The margin covers the
 * roundings of the cell rule and of gap as it does there.  A triangle met in several cells is tested several times, which the tie
 * rule makes harmless.  A query not accepted after ring RMAX is appended to a list (integer atomic cursor) and a second kernel
 * resolves it by brute force: a workgroup per query, all T records tiled through LDS, same function, same tie rule.
 * No loop runs longer than RMAX rings, the large list or T triangles.  No floating-point atomics.  fallback_count (may be NULL): one
 * int32, the number of queries that took the brute-force route.  N == 0 is a no-op.  Limit: N < 2^30.
 * Workspace (lara_meshdist_query_workspace_bytes(N)): the list and its length.
 *
 * ---- lara_meshdist_face_normals ------------------------------------------------------------------------------------------------------
 * normals [T][3] f32 = c / |c| for c = (p1 - p0) x (p2 - p0), in double from the fp32 vertices, as the sampler computes them; a
 * zero vector where |c| is 0 or not finite, or an index lies outside [0, Nv).
 */
#ifndef LARA_MESHDIST_H
#define LARA_MESHDIST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LARA_MESHDIST_RMAX 4
#define LARA_MESHDIST_MAX_SPAN 4
#define LARA_MESHDIST_MAX_GRID 256
#define LARA_MESHDIST_HEADER_INTS 4
#define LARA_MESHDIST_HDR_BAD 0
#define LARA_MESHDIST_HDR_LARGE 1
#define LARA_MESHDIST_HDR_PAIRS 2
#define LARA_MESHDIST_HDR_TRIANGLES 3

int32_t lara_meshdist_grid_resolution(int32_t T);

int64_t lara_meshdist_grid_bytes(int32_t T);

int lara_meshdist_build(int32_t Nv, int32_t T, const float *vertices, const int32_t *triangles, void *grid, void *stream);

int64_t lara_meshdist_query_workspace_bytes(int32_t N);

int lara_meshdist_query(int32_t N, const float *queries, const void *grid, float *dist, int32_t *face, float *closest,
                        int32_t *fallback_count, void *workspace, void *stream);

int lara_meshdist_face_normals(int32_t Nv, int32_t T, const float *vertices, const int32_t *triangles, float *normals, void *stream);

int lara_meshdist_point_triangle_host(int64_t n, const float *queries, const float *triangles9, double *d2, double *closest);

#ifdef __cplusplus
}
#endif
#endif
