/*
 * meshsign/lara_meshsign.h -- is a point inside a mesh: crossings of fixed rays counted on the triangle hierarchy of
 * meshbvh/lara_meshbvh.h, the vote over them, signed distances, lattice counts for a volume IoU and the mesh's own signed volume
 * (part of liblara2dgs.so; opt-in, python side: lara_amd/meshsign.py; kernels: csrc/meshsign.hip; the crossing: csrc/raycross.h on
 * csrc/raytri.h; the box test: csrc/raybox.h; the walk: csrc/bvhwalk.h).  `bvh` is the buffer lara_meshbvh_build wrote; nothing
 * is added to it.  All pointers are device pointers unless a parameter says HOST.  Returns 0 or a negative LARA2DGS_E_* code.  Work
 * is enqueued on `stream`; no entry point reads anything back to the host.  Built with -ffp-contract=off: the sequences written
 * here and in meshray/lara_meshray.h are the instructions.
 *
 * ---- one crossing (csrc/raycross.h; lara_meshsign_cross_host runs it on the CPU) ------------------------------------------------------
 * lara_raycross(ray, p0, p1, p2) accepts exactly when lara_raytri of meshray/lara_meshray.h accepts with the window [0, +inf): U, V, W
 * of one sign (zeros inclusive), det = (U + V) + W != 0, t >= 0, the sanity clause.  On acceptance, from the same U, V, W:
 *     orient = +1 when det < 0: the ray leaves through a face whose normal (p1 - p0) x (p2 - p0) points along it; else -1
 *     touch  = 1 when one of U, V, W is exactly zero: the ray meets an edge or a vertex of the triangle AS COMPUTED
 * The sheared vertices depend on the ray and the vertex alone, so all triangles around an edge or a vertex see the same zero:
 * lara_meshray_cast counts such a ray once per touching triangle, right for a first hit and wrong for parity.  Here a touching ray
 * is not counted at all: it is unusable, and the vote goes on without it.
 * lara_meshsign_cross_host: origins, directions HOST [n][3] f32, triangles9 HOST [n][9] f32 -> hit HOST [n] u8, orient HOST [n] i8
 * (0 on a miss), touch HOST [n] u8 (0 on a miss).  No device is touched.
 *
 * ---- the rays ---------------------------------------------------------------------------------------------------------------------------
 * Ray k of a point p is o = p, d = LARA_MESHSIGN_DIRECTIONS[k], the window [0, +inf).  The dominant component of every direction
 * is exactly +-1, so Sx, Sy, Sz of the shear are the other components themselves, exactly; those are dyadics of four bits:
 *     D0 = (1, 3/8, 11/16)      D1 = (-7/16, 1, 5/16)      D2 = (9/16, -5/16, -1)
 *
 * ---- lara_meshsign_rows: the counting walk ---------------------------------------------------------------------------------------------
 * points [N][3] f32, K in 1 .. LARA_MESHSIGN_MAX_RAYS, bvh as built -> cross [N][K] i32, wind [N][K] i32.  Over all valid triangles
 * (record id >= 0):   cross = the number of accepted crossings,   wind = the sum of orient.
 * If an accepted crossing has touch, the ray is unusable: cross = -1, wind = 0; so is every ray of a point with a coordinate that is
 * not finite.  For an outward-oriented closed mesh wind is +1 inside and 0 outside, cross odd inside and even outside.
 * One thread per (point, ray), blockIdx.y = k, so that a wave holds neighbouring points under one direction; no LDS, no atomics, no
 * stack.  The walk is the one of lara_meshbvh_query and lara_meshray_cast (csrc/bvhwalk.h) from the root, in the stored sibling order,
 * without a best-so-far, a skip id or an early end: a slot is entered exactly when it is non-empty and lara_raybox(ray, lo, hi, 0,
 * +inf) is finite.  By the bound's contract (meshray/lara_meshray.h) every triangle lara_raytri accepts lies in entered boxes only,
 * and a leaf's records are all tested, so the counts equal brute force over all triangles as integers.
 * lara_meshsign_rows_host: points HOST [N][3] f32, triangles9 HOST [T][9] f32 (all taken as valid) -> cross, wind HOST [N][K] i32:
 * brute force over all T triangles with the same function.
 *
 * ---- lara_meshsign_vote ----------------------------------------------------------------------------------------------------------------
 * cross, wind [N][K] i32, rule, dist [N] f32 or NULL -> inside [N] u8, status [N] u8, sdf [N] f32 or NULL (NULL when dist is).
 *     a ray is usable when cross >= 0
 *     rule LARA_MESHSIGN_RULE_PARITY (0): a usable ray votes inside when cross is odd
 *     rule LARA_MESHSIGN_RULE_WINDING (1): a usable ray votes inside when wind != 0 (the union of overlapping closed parts)
 *     inside = (2 x inside votes > usable rays): a tie counts as outside, and so does a point without a usable ray
 *     status bit 0: the usable rays disagree;  bit 1: some ray was unusable;  bit 2: no ray was usable
 *     sdf = -dist when inside, else dist: the magnitude's bits are lara_meshbvh_query's; NaN stays NaN
 *
 * ---- lara_meshsign_counts ----------------------------------------------------------------------------------------------------------------
 * inside_a, status_a, inside_b, status_b [N] u8 -> out [8] i64, which the call sets itself (a memset on `stream`, then the kernel):
 *     out[0] = n_a, out[1] = n_b, out[2] = n_and, out[3] = n_or (points inside a, b, both, either),
 *     out[4], out[5] = points with status bit 0 on side a, b;   out[6], out[7] = points with status bit 2 on side a, b.
 * Integer sums: a wave's butterfly, the four waves of a workgroup through 128 bytes of LDS, one 64-bit integer atomic per workgroup
 * and count.  Exact, whatever the order.  N may be 0 (all zero).
 *
 * ---- lara_meshsign_volume ----------------------------------------------------------------------------------------------------------------
 * bvh as built -> out [3] f64: the signed volume sum (p0 - c) . ((p1 - c) x (p2 - c)) / 6, the area sum |(p1 - p0) x (p2 - p0)| / 2 and
 * the number of valid records, over the valid records in their stored order.  c = the centre 0.5 lo + 0.5 hi of the root's
 * box, which keeps the terms small for a mesh far from the origin.  All arithmetic is double:
 *     a = p0 - c, b = p1 - c, e = p2 - c;   term = (a_x (b_y e_z - b_z e_y) + a_y (b_z e_x - b_x e_z)) + a_z (b_x e_y - b_y e_x)
 *     u = p1 - p0, v = p2 - p0, n = u x v (each component one product pair and one subtraction);   area term = sqrt((n_x n_x + n_y n_y) + n_z n_z)
 * One workgroup of 256: thread j adds the records j, j + 256, ... in that order, then csrc/rowsum.h's order (the xor butterfly inside
 * a wave, the four waves as ((w0 + w1) + w2) + w3); the two sums are then divided by 6 and by 2.  No floating-point atomics and no
 * workspace: two calls give the same bits.  A positive volume: the faces of a closed mesh are oriented outwards.
 *
 * N == 0 is a no-op for rows and vote.  Limits: N K < 2^30 (rows), N < 2^30 (vote, counts).
 */
#ifndef LARA_MESHSIGN_H
#define LARA_MESHSIGN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LARA_MESHSIGN_MAX_RAYS 3
#define LARA_MESHSIGN_RULE_PARITY 0
#define LARA_MESHSIGN_RULE_WINDING 1
#define LARA_MESHSIGN_DIRECTIONS {{1.0f, 0.375f, 0.6875f}, {-0.4375f, 1.0f, 0.3125f}, {0.5625f, -0.3125f, -1.0f}}

int lara_meshsign_rows(int32_t N, const float *points, int32_t K, const void *bvh, int32_t *cross, int32_t *wind, void *stream);

int lara_meshsign_vote(int32_t N, int32_t K, const int32_t *cross, const int32_t *wind, int32_t rule, const float *dist,
                       uint8_t *inside, uint8_t *status, float *sdf, void *stream);

int lara_meshsign_counts(int32_t N, const uint8_t *inside_a, const uint8_t *status_a, const uint8_t *inside_b, const uint8_t *status_b,
                         int64_t *out, void *stream);

int lara_meshsign_volume(const void *bvh, double *out, void *stream);

int lara_meshsign_cross_host(int64_t n, const float *origins, const float *directions, const float *triangles9, uint8_t *hit,
                             int8_t *orient, uint8_t *touch);

int lara_meshsign_rows_host(int32_t N, const float *points, int32_t K, int64_t T, const float *triangles9, int32_t *cross,
                            int32_t *wind);

#ifdef __cplusplus
}
#endif
#endif
