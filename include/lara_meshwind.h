/*
 * meshwind/lara_meshwind.h -- generalised (solid-angle) winding numbers of a mesh on the triangle hierarchy of
 * meshbvh/lara_meshbvh.h: w(q) = (1 / 4 pi) sum over the valid triangles of the signed solid angle Omega_t(q).  For an
 * outward-oriented closed mesh w is 1 inside and 0 outside; for a mesh with holes, open boundaries, duplicated or non-manifold
 * parts it degrades smoothly, where the crossing counts of meshsign/lara_meshsign.h have no meaning (part of liblara2dgs.so;
 * opt-in, python side: lara_amd/meshwind.py; kernels: csrc/meshwind.hip; the term: csrc/solidangle.h; the walk:
 * csrc/bvhwalk.h).  `bvh` is the buffer lara_meshbvh_build wrote; nothing is added to it.  All pointers are device pointers unless a
 * parameter says HOST.  Returns 0 or a negative LARA2DGS_E_* code.  Work is enqueued on `stream`; no entry point reads anything
 * back to the host.  Built with -ffp-contract=off: the sequences written here are the instructions.
 *
 * ---- one term (csrc/solidangle.h; lara_meshwind_solid_host runs it on the CPU) --------------------------------------------------------
 * Van Oosterom and Strackee, double on the fp32 inputs:
 *     a = p0 - q, b = p1 - q, c = p2 - q;   x = b x c (each component one product pair and one subtraction)
 *     num = (a_0 x_0 + a_1 x_1) + a_2 x_2
 *     den = (|a| (|b| |c|) + (b . c) |a|) + ((a . b) |c| + (c . a) |b|),   |v| = sqrt((v_0 v_0 + v_1 v_1) + v_2 v_2), u . v likewise
 *     Omega = 2 atan2(num, den);   num == 0 gives exactly 0
 * The rule on num covers a triangle without area, q in the triangle's plane (on it or beside it) and q at a vertex; without it
 * atan2(+-0, negative) = +-pi would count half a turn for a point on a face.  Omega > 0: q sees the face whose normal
 * (p1 - p0) x (p2 - p0) points away from it.  atan2 is the only operation that is not correctly rounded.  den is symmetric in p1
 * and p2 as written and num changes its sign exactly under that swap: a triangle with p1 and p2 exchanged gives -Omega bit for bit.
 * lara_meshwind_solid_host: points HOST [n][3] f32, triangles9 HOST [n][9] f32 -> omega HOST [n] f64.  No device is touched.
 * lara_meshwind_brute_host: points HOST [N][3] f32, triangles9 HOST [T][9] f32 (all taken as valid) -> w HOST [N] f64 = (the sum of
 * Omega in triangle order) / 4 pi; NaN for a point with a coordinate that is not finite.  No device is touched.
 *
 * ---- lara_meshwind_moments: per-node data -----------------------------------------------------------------------------------------------
 * A caller-owned buffer of lara_meshwind_moments_bytes(T) bytes beside the hierarchy's; its layout is a function of T alone:
 *     bytes 0 .. 255      int64 off[LARA_MESHBVH_MAX_LEVELS]: the byte offset of level k's slots (0 beyond the levels), then int64 T
 *     level k             64 bytes for each of its STORED slots (n_k rounded up to a multiple of 8, the box slots of mb_layout),
 *                         level 0 first; off[0] = 256, off[k + 1] = off[k] + 64 stored_k
 * T is the number of triangles the hierarchy was built for; the entry takes it because the launches are sized on the host.  (A
 * buffer whose header names another T is left untouched.)  A slot holds 8 doubles {N_x, N_y, N_z, A, c_x, c_y, c_z, r2}:
 *     N  = sum 1/2 n_t,  n_t = (p1 - p0) x (p2 - p0)                     the dipole (the area vector)
 *     A  = sum A_t,  A_t = 1/2 sqrt((n_x n_x + n_y n_y) + n_z n_z)       the area
 *     c  = (sum A_t c_t) / A,  c_t = ((p0 + p1) + p2) / 3                the area-weighted centre
 *     r2 = (m_x + m_y) + m_z,  m_a = max((c_a - lo_a)^2, (hi_a - c_a)^2) the far corner of the slot's stored fp32 box
 * Level 0: one thread per slot sums its up-to-8 valid records in stored order.  Level k: one thread per slot sums its 8 children in
 * slot order: N and A as they are stored, and A_child c_child for the centre.  One launch per level, no atomics: two calls give the
 * same bits.  A slot with A == 0 (empty, a padding slot, or one that holds only triangles without area) is FLAGGED: all 8 doubles
 * are zero, it contributes exactly 0 and is never entered.
 *
 * ---- lara_meshwind_rows: the walk ------------------------------------------------------------------------------------------------------
 * points [N][3] f32, bvh as built, moments as built, beta > 0 (+inf allowed) -> w [N] f64, n_tri [N] i32 or NULL, n_far [N] i32 or
 * NULL.  One thread per point; the stackless walk of csrc/bvhwalk.h with mask 0 (the stored order), from the root.  At a slot
 * that is not flagged, with d = c - q, d2 = (d_x d_x + d_y d_y) + d_z d_z:
 *     if d2 > (beta beta) r2:   sum += ((d_x N_x + d_y N_y) + d_z N_z) / (d2 sqrt(d2)), n_far += 1, step over the slot
 *     else at level 0:          sum += Omega of each valid record in stored order, n_tri += 1 for each
 *     else:                     descend
 * w = sum / 4 pi (4 pi = 12.566370614359172).  beta = +inf never approximates: the exact sum in tree order.  The order of the sum
 * is the walk's order: two calls give the same bits.  A point with a coordinate that is not finite gives w = NaN and zero counters; a
 * mesh without a valid triangle gives w = 0.  No LDS, no atomics, no stack.  Moments built for another T give NaN, not a walk.
 *
 * ---- lara_meshwind_classify ------------------------------------------------------------------------------------------------------------
 * w [N] f64, threshold, band >= 0, dist [N] f32 or NULL -> inside [N] u8, status [N] u8, sdf [N] f32 or NULL (NULL when dist is).
 *     inside = w > threshold
 *     status bit 0: |w - threshold| < band (undecided);   bit 2: w is not finite (counts as outside);   bit 1 is never set
 *     sdf = -dist when inside, else dist: the magnitude's bits are lara_meshbvh_query's; NaN stays NaN
 * The bits are those lara_meshsign_counts reads, so it is called unchanged on two sides' inside / status.
 *
 * N == 0 is a no-op for rows and classify.  Limits: N < 2^30, T as lara_meshbvh_bytes takes it.
 */
#ifndef LARA_MESHWIND_H
#define LARA_MESHWIND_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LARA_MESHWIND_SLOT_BYTES 64
#define LARA_MESHWIND_HEADER_BYTES 256

int64_t lara_meshwind_moments_bytes(int32_t T);

int lara_meshwind_moments(int32_t T, const void *bvh, void *moments, void *stream);

int lara_meshwind_rows(int32_t N, const float *points, const void *bvh, const void *moments, double beta, double *w, int32_t *n_tri,
                       int32_t *n_far, void *stream);

int lara_meshwind_classify(int32_t N, const double *w, double threshold, double band, const float *dist, uint8_t *inside,
                           uint8_t *status, float *sdf, void *stream);

int lara_meshwind_solid_host(int64_t n, const float *points, const float *triangles9, double *omega);

int lara_meshwind_brute_host(int32_t N, const float *points, int64_t T, const float *triangles9, double *w);

#ifdef __cplusplus
}
#endif
#endif
