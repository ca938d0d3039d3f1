/*
 * meshbvh/lara_meshbvh.h -- exact distances from points to a triangle mesh at ANY distance: a bounding-volume hierarchy over the
 * triangles, the second search structure next to the uniform grid of meshdist/lara_meshdist.h (part of liblara2dgs.so; opt-in,
 * python side: lara_amd/meshbvh.py; kernels: csrc/meshbvh.hip; the distance function: csrc/tridist.h, the one meshdist runs; the
 * bound from a point to a box: csrc/boxbound.h, shared by host and device).  All pointers are device pointers unless a parameter
 * says HOST.  Returns 0 or a negative LARA2DGS_E_* code.  Work is enqueued on `stream`; no entry point reads anything back to the
 * host.  Built with -ffp-contract=off: the sequences written here are the instructions.
 *
 * ---- the structure: sorted records and an implicit complete 8-ary tree of boxes ------------------------------------------------------
 * vertices [Nv][3] f32, triangles [T][3] i32 -> bvh: lara_meshbvh_bytes(T) bytes, a function of T alone.  Two calls with a sort of
 * T 64-bit keys between them, which the caller does (python: torch.sort): lara_meshbvh_keys, sort keys[0 .. T) ascending in place
 * (byte offset: lara_meshbvh_layout), lara_meshbvh_build.  The keys are unique, so any sort gives the same order.
 *
 * lara_meshbvh_keys.  A triangle with an index outside [0, Nv) or a coordinate that is not finite is never a candidate, exactly as
 * lara_meshdist_build states it; such triangles are counted.  lo, hi = the fp32 bounding box of the valid triangles' vertices.  Per
 * axis a, in fp32:
 *     ext_a = hi_a - lo_a,   inv_a = 1024 / ext_a  where ext_a > 0 and the quotient is finite, else 0      (no valid triangle: lo = 0, inv = 0)
 * A valid triangle's box mn, mx (fp32 min / max of its three vertices) has the centre and the cell
 *     c_a = 0.5 mn_a + 0.5 mx_a,   cell_a(c) = clamp(floor((c_a - lo_a) inv_a), 0, 1023)   in fp32; a NaN goes to cell 0
 * and the 30-bit Morton code m = sum over bits b = 0 .. 9 of (cell_x >> b & 1) << 3b | (cell_y >> b & 1) << 3b + 1 | (cell_z >> b & 1)
 * << 3b + 2.  The same rule gives a query's code (the seed, below).  Key: a valid triangle i gets m << 26 | i, an invalid one
 * 1 << 62 | i; T < 2^26 keeps them unique, and the invalid ones sort to the end.  The valid triangles are counted with an integer atomic.
 *
 * lara_meshbvh_build (keys sorted).  Records: the triangle of sorted position j packed into 48 bytes {p0, p1, p2, id, -, -} as
 * meshdist packs them (an invalid one: zero coordinates, id = -1).  Boxes, 24 bytes {lo x y z, hi x y z} each, fp32 min / max and
 * therefore exact:
 *     level 0, slot j:      the box of the valid records 8 j .. 8 j + 7;          n_0 = ceil(T / 8) slots
 *     level k + 1, slot j:  the box of the level-k slots 8 j .. 8 j + 7 below n_k;  n_(k+1) = ceil(n_k / 8), until n_k = 1 (the root)
 * A slot without a valid record below it is EMPTY: lo = +inf, hi = -inf.  Every level is stored with its slot count rounded up to a
 * multiple of 8 (the padding slots are empty), so the eight children of any slot exist.  One launch per level -- at most
 * LARA_MESHBVH_MAX_LEVELS = 9 for T < 2^26, known from T alone --: the kernel boundary is the hand-off between levels, no box is
 * published to another workgroup inside a launch.
 * The first LARA_MESHBVH_HEADER_INTS int32 of bvh may be read by the caller: [LARA_MESHBVH_HDR_BAD] triangles refused as above,
 * [_HDR_VALID] the valid ones, [_HDR_TRIANGLES] T, [_HDR_LEVELS] the number of levels.
 * Size, exactly (P(n) = 8 ceil(n / 8), A(x) = x rounded up to a multiple of 256):
 *     lara_meshbvh_bytes(T) = 256 + A(8 T) + A(48 T) + A(24 * 1024) + sum over the levels k of A(24 P(n_k))
 * that is 8 (keys) + 48 (records) + 24 / 8 * (1 + 1/8 + ...) = 3.43 (boxes) = 59.4 bytes a triangle, 51.4 without the keys, plus at
 * most 24 KB + 256 bytes a level: 33 MB at the bench mesh of tools/meshdist_bench.py (556 516 triangles), where the grid takes 310 MB.
 * lara_meshbvh_layout(T, out HOST [4 + 2 * 9] int64): out[0] = the keys' byte offset, [1] = the records', [2] = the number of levels,
 * [3] = the total; [4 + 2 k], [5 + 2 k] = the byte offset and n_k of level k.
 * Limits: 0 < T < 2^26, 0 < Nv < 2^30.
 *
 * ---- the bound from a point to a box, and its margin (csrc/boxbound.h; lara_meshbvh_box_bound_host runs it on the CPU) -------------------
 * fp32 inputs, every operation in double:
 *     an empty box (not lo_x <= hi_x): +inf
 *     g_a = max(lo_a - q_a, q_a - hi_a, 0),   s = (g_x g_x + g_y g_y) + g_z g_z,   M = max over a of |q_a|, |lo_a|, |hi_a|
 *     bound = max(0, s - (2^-12 s + 2^-40 M M))
 * A node is skipped only when bound > (the best d2 so far), strictly: at equality the node is entered, because the tie rule may
 * prefer a smaller id there.  What has to hold is  bound(q, box) <= the COMPUTED d2 of lara_tridist(q, t) for every triangle t with
 * its vertices in the box.  In real numbers s <= D^2, D the distance from q to t.  In computed numbers that fails: with q over
 * the interior of a flat, axis-aligned triangle the unmargined s exceeds the computed (s' s') / nn in about 2 % of random pairs, by up
 * to 4.3e-16 relative (tests/test_meshbvh.py finds them), because that quotient rounds below the exact value.  The margin:
 *   * lara_tridist's interior branch measures the distance to the plane through p0 with the COMPUTED normal n^.  With u = 2^-53 and
 *     the aspect A = |e0| |e2| / |n|, |n^ - n| <= 6 u |e0| |e2|, an angle of at most 6 u A; over the lever |q - p0| <= 2 sqrt(3) M and
 *     with the roundings of s' itself the computed distance is at least D - E with E <= 28 u A M.  The side branch has no
 *     cancellation: its error is a few u D.
 *   * so the computed d2 >= (D - E)^2 >= (sqrt(s) - E)^2 >= s (1 - e) - E^2 / e for every e > 0 (2 E sqrt(s) <= e s + E^2 / e), and
 *     where sqrt(s) < E the right side is negative and the bound is 0.  With e = 2^-12 and E = 2^-26 M this is the bound above; it
 *     holds for A <= 2^22 (28 u A <= 2^-26), slivers four times thinner than the 1 : 10^6 ones of tests/test_meshdist.py.  The
 *     roundings of g, s and the bound itself (under 8 u s) vanish in 2^-12 s.
 *   * the price: a node is entered although it lies up to 2^-13 D + 2^-20 M beyond the best distance -- 2^-20 M only for queries
 *     nearer than that to the surface.  Nothing measurable.
 * lara_meshbvh_box_bound_host: queries HOST [n][3] f32, boxes6 HOST [n][6] f32 (lo, hi) -> out HOST [n] double.  No device is touched.
 *
 * ---- lara_meshbvh_query: for every query the nearest triangle, exactly, with no ring limit and no fallback ----------------------------
 * queries [N][3] f32, bvh as built -> dist [N] f32 = (float)sqrt(d2), face [N] i32, closest [N][3] f32 (may be NULL): c rounded once.
 *     face = argmin d2 (lara_tridist) over the valid triangles; an exact tie of d2 goes to the SMALLER triangle id.  With no valid
 *     triangle, or a query with a coordinate that is not finite: face = -1, dist = +inf, closest = NaN.
 * Both sides being argmins of the same computed numbers under the same tie rule, the result equals lara_meshdist_query's bit for bit.
 * One thread per query.  Seed: a binary search (at most 26 steps) of the query's own Morton code in the sorted keys, and the eight
 * records of the leaf it lands in: a first best.  (A greedy descent into the child of the smallest bound was tried as the seed in
 * the restatement: on the bench mesh it costs 25 x the triangle tests, because the boxes of siblings overlap and many bounds are 0.)
 * Then a fixed-order walk over the implicit tree by index arithmetic, with no stack (lara_bvhwalk of csrc/bvhwalk.h, the one walk
 * of every unit on this buffer; mask 0, the stored order):
 * from the root, a slot whose box is not empty and whose bound is <= best.d2 is entered (its first child, or at level 0 its eight
 * records), any other is stepped over; after the last of eight siblings the walk continues behind their parent.  Every slot is met at
 * most once, so the walk ends after at most sum P(n_k) steps.  The seed's leaf is met again; the tie rule makes that harmless.
 * No floating-point atomics, no atomics at all in the query.  N == 0 is a no-op.  Limit: N < 2^30.
 */
#ifndef LARA_MESHBVH_H
#define LARA_MESHBVH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LARA_MESHBVH_MAX_LEVELS 9
#define LARA_MESHBVH_HEADER_INTS 4
#define LARA_MESHBVH_HDR_BAD 0
#define LARA_MESHBVH_HDR_VALID 1
#define LARA_MESHBVH_HDR_TRIANGLES 2
#define LARA_MESHBVH_HDR_LEVELS 3

int64_t lara_meshbvh_bytes(int32_t T);

int lara_meshbvh_layout(int32_t T, int64_t *out);

int lara_meshbvh_keys(int32_t Nv, int32_t T, const float *vertices, const int32_t *triangles, void *bvh, void *stream);

int lara_meshbvh_build(int32_t Nv, int32_t T, const float *vertices, const int32_t *triangles, void *bvh, void *stream);

int lara_meshbvh_query(int32_t N, const float *queries, const void *bvh, float *dist, int32_t *face, float *closest, void *stream);

int lara_meshbvh_box_bound_host(int64_t n, const float *queries, const float *boxes6, double *out);

#ifdef __cplusplus
}
#endif
#endif
