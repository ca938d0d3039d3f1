/*
 * meshray/lara_meshray.h -- ray queries on the triangle hierarchy of meshbvh/lara_meshbvh.h: which triangle a ray meets first, whether
 * it meets any, and which of up to 64 eyes see a point past the mesh (part of liblara2dgs.so; opt-in, python side:
 * lara_amd/meshray.py; kernels: csrc/meshray.hip; the ray-triangle function: csrc/raytri.h; the entry parameter of a ray into a
 * box: csrc/raybox.h; both shared by host and device).  `bvh` is the buffer lara_meshbvh_build wrote; nothing is added to it.  All
 * pointers are device pointers unless a parameter says HOST.  Returns 0 or a negative LARA2DGS_E_* code.  Work is enqueued on
 * `stream`; no entry point reads anything back to the host.  Built with -ffp-contract=off: the sequences written here are the
 * instructions.
 *
 * ---- the ray-triangle function (csrc/raytri.h; lara_meshray_raytri_host runs it on the CPU) ------------------------------------------
 * A ray is o + t d, o and d fp32, d NOT normalised; a window t_min <= t <= t_max.  fp32 inputs, every operation in double.
 * Per ray, once:
 *     kz = the axis of the largest |d_a|, the first one on a tie;  kx = (kz + 1) % 3,  ky = (kx + 1) % 3, swapped when d[kz] < 0
 *     Sx = d[kx] / d[kz],   Sy = d[ky] / d[kz],   Sz = 1 / d[kz],   inv_a = 1 / d_a (the box test)
 *     a ray with a component of o or d that is not finite, or with d = 0, never hits
 * Per vertex p:   a = p - o,   X = a[kx] - Sx a[kz],   Y = a[ky] - Sy a[kz],   Z = Sz a[kz]
 * With A, B, C the sheared p0, p1, p2:
 *     U = Cx By - Cy Bx,   V = Ax Cy - Ay Cx,   W = Bx Ay - By Ax
 * A hit needs all of:
 *     U, V, W all >= 0 or all <= 0 (both sides count, zeros inclusive);   det = (U + V) + W != 0
 *     t = ((U Az + V Bz) + W Cz) / det  with  t_min <= t <= t_max
 *     the sanity clause: on every axis a,  x_a = o_a + t d_a  lies in [mn_a - m_a, mx_a + m_a],  mn_a / mx_a the smallest / largest
 *     of the three p_a,  m_a = 2^-20 max(|o_a|, |mn_a|, |mx_a|)
 * The barycentric weights of p0, p1, p2 are U / det, V / det, W / det; the hit is at o + t d.
 * Why this form: X and Y of a vertex depend on the ray and the vertex alone, so the triangles around an edge or a vertex classify
 * the ray against the same computed points; an edge function is two products and one subtraction, each rounding monotone, so its
 * computed sign never contradicts the exact sign FOR THOSE POINTS, and two triangles that share an edge see opposite signs of the
 * same number: a ray cannot slip between two triangles of a closed surface.  The scalar triple product d . (b x c) of unsheared
 * vertices has no such property (tests/test_meshray.py: the ray from the origin through the pole of the 8 x 64 UV sphere misses all
 * 64 wedges under it).  The sanity clause removes the hits of rays that lie in a triangle's plane, where det is rounding noise,
 * and it is what the box bound below stands on.
 * lara_meshray_raytri_host: origins, directions HOST [n][3] f32, t_min, t_max HOST [n] f32 (NULL: 0 and +inf), triangles9 HOST
 * [n][9] f32 -> hit HOST [n] u8, t HOST [n] double (+inf on a miss), bary HOST [n][3] double (may be NULL; NaN on a miss).
 *
 * ---- the entry parameter of a ray into a box, and its margins (csrc/raybox.h; lara_meshray_box_entry_host) ----------------------------
 * fp32 box lo, hi, the ray's constants as above, a window [t_min, t_hi], every operation in double:
 *     an empty box (not lo_x <= hi_x) or a ray that never hits: +inf
 *     per axis a:   e_a = 2^-19 max(|o_a|, |lo_a|, |hi_a|),   l_a = lo_a - e_a,   h_a = hi_a + e_a
 *         d_a == 0:  +inf unless l_a <= o_a <= h_a                                                   (no division)
 *         else       t1 = (l_a - o_a) inv_a,  t2 = (h_a - o_a) inv_a,  n_a = min(t1, t2) - 2^-40 |min|,  f_a = max(t1, t2) + 2^-40 |max|
 *     near = max(t_min, n_x, n_y, n_z),   far = min(t_hi, f_x, f_y, f_z);   near <= far: near, else +inf
 * What has to hold: for every triangle with its three vertices in the box, if lara_raytri COMPUTES a hit at t with the same t_min
 * and t_max = t_hi, the result is finite and <= t.  Computed numbers, as boxbound.h's bound <= d2.  With u = 2^-53:
 *   * the hit passed the sanity clause: the computed x_a = fl(o_a + fl(t d_a)) lies in [fl(mn_a - m_a), fl(mx_a + m_a)].  The box
 *     holds the vertices, so lo_a <= mn_a, mx_a <= hi_a and max(|mn_a|, |mx_a|) <= max(|lo_a|, |hi_a|) =: B_a; with M_a = max(|o_a|, B_a),
 *     m_a <= 2^-20 M_a = e_a / 2.  So x_a lies within [lo_a, hi_a] widened by e_a / 2 (1 + u).
 *   * the exact x*_a = o_a + t d_a (t the computed double) differs from x_a by at most u |t d_a| + u |x_a| <= u (|o_a| + 2 |x_a|)
 *     (1 + u) < 4 u M_a: it lies within [lo_a, hi_a] widened by e_a / 2 + 2^-50 M_a < e_a - 2^-50 M_a, hence strictly inside [l_a, h_a]
 *     as computed (one rounding each, under u (M_a + e_a)).
 *   * d_a == 0: x_a = o_a exactly, and the test above passes.  Else t = (x*_a - o_a) / d_a exactly, which lies between the exact
 *     (l_a - o_a) / d_a and (h_a - o_a) / d_a; the computed t1, t2 carry three roundings each (the difference, inv_a, the product):
 *     a relative 3 u (1 + u), which 2^-40, less its own rounding, covers 2^11 times over.  So n_a <= t <= f_a on every axis, and
 *     t_min <= t <= t_hi by the window: near <= t <= far, near is returned, and it is finite because some d_a != 0.
 *   * outside the derivation: a product that underflows (|t d_a| or |t1| below 2^-1022, which fp32 inputs reach only with
 *     |t| < 2^-873).
 *   * the price: a box is entered although the ray passes up to 2^-19 M_a beside it, or ends 2^-40 t before it.  Nothing measurable.
 * An un-inflated, unwidened slab test violates the contract on flat, axis-aligned triangles (a box without thickness: the exact
 * parameter interval is one point, and the computed t of the hit lies beside it half the time); tests/test_meshray.py keeps that.
 * lara_meshray_box_entry_host: origins, directions HOST [n][3] f32, boxes6 HOST [n][6] f32 (lo, hi), t_min, t_max HOST [n] f32
 * (NULL: 0 and +inf) -> out HOST [n] double.  No device is touched.
 *
 * ---- lara_meshray_cast: the first hit --------------------------------------------------------------------------------------------------
 * origins, directions [R][3] f32, t_min, t_max [R] f32 (NULL: 0 and +inf), bvh as built -> t [R] f32 = (float)t, face [R] i32,
 * bary [R][3] f32 (may be NULL): the three weights rounded once.
 *     face = argmin t (lara_raytri) over the valid triangles the ray hits; an exact tie of t goes to the SMALLER triangle id.
 *     No hit: t = +inf, face = -1, bary = NaN.
 * One thread per ray; no LDS, no atomics, no stack, no seed: the walk of lara_meshbvh_query (csrc/bvhwalk.h) from the root.  A slot
 * is stepped over when its box is empty, when lara_raybox(window [t_min, t_max]) is +inf, or when that entry parameter is STRICTLY
 * greater than the best t so far; at equality the slot is entered, because the tie rule may prefer a smaller id there.  The answer
 * does not depend on the order in which eight siblings are met, the work does: of eight siblings the one at counter c = 0 .. 7 is
 * slot c ^ mask, mask = (d_x < 0) | (d_y < 0) << 1 | (d_z < 0) << 2 -- the bit order of the Morton code that sorted the records, so
 * roughly front to back (LARA_MESHRAY_MASKED_ORDER 1).  lara_meshray_cast_other_order is the same query with the order that was
 * NOT chosen (mask = 0, the stored order), kept for the bench and the tests: the same bits.
 * lara_meshray_occluded: the same walk, ended by the first accepted triangle -> out [R] u8 (1: some triangle is hit in the window).
 *
 * ---- lara_meshray_visible: which eyes see a point ----------------------------------------------------------------------------------------
 * points [N][3] f32, skip_face [N] i32 or NULL, eyes [E][3] f32, E <= LARA_MESHRAY_MAX_EYES = 64, 0 <= shrink < 1 -> seen [N] i64.
 * For point i and eye e the ray is o = eye_e, d = fl32(p_i - eye_e) (t = 1 at the point), the window [0, fl32(1 - shrink)];
 * triangle skip_face[i] (the one the point was sampled from) is ignored.  Bit e of seen[i] is set when NO triangle is hit.  One
 * thread owns one word and loops over the eyes: no atomics.  A point with a coordinate that is not finite has seen = 0.
 *
 * R == 0 or N == 0 is a no-op.  Limits: R, N < 2^30.
 */
#ifndef LARA_MESHRAY_H
#define LARA_MESHRAY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LARA_MESHRAY_MAX_EYES 64
#define LARA_MESHRAY_MASKED_ORDER 1

int lara_meshray_cast(int32_t R, const float *origins, const float *directions, const float *t_min, const float *t_max,
                      const void *bvh, float *t, int32_t *face, float *bary, void *stream);

int lara_meshray_cast_other_order(int32_t R, const float *origins, const float *directions, const float *t_min, const float *t_max,
                                  const void *bvh, float *t, int32_t *face, float *bary, void *stream);

int lara_meshray_occluded(int32_t R, const float *origins, const float *directions, const float *t_min, const float *t_max,
                          const void *bvh, uint8_t *out, void *stream);

int lara_meshray_visible(int32_t N, const float *points, const int32_t *skip_face, int32_t E, const float *eyes, float shrink,
                         const void *bvh, int64_t *seen, void *stream);

int lara_meshray_raytri_host(int64_t n, const float *origins, const float *directions, const float *t_min, const float *t_max,
                             const float *triangles9, uint8_t *hit, double *t, double *bary);

int lara_meshray_box_entry_host(int64_t n, const float *origins, const float *directions, const float *boxes6, const float *t_min,
                                const float *t_max, double *out);

#ifdef __cplusplus
}
#endif
#endif
