/*
 * lara_splatxform.h -- a similarity T = [[sR, t], [0, 1]] (s > 0, R a proper rotation) applied to a cloud of predicted surfels: centres,
 * log scales, the quaternion and the view-dependent colour, whose SH coefficients of bands 1..3 are rotated in the rasteriser's own
 * basis (csrc/preprocess.hip: the 3DGS constants, signs and band order), so that the moved cloud seen from a camera moved with it
 * renders as the original did (part of liblara2dgs.so; opt-in, python side: lara_amd/splatxform.py; kernel: csrc/splatxform.hip; the
 * per-surfel function, for the device and the host: csrc/splatxform_ops.h).  Returns 0 or a negative LARA2DGS_E_* code.  Built with
 * -ffp-contract=off: the sequences written here are the instructions.
 *
 * ---- the cloud ---------------------------------------------------------------------------------------------------------------------------
 * P surfels as Renderer.render_img takes them, every value pre-activation, fp32, rows contiguous:
 *     centers [P][3]   shs [P][n][3], n = (sh_degree + 1)^2, sh_degree in 0..3   opacity [P][1]   scales [P][2]   rotations [P][4] (w, x, y, z)
 * The five outputs have the same row shapes and out_rows rows; the call writes rows [out_row0, out_row0 + P) of them and nothing else.
 * An output may be its input (out_row0 = 0: in place); any other overlap of an output with an input is the caller's to refuse.
 *
 * ---- the plan: LARA_SPLATXFORM_PLAN = 100 doubles in HOST memory (both entry points), built by lara_amd.splatxform.similarity ----------------
 *     [0:9]    A = sR, row-major                        [9:12]  t
 *     [12:16]  r, the unit quaternion of R (w, x, y, z) [16]    log s
 *     [17:26]  D1 [3][3]    [26:51]  D2 [5][5]    [51:100]  D3 [7][7], row-major: the rotation of band l in the rasteriser's basis,
 *              sum_m (Dl c)_m Y_m(R d) = sum_m c_m Y_m(d) for every unit d
 * The device entry passes the plan to the kernel by value, in its arguments (800 bytes): no device buffer, no copy.
 *
 * ---- the per-surfel function (csrc/splatxform_ops.h, the single definition of both answers) ----------------------------------------------
 * All arithmetic is double on the fp32 inputs; every output is rounded to fp32 once.  fl32(v) below is that rounding, and a NaN is
 * stored as the one word 0x7FC00000: an invalid operation (inf - inf, 0 inf) has another sign on the host than on the device and the
 * payload that survives two NaN operands is the compiler's choice, so the payload is no part of the answer.  Nothing else is
 * clamped, checked or refused per surfel: NaN and inf propagate, and a zero quaternion stays zero.
 *     centre    c'_i = fl32(((A_i0 x + A_i1 y) + A_i2 z) + t_i)                 (the bits of lara_meshalign_transform on the same points)
 *     rotation  q' = r (x) q, the Hamilton product, so that R(q') = R R(q) and |q'| = |q| (q is not normalised here):
 *                   w' = fl32(((r_w q_w - r_x q_x) - r_y q_y) - r_z q_z)
 *                   x' = fl32(((r_w q_x + r_x q_w) + r_y q_z) - r_z q_y)
 *                   y' = fl32(((r_w q_y - r_x q_z) + r_y q_w) + r_z q_x)
 *                   z' = fl32(((r_w q_z + r_x q_y) - r_y q_x) + r_z q_w)
 *     scales    s'_k = fl32((double)s_k + log s)
 *     opacity, SH band 0 (shs[p][0][.])                                         the words are copied
 *     SH band l = 1..sh_degree, per channel ch, c_j = shs[p][l^2 + j][ch], j = 0..2l:
 *                   c'_i = fl32((..((Dl_i0 c_0 + Dl_i1 c_1) + Dl_i2 c_2) + ..) + Dl_i,2l c_2l)      (the first product, then ascending j)
 *
 * lara_splatxform_apply: ONE kernel, one workgroup of 256 threads per span of LARA_SPLATXFORM_SPAN consecutive surfels.  The
 *     workgroup loads the span of each of the five arrays as the contiguous bytes it is (16-byte loads where the address allows, lane i
 *     next to lane i + 1) into LDS, every thread transforms one row there, and the span is stored the same way.  A workgroup has read
 *     all of its span before it writes any of it, and no workgroup reads another's span: that is what makes the in-place call safe.
 *     No atomics, no scratch, no workspace.  P = 0 launches nothing.  All ten pointers are device pointers.
 * lara_splatxform_apply_host: the same function over the same arrays in HOST memory, row by row; no device is touched.
 * Both refuse (LARA2DGS_E_INVALID): a null pointer (the plan included), sh_degree outside 0..3, P < 0, out_row0 < 0,
 * out_row0 + P > out_rows.
 */
#ifndef LARA_SPLATXFORM_H
#define LARA_SPLATXFORM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LARA_SPLATXFORM_PLAN 100
#define LARA_SPLATXFORM_SPAN 256

int lara_splatxform_apply(const double *plan, int32_t sh_degree, int64_t P, const float *centers, const float *shs, const float *opacity,
                          const float *scales, const float *rotations, float *out_centers, float *out_shs, float *out_opacity,
                          float *out_scales, float *out_rotations, int64_t out_row0, int64_t out_rows, void *stream);

int lara_splatxform_apply_host(const double *plan, int32_t sh_degree, int64_t P, const float *centers, const float *shs,
                               const float *opacity, const float *scales, const float *rotations, float *out_centers, float *out_shs,
                               float *out_opacity, float *out_scales, float *out_rotations, int64_t out_row0, int64_t out_rows);

#ifdef __cplusplus
}
#endif
#endif
