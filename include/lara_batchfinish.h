/*
 * lara_batchfinish.h -- the image half of a loader batch, finished from the arrays as they are stored: uint8 RGBA and uint8 normals
 * in, the fp32 colour over each view's background, the uint8 mask and the fp32 normals in the first view's frame out, in the layouts
 * the reference's items collate to (dataLoader/gobjverse.py:82-84, :127-141 do this per item on a CPU worker).  Part of
 * liblara2dgs.so; opt-in, python side: lara_amd/dataset.py (finish_images); kernel: csrc/batchfinish.hip; the per-pixel function, for
 * the device and the host: csrc/batchfinish_ops.h.  Returns 0 or a negative LARA2DGS_E_* code.  Built with -ffp-contract=off: the
 * sequences written here are the instructions.
 *
 * ---- the arrays, all contiguous -----------------------------------------------------------------------------------------------------------
 *     rgba     uint8 [B][V][H][W][4]   the stored image                      bg       fp32 [B][V][3]   each view's background colour
 *     nrm_u8   uint8 [B][V][H][W][3]   the stored normals                    rot      fp32 [B][3][3]   R = transform_mats[b, 0, :3, :3]
 *     out_rgb  fp32  [B][V][H][W][3]   out_msk  uint8 [B][V][H][W]           out_nrm  fp32 [B][H][V W][3]
 * nrm_u8, rot and out_nrm go together: all three null is the rgb-only form.  B V H W < 2^31 pixels in one call (more is refused: the
 * kernel counts pixels in 32 bits and forms byte addresses in 64).  B V H W = 0 does nothing and looks at no pointer.
 *
 * ---- the per-pixel function (csrc/batchfinish_ops.h, the single definition of both answers) -----------------------------------------------
 * fp32, each operation rounded once, no contraction; the reference's numpy float32 expressions operation by operation:
 *     f      = (float)u8 / 255.0f                              the correctly rounded quotient, for all four channels; computed as
 *                                                              q = u r, q + fma(-q, 255, u) r with r = fl(1 / 255): the same 256 words
 *     rgb_c  = f_c * f_a + bg_c * (1.0f - f_a)                 c = 0..2; bg is the colour of the pixel's own view (b, v)
 *     msk    = alpha_u8 > 0 ? 1 : 0
 *     n_k    = f_k * 2.0f - 1.0f                               k = 0..2, f_k of the stored normal's bytes
 *     nrm_j  = (n_0 * R[j][0] + n_1 * R[j][1]) + n_2 * R[j][2] j = 0..2; R is any finite 3x3, nothing is normalised
 *     out_rgb[b][v][h][w][c] = rgb_c     out_msk[b][v][h][w] = msk     out_nrm[b][h][v W + w][j] = nrm_j
 * Nothing is clamped or checked per pixel: an inf or NaN in bg or R propagates as fp32 arithmetic has it.
 *
 * lara_batch_finish: ONE kernel, workgroups of 256 threads, at most LARA_BATCHFINISH_MAX_GROUPS of them striding over the batch.  A
 *     thread takes 4 consecutive pixels of the flat index (b, v, h, w) at a time.  Colour and mask go the wide way -- one 16-byte load of
 *     RGBA, three 16-byte stores of rgb, one 4-byte word of masks -- when H W % 4 == 0 (the four pixels share a view), rgba and out_rgb
 *     are 16-byte aligned and out_msk 4-byte aligned.  Normals go the wide way -- three 4-byte loads, three 16-byte stores, contiguous
 *     in the transposed layout because the four pixels share a row -- when W % 4 == 0, nrm_u8 is 4-byte aligned and out_nrm 16-byte
 *     aligned.  Otherwise (odd shapes, tensor views at a storage offset) the same thread runs the per-pixel function on each of its
 *     pixels with byte and word accesses.  Both ways store the same words.  No LDS, no atomics, no workspace; all pointers are device
 *     pointers; bg and rot are read by the kernel, never on the host.
 * lara_batch_finish_host: the same function over the same arrays in HOST memory, pixel by pixel; no device is touched.
 * Both refuse (LARA2DGS_E_INVALID): a negative dimension, 2^31 pixels or more, and for a batch that is not empty a null rgba, bg,
 * out_rgb or out_msk, or only some of nrm_u8, rot, out_nrm.
 */
#ifndef LARA_BATCHFINISH_H
#define LARA_BATCHFINISH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LARA_BATCHFINISH_MAX_GROUPS 2048

int lara_batch_finish(const uint8_t *rgba, const float *bg, const uint8_t *nrm_u8, const float *rot, int64_t B, int64_t V, int64_t H,
                      int64_t W, float *out_rgb, uint8_t *out_msk, float *out_nrm, void *stream);

int lara_batch_finish_host(const uint8_t *rgba, const float *bg, const uint8_t *nrm_u8, const float *rot, int64_t B, int64_t V, int64_t H,
                           int64_t W, float *out_rgb, uint8_t *out_msk, float *out_nrm);

#ifdef __cplusplus
}
#endif
#endif
