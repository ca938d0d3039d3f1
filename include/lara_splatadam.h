/*
 * lara_splatadam.h -- one Adam step over the five tensors of a cloud of predicted surfels, with the gates the Gaussian-splatting code
 * bases put on it: surfels no view saw keep their parameters and their moments (3DGS's "sparse Adam"), a non-finite gradient word
 * skips its element, and the gradients may be zeroed in the same pass (part of liblara2dgs.so; opt-in, python side:
 * lara_amd/splatrefine.py; kernel: csrc/splatadam.hip; the per-word function, for the device and the host: csrc/splatadam_ops.h).
 * Returns 0 or a negative LARA2DGS_E_* code.  Built with -ffp-contract=off: the sequences written here are the instructions.
 *
 * ---- the cloud ---------------------------------------------------------------------------------------------------------------------------
 * P surfels as Renderer.render_views takes them, every value pre-activation, fp32, rows contiguous:
 *     centers [P][3]   shs [P][n][3], n = (sh_degree + 1)^2, sh_degree in 0..3   opacity [P][1]   scales [P][2]   rotations [P][4]
 * Each field f has four arrays of that shape: the parameter p_f, its gradient g_f and the two moments m_f, v_f (torch.optim.Adam's
 * exp_avg and exp_avg_sq).  The twenty arrays do not overlap.
 *
 * ---- the plan: LARA_SPLATADAM_PLAN = 13 doubles in HOST memory (both entry points), built by lara_amd.splatrefine.plan ----------------------
 *     [0] b1   [1] 1 - b1   [2] b2   [3] 1 - b2   [4] bc1 = 1 - b1^t   [5] sqrt(bc2), bc2 = 1 - b2^t   [6] eps
 *     [7:13]   the learning rates of: centers, SH coefficient 0 (shs[p][0][.]), SH coefficients >= 1, opacity, scales, rotations
 * t is the 1-based step; the powers and the root are float64 on the host, no pow runs in the kernel.  The device entry passes the plan
 * to the kernel by value, in its arguments: no device buffer, no copy, no host read.
 *
 * ---- the per-word function (csrc/splatadam_ops.h, the single definition of both answers) --------------------------------------------------
 * torch.optim.Adam's formula in double on the fp32 words, + - * / and sqrt only, each a correctly rounded IEEE operation, left to right
 * as bracketed; fl32 is the one rounding at a store (a NaN is stored as 0x7FC00000):
 *     m' = m + (g - m) (1 - b1)
 *     v' = b2 v + ((1 - b2) g) g
 *     p' = p - (lr_f / bc1) (m' / (sqrt(v') / sqrt(bc2) + eps))          from the unrounded m', v'
 *     m <- fl32(m')   v <- fl32(v')   p <- fl32(p')
 * lr_f is the field's rate; inside shs it is chosen by the word's index modulo 3 n (< 3: coefficient 0).  A finite gradient whose
 * (1 - b2) g^2 is beyond fp32 (|g| > ~5.8e20 at b2 = 0.999) leaves v = inf, as torch's fp32 Adam does: p stays finite, and the element
 * no longer moves.
 *
 * ---- the gates -----------------------------------------------------------------------------------------------------------------------------
 *     visible     uint8 [P] or NULL.  NULL is dense mode: torch.optim.Adam's semantics.  Where visible[s] == 0 the words of p, m and v
 *                 of surfel s (= word index / the field's width) are not written: they keep their bits.  Its gradient is not looked at.
 *     non-finite  a gradient word that is inf or NaN (of a visible surfel) skips its element: p, m and v keep their bits, and the word
 *                 is counted in *skipped (int64, added to, never zeroed here; may be NULL on neither entry).
 *     zero_grads  != 0: +0.0 is stored over EVERY gradient word, skipped and invisible ones included.
 *
 * lara_splatadam_step: ONE kernel, one thread per word, 256 words of one field per workgroup; a table of six block offsets in the
 *     kernel's arguments maps a workgroup to its field, so lane i and lane i + 1 touch consecutive words of every array they read or
 *     write (of `visible`, the same or consecutive bytes).  The count goes through one ballot per wave and at most one 64-bit integer
 *     atomic per wave.  No LDS, no scratch, no workspace.  P = 0 launches nothing.  The pointers are device pointers (the plan: host).
 * lara_splatadam_step_host: the same function over the same arrays in HOST memory, field by field, word by word; no device is touched.
 * Both refuse (LARA2DGS_E_INVALID): a null pointer (the plan and the counter included; `visible` may be), sh_degree outside 0..3, P < 0,
 * P so large that the launch would need 2^31 workgroups.
 */
#ifndef LARA_SPLATADAM_H
#define LARA_SPLATADAM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LARA_SPLATADAM_PLAN 13
#define LARA_SPLATADAM_SPAN 256

int lara_splatadam_step(const double *plan, int32_t sh_degree, int64_t P, float *centers, float *shs, float *opacity, float *scales,
                        float *rotations, float *g_centers, float *g_shs, float *g_opacity, float *g_scales, float *g_rotations,
                        float *m_centers, float *m_shs, float *m_opacity, float *m_scales, float *m_rotations, float *v_centers,
                        float *v_shs, float *v_opacity, float *v_scales, float *v_rotations, const uint8_t *visible, int32_t zero_grads,
                        int64_t *skipped, void *stream);

int lara_splatadam_step_host(const double *plan, int32_t sh_degree, int64_t P, float *centers, float *shs, float *opacity, float *scales,
                             float *rotations, float *g_centers, float *g_shs, float *g_opacity, float *g_scales, float *g_rotations,
                             float *m_centers, float *m_shs, float *m_opacity, float *m_scales, float *m_rotations, float *v_centers,
                             float *v_shs, float *v_opacity, float *v_scales, float *v_rotations, const uint8_t *visible,
                             int32_t zero_grads, int64_t *skipped);

#ifdef __cplusplus
}
#endif
#endif
