/*
 * lara_splatdensify.h -- one densification round of a cloud of surfels under refinement: clone the small surfels and split the large ones
 * where the screen-space gradient is high, prune the transparent and the oversized, and carry the Adam moments with the rows that
 * survive (part of liblara2dgs.so; opt-in, python side: lara_amd/splatdensify.py; kernels: csrc/splatdensify.hip; the per-row functions,
 * for the device and the host: csrc/splatdensify_ops.h).  Returns 0 or a negative LARA2DGS_E_* code.  Built with -ffp-contract=off: the
 * sequences written here are the instructions.
 *
 * The rules are those of 3DGS's / 2DGS's densify_and_prune as recalled [RECALLED: neither code base is in the build image; nothing pins
 * them], with ONE deliberate difference: 3DGS applies its prune test after the new rows exist, with a zero screen radius for them; here
 * a row that fails the test leaves no descendants.
 *
 * ---- the cloud ---------------------------------------------------------------------------------------------------------------------------
 * P surfels as Renderer.render_views takes them, every value pre-activation, fp32, rows contiguous:
 *     centers [P][3]   shs [P][n][3], n = (sh_degree + 1)^2, sh_degree in 0..3   opacity [P][1]   scales [P][2]   rotations [P][4]
 * and the two Adam moments of each (exp_avg, exp_avg_sq): 15 arrays, handed over as a HOST array of 15 pointers in the order
 * parameters (the five fields), exp_avg (the five fields), exp_avg_sq (the five fields).  P <= 2^27.
 *
 * ---- 1. statistics: lara_splatdensify_accumulate --------------------------------------------------------------------------------------------
 * grad_means2D [P][3] fp32 is what the rasteriser hands back for its means2D argument; radii [V][P] int32 what it returns.  In/out rows
 * [P]: grad_sum (fp32), seen (int32), max_radius (int32).  A surfel is seen when any radii[v][s] > 0.  For a seen surfel:
 *     n = sqrt(gx gx + gy gy)      in double on the fp32 words gx = grad[s][0], gy = grad[s][1]
 *     n finite (gx and gy finite):  grad_sum <- fl32(double(grad_sum) + n),   seen <- seen + 1
 *     max_radius <- max(max_radius, max_v radii[v][s])                        either way
 * Rows of unseen surfels keep their bits.  The rasteriser sums the screen-space gradient over the views of one call, so the statistic
 * is PER RENDER CALL, not per view: one call of V views adds one norm (of the summed gradient) and one count.  A loop that renders one
 * view per step accumulates 3DGS's per-view statistic.  One launch, one thread per surfel.
 *
 * ---- 2. decision: lara_splatdensify_decide -------------------------------------------------------------------------------------------------
 * The plan: LARA_SPLATDENSIFY_PLAN = 8 doubles in HOST memory, built in float64 by lara_amd.splatdensify.plan (no exp, log or sigmoid
 * runs in the kernel), passed to the kernel by value:
 *     [0] grad_threshold   [1] log_dense = log(percent_dense extent)   [2] logit_min_opacity   [3] max_screen_radius (<= 0: off)
 *     [4] log_max_world = log(0.1 extent)   [5] log_shrink = log(0.8 N)   [6] N, the children per split, 1..8
 *     [7] flags: 1 allow clone, 2 allow split, 4 allow prune
 * Per surfel, on the stored opacity logit and log scales:
 *     avg = seen > 0 ? double(grad_sum) / seen : 0        hot = avg >= grad_threshold (a NaN is not hot)
 *     smax = scales[s][0] > scales[s][1] ? scales[s][0] : scales[s][1]
 *     prune   (flag 4) opacity < logit_min_opacity, or a non-finite opacity or scale word, or -- max_screen_radius > 0 --
 *             max_radius > max_screen_radius or smax > log_max_world
 *     split   else hot and smax > log_dense    (flag 2; without it: keep)
 *     clone   else hot and smax <= log_dense   (flag 1; without it: keep)
 *     keep    otherwise
 * Outputs: action [P] uint8 (0 keep, 1 clone, 2 split, 3 prune); offset [3 P] int32, the EXCLUSIVE scan of the concatenation
 * [1 per keep or clone | 1 per clone | N per split]; counts: five int64 on the device -- kept (action keep), cloned, split parents,
 * pruned, P_out = kept + 2 cloned + N split.  The output order is thereby fixed, and it is 3DGS's: the surviving originals in ascending
 * order, then the clones ascending by source, then the split children ascending by source, child 0 .. N - 1.
 * Launches: the decide kernel (action and flags), the three-launch scan of csrc/unigrid.h into `workspace`
 * (lara_splatdensify_workspace_bytes(P) bytes of device memory), one pass that turns the scan exclusive and stores the counts.  No wave
 * waits for another wave's flag.  P = 0 zeroes the counts.
 *
 * ---- 3. application: lara_splatdensify_apply -----------------------------------------------------------------------------------------------
 * P_out and survivors = kept + cloned are the caller's, read from `counts`: the single host read of a round, needed to allocate.
 * `in` and `out` are the 15 arrays of the cloud before (P rows) and after (P_out rows); they do not overlap.  Two launches:
 *     rows     one thread per source surfel, through `offset`: row_source [P_out] int32, row_child [P_out] uint8 (255: not a split child)
 *     gather   one thread per output word of a parameter, 256 words of one field per workgroup; the thread stores the parameter word
 *              and the two moment words
 * Values of output row o with source s = row_source[o]:
 *     kept and cloned rows      parameter words are copied bit for bit
 *     kept rows (o < survivors) moment words are copied bit for bit
 *     clones and split children moments are +0.0
 *     split child k             shs, opacity and rotation copied; log scales fl32(double(scale) - log_shrink); centre, in double,
 *                               (w, x, y, z) = q / |q| with |q|^2 = ((w w + x x) + y y) + z z and 1 / sqrt, R the rasteriser's matrix of it,
 *                               u = exp(s0) z0, v = exp(s1) z1, z = noise[s][k][0:2], centre[r] <- fl32(c[r] + (R[r][0] u + R[r][1] v))
 * noise [P][N][2] fp32 is the caller's (python fills it with torch.randn under a seeded generator): no random-number generator runs in
 * the kernel, so a round is reproducible and restatable.  The double exp is the one operation that is not correctly rounded: two
 * correct implementations may differ in the last bit of a child's centre word, and no more.  A row at or beyond P_out is not written,
 * a source outside 0 .. P - 1 is not read.  P = 0 or P_out = 0 launches nothing.
 *
 * Every entry has a _host twin that runs the same per-row functions over HOST memory, row by row: the reference the kernels are held
 * to, not a fast path.  All refuse (LARA2DGS_E_INVALID): a null pointer, P < 0 or P > 2^27, V outside 1..4096, sh_degree outside 0..3,
 * a plan whose N is not an integer in 1..8 or whose flags are not an integer in 0..7, P_out > 9 P, survivors > min(P, P_out).
 */
#ifndef LARA_SPLATDENSIFY_H
#define LARA_SPLATDENSIFY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LARA_SPLATDENSIFY_PLAN 8
#define LARA_SPLATDENSIFY_SPAN 256

int lara_splatdensify_accumulate(int64_t P, int32_t V, const float *grad_means2D, const int32_t *radii, float *grad_sum, int32_t *seen,
                                 int32_t *max_radius, void *stream);
int lara_splatdensify_accumulate_host(int64_t P, int32_t V, const float *grad_means2D, const int32_t *radii, float *grad_sum, int32_t *seen,
                                      int32_t *max_radius);

int64_t lara_splatdensify_workspace_bytes(int64_t P);
int lara_splatdensify_decide(const double *plan, int64_t P, const float *opacity, const float *scales, const float *grad_sum,
                             const int32_t *seen, const int32_t *max_radius, uint8_t *action, int32_t *offset, int64_t *counts,
                             void *workspace, void *stream);
int lara_splatdensify_decide_host(const double *plan, int64_t P, const float *opacity, const float *scales, const float *grad_sum,
                                  const int32_t *seen, const int32_t *max_radius, uint8_t *action, int32_t *offset, int64_t *counts,
                                  void *workspace);

int lara_splatdensify_apply(const double *plan, int32_t sh_degree, int64_t P, int64_t P_out, int64_t survivors, const uint8_t *action,
                            const int32_t *offset, const float *noise, const float *const *in, float *const *out, int32_t *row_source,
                            uint8_t *row_child, void *stream);
int lara_splatdensify_apply_host(const double *plan, int32_t sh_degree, int64_t P, int64_t P_out, int64_t survivors, const uint8_t *action,
                                 const int32_t *offset, const float *noise, const float *const *in, float *const *out, int32_t *row_source,
                                 uint8_t *row_child);

#ifdef __cplusplus
}
#endif
#endif
