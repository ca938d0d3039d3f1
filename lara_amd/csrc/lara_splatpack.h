/*
 * lara_splatpack.h -- packing a cloud of surfels for Gaussian-splat viewers: the web viewers' compressed PLY (16 bytes per surfel plus a
 * 72-byte record per 256 surfels, plus quantised SH) and the 32-byte .splat row, and the reverse of both (part of liblara2dgs.so; opt-in,
 * python side: lara_amd/splatpack.py, which binds these functions itself; kernels: csrc/splatpack.hip; the per-row functions, for the
 * device and the host: csrc/splatpack_ops.h).  Returns 0 or a negative LARA2DGS_E_* code.  Built with -ffp-contract=off: the sequences
 * written here are the instructions.
 *
 * The formats are the PlayCanvas / SuperSplat compressed PLY and the antimatter15 .splat as recalled [RECALLED: neither code base is in
 * the build image; nothing pins parity with the viewers' own readers].
 *
 * ---- the cloud ---------------------------------------------------------------------------------------------------------------------------
 * P surfels as Renderer.render_views takes them, every value pre-activation, fp32, rows contiguous, handed over as a HOST array `in` of
 * five pointers:  centers [P][3]   shs [P][n][3], n = (sh_degree + 1)^2   opacity [P][1]   scales [P][2]   rotations [P][4] (w, x, y, z).
 * P <= 2^27.  All arithmetic is double on the fp32 words, with one rounding fl32 per stored fp32.
 *     pack(x, b) = clamp(floor(x (2^b - 1) + 0.5), 0, 2^b - 1)        C0 = 0.28209479177387814        canon(v) = v + 0.0f (-0.0 -> +0.0)
 * The plan: LARA_SPLATPACK_PLAN = 2 doubles in HOST memory: [0] s2 = fl32(log(thickness)), [1] fl32(thickness).
 *
 * ---- 1. lara_splatpack_bounds ----------------------------------------------------------------------------------------------------------
 * valid [P] uint8: 1 where every word of the row's five fields is finite and ((w w + x x) + y y) + z z of its quaternion is > 0 and
 * finite.  box [6] fp32: the minimum and the maximum of canon(centre) over the valid rows, (lo xyz, hi xyz); (+inf, -inf) without one.
 * dropped: one int64 on the device, the invalid rows.  Two launches: 256 rows per workgroup into `workspace`
 * (lara_splatpack_workspace_bytes(P) bytes of device memory), one workgroup over the partial results; no float atomics.
 *
 * ---- 2. lara_splatpack_morton_keys, lara_splatpack_importance_keys -----------------------------------------------------------------------
 * keys [P] int64, to be sorted ascending by the caller; the row is a key's low 31 bits.  An invalid row: 1 << 62 | row.
 *     morton      q = min(1023, floor((canon(v) - lo) / (hi - lo) 1024)), 0 where hi == lo; 30 bits, x the most significant bit of each
 *                 triple; key = morton << 32 | row
 *     importance  i = fl32(exp((s0 + s1) + s2) / (1 + exp(-o))); key = (0x7FFFFFFF - bits(i)) << 31 | row: descending importance
 *                 (31 and not 32: a row index fits 27 bits, and a shift of 32 would carry small importances past the invalid rows' bit 62)
 *
 * ---- 3. lara_splatpack_encode ------------------------------------------------------------------------------------------------------------
 * order [P_out] int64: the source row of every output row.  Chunk c is output rows 256 c .. 256 c + 255, the last one may be partial.
 * chunks [C][18] fp32, C = ceil(P_out / 256):  min xyz, max xyz | min scale xyz, max scale xyz | min rgb, max rgb  over the chunk's
 * own rows of   canon(centre) | canon(clamp(s, -20, 20)) with s2 as z | canon(k), k = fl32(0.5 + C0 f_dc).
 * words [P_out][4] uint32 (16-byte aligned), n = (v - min) / (max - min), 0 where max == min:
 *     [0] position  pack(nx, 11) << 21 | pack(ny, 10) << 11 | pack(nz, 11)
 *     [1] rotation  q = (w, x, y, z) / sqrt(|q|^2); L the smallest index of the largest |q_i|; q negated where q_L < 0;
 *                   L << 30 | pack(q_a 0.70710678118654752 + 0.5, 10) << 20 | .. << 10 | ..  over the other three, ascending index
 *     [2] scale     as the position, on the clamped log scales
 *     [3] colour    pack(nr, 8) << 24 | pack(ng, 8) << 16 | pack(nb, 8) << 8 | pack(1 / (1 + exp(-o)), 8)
 * sh [P_out][3 (n - 1)] uint8: byte c (n - 1) + k = clamp(floor((shs[1 + k][c] / 8 + 0.5) 256), 0, 255).
 * One launch, one workgroup of 256 threads per chunk.  A source row outside 0 .. P - 1 takes no part in the bounds and packs to zeros.
 *
 * ---- 4. lara_splatpack_decode ------------------------------------------------------------------------------------------------------------
 * `out`: five pointers, P_out rows.  centre, scales, k: fl32(min + code / (2^b - 1) (max - min)), f_dc = (k - 0.5) / C0 (k kept in double);
 * rotation components (code / 1023 - 0.5) 1.4142135623730951, the largest sqrt(max(0, 1 - sum of squares)); opacity
 * log(a / (1 - a)), a = clamp(code, 0.5, 254.5) / 255; SH ((code + 0.5) / 256 - 0.5) 8.  Scale z is not decoded.  One thread per row.
 *
 * ---- 5. lara_splatpack_splat_encode / _decode --------------------------------------------------------------------------------------------
 * rows [P_out][8] uint32 (32 bytes, 16-byte aligned): the centre's three words; fl32(exp(s0)), fl32(exp(s1)), fl32(thickness); bytes
 * pack(clamp(k, 0, 1), 8) for r, g, b and pack(alpha, 8); bytes clamp(floor(q_i / |q| 128 + 128 + 0.5), 0, 255) for w, x, y, z.  Decoding:
 * the centre's words, fl32(log(e)), f_dc = (byte / 255 - 0.5) / C0, the logit as above, (byte - 128) / 128; SH band 0 only.
 *
 * Every entry has a _host twin that runs the same per-row functions over HOST memory, row by row: the reference the kernels are held
 * to, not a fast path.  All refuse (LARA2DGS_E_INVALID): a null pointer, P or P_out < 0 or > 2^27, P_out > P where both are given,
 * sh_degree outside 0..3, words or rows off a 16-byte boundary, a grid beyond one launch.  P = 0 or P_out = 0 launches nothing (bounds
 * still stores the empty box and the count).
 */
#ifndef LARA_SPLATPACK_H
#define LARA_SPLATPACK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LARA_SPLATPACK_PLAN 2
#define LARA_SPLATPACK_SPAN 256

int64_t lara_splatpack_workspace_bytes(int64_t P);
int lara_splatpack_bounds(int32_t sh_degree, int64_t P, const float *const *in, uint8_t *valid, float *box, int64_t *dropped, void *workspace,
                          void *stream);
int lara_splatpack_bounds_host(int32_t sh_degree, int64_t P, const float *const *in, uint8_t *valid, float *box, int64_t *dropped,
                               void *workspace);

int lara_splatpack_morton_keys(int64_t P, const float *centers, const uint8_t *valid, const float *box, int64_t *keys, void *stream);
int lara_splatpack_morton_keys_host(int64_t P, const float *centers, const uint8_t *valid, const float *box, int64_t *keys);
int lara_splatpack_importance_keys(const double *plan, int64_t P, const float *opacity, const float *scales, const uint8_t *valid,
                                   int64_t *keys, void *stream);
int lara_splatpack_importance_keys_host(const double *plan, int64_t P, const float *opacity, const float *scales, const uint8_t *valid,
                                        int64_t *keys);

int lara_splatpack_encode(const double *plan, int32_t sh_degree, int64_t P, int64_t P_out, const float *const *in, const int64_t *order,
                          float *chunks, uint32_t *words, uint8_t *sh, void *stream);
int lara_splatpack_encode_host(const double *plan, int32_t sh_degree, int64_t P, int64_t P_out, const float *const *in, const int64_t *order,
                               float *chunks, uint32_t *words, uint8_t *sh);
int lara_splatpack_decode(int32_t sh_degree, int64_t P_out, const float *chunks, const uint32_t *words, const uint8_t *sh, float *const *out,
                          void *stream);
int lara_splatpack_decode_host(int32_t sh_degree, int64_t P_out, const float *chunks, const uint32_t *words, const uint8_t *sh,
                               float *const *out);

int lara_splatpack_splat_encode(const double *plan, int32_t sh_degree, int64_t P, int64_t P_out, const float *const *in, const int64_t *order,
                                uint32_t *rows, void *stream);
int lara_splatpack_splat_encode_host(const double *plan, int32_t sh_degree, int64_t P, int64_t P_out, const float *const *in,
                                     const int64_t *order, uint32_t *rows);
int lara_splatpack_splat_decode(int64_t P_out, const uint32_t *rows, float *const *out, void *stream);
int lara_splatpack_splat_decode_host(int64_t P_out, const uint32_t *rows, float *const *out);

#ifdef __cplusplus
}
#endif
#endif
