/*
 * meshio/lara_meshio.h -- the extracted mesh as file bytes, built on the device: Wavefront OBJ text (the bytes lara_amd.mesh.write_obj
 * writes) and binary little-endian PLY (part of liblara2dgs.so; opt-in, python side: lara_amd/meshio.py; kernels: csrc/meshio.hip;
 * the number formatting: csrc/fmt9g.h).  All pointers are device pointers unless a parameter says HOST.  Returns 0 or a negative
 * LARA2DGS_E_* code.  Work is enqueued on `stream`; no function here waits for it or reads anything back.  Integer arithmetic only,
 * apart from the colour rule of the PLY rows (double).
 *
 * ---- conventions ------------------------------------------------------------------------------------------------------------------
 * vertices, colors, normals [nv][3] f32 (colors / normals may be NULL).  triangles [nt][3], int32 or int64 by `index_bytes` (4 or 8).
 * Limits: 0 <= nv <= LARA_MESHIO_MAX_VERTICES, 0 <= nt <= LARA_MESHIO_MAX_TRIANGLES (nv < 2^31, 3 nt < 2^31).
 * An index is IN RANGE when 0 <= index <= LARA_MESHIO_MAX_INDEX (2^31 - 2: the 1-based OBJ index still fits an int32); it is not
 * compared with nv (write_obj does not either).  An index out of range sets bit 0 of the call's ERROR WORD (an int64 in the
 * workspace, zeroed by the call before its kernels run) and is written as if it were 0, so that no length depends on it.
 * One thread per line / row, LARA_MESHIO_BLOCK_LINES of them per workgroup.  A workgroup's lines are adjacent in the file: it builds
 * them in LDS and copies the span out with aligned 16-byte stores, byte stores only for the unaligned head and tail.  No byte outside
 * the span is written.  All offsets are int64.
 *
 * ---- OBJ: lara_meshio_obj_lengths, lara_meshio_obj_emit ----------------------------------------------------------------------------
 * The text: one line "v x y z\n" or "v x y z r g b\n" per vertex, then one line "f a b c\n" per triangle (a = index + 1, decimal).
 * A number is C's "%.9g" of the fp32 value taken to double (csrc/fmt9g.h: exact for all 2^32 bit patterns; the longest token has
 * LARA_MESHIO_MAX_F32_TOKEN characters, an index LARA_MESHIO_MAX_U32_TOKEN at the most), so a vertex line has at most
 * LARA_MESHIO_MAX_VERTEX_LINE = 1 + 6 (1 + 15) + 1 bytes and a face line LARA_MESHIO_MAX_FACE_LINE = 1 + 3 (1 + 10) + 1.
 * Blocks: bv = ceil(nv / 256) vertex blocks, then bt = ceil(nt / 256) face blocks.
 *   _lengths: workspace (lara_meshio_obj_workspace_bytes(nv, nt) bytes, 8-byte aligned) = int64 totals[bv + bt], the bytes of each
 *             block's lines, then the int64 error word.  Two launches (vertex lines, face lines).
 *   the caller turns the totals into exclusive offsets (a scan) and reads the grand total and the error word,
 *   _emit:    block_offsets int64 [bv + bt], out: room for the grand total.  Two launches.  Block b's lines start at
 *             out + block_offsets[b]; within the block a line's offset is the in-block exclusive scan of the lengths.
 * nv == 0 and nt == 0: a no-op.
 *
 * ---- PLY: lara_meshio_ply_pack ------------------------------------------------------------------------------------------------------
 * The BODY of a binary_little_endian 1.0 file (the header text, about 300 bytes, is the caller's): nv packed vertex rows
 *     float x, y, z  [float nx, ny, nz]  [uchar red, green, blue]            12, 15, 24 or 27 bytes
 * then nt packed face rows of LARA_MESHIO_PLY_FACE_ROW bytes: the byte 3, then three little-endian int32 indices, 0-based.
 * Floats are bit copies.  A colour c becomes floor(255.0 * (double)min(max(c, 0), 1) + 0.5), NaN becomes 0 (exact in double).
 * out: room for lara_meshio_ply_body_bytes(nv, nt, has_normals, has_colors).  workspace: lara_meshio_ply_workspace_bytes() bytes,
 * the int64 error word.  One launch per part; offsets are closed-form.
 *
 * ---- host-only entries ----------------------------------------------------------------------------------------------------------------
 * lara_meshio_format_f32_host / _u32_host run the formatting routines of csrc/fmt9g.h on the CPU: HOST v [n], HOST out [16 n] /
 * [10 n] (token i starts at 16 i / 10 i; nothing beyond its length is written), HOST len [n].  LARA2DGS_E_INVALID for n < 0 or a
 * null pointer with n > 0; n == 0 is a no-op.
 */
#ifndef LARA_MESHIO_H
#define LARA_MESHIO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LARA_MESHIO_BLOCK_LINES 256
#define LARA_MESHIO_MAX_F32_TOKEN 15
#define LARA_MESHIO_MAX_U32_TOKEN 10
#define LARA_MESHIO_MAX_VERTEX_LINE 98
#define LARA_MESHIO_MAX_FACE_LINE 35
#define LARA_MESHIO_PLY_FACE_ROW 13
#define LARA_MESHIO_MAX_VERTICES 2147483647
#define LARA_MESHIO_MAX_TRIANGLES 715827882
#define LARA_MESHIO_MAX_INDEX 2147483646
#define LARA_MESHIO_ERR_INDEX 1

int64_t lara_meshio_obj_workspace_bytes(int64_t nv, int64_t nt);

int lara_meshio_obj_lengths(int64_t nv, const float *vertices, const float *colors, int64_t nt, const void *triangles,
                            int32_t index_bytes, void *workspace, void *stream);

int lara_meshio_obj_emit(int64_t nv, const float *vertices, const float *colors, int64_t nt, const void *triangles, int32_t index_bytes,
                         const int64_t *block_offsets, uint8_t *out, void *stream);

int64_t lara_meshio_ply_body_bytes(int64_t nv, int64_t nt, int32_t has_normals, int32_t has_colors);

int64_t lara_meshio_ply_workspace_bytes(void);

int lara_meshio_ply_pack(int64_t nv, const float *vertices, const float *normals, const float *colors, int64_t nt, const void *triangles,
                         int32_t index_bytes, uint8_t *out, void *workspace, void *stream);

int lara_meshio_format_f32_host(int64_t n, const float *v, char *out, int *len);

int lara_meshio_format_u32_host(int64_t n, const uint32_t *v, char *out, int *len);

#ifdef __cplusplus
}
#endif
#endif
