/*
 * meshrender/lara_meshrender.h -- a deterministic z-buffer rasteriser for the extracted mesh's turntable (evaluation.py:150-155 goes through
 * tools/meshRender.py, i.e. Mitsuba; that image is not imitated) on the device (part of liblara2dgs.so; opt-in, python side:
 * lara_amd/meshrender.py; kernels: csrc/meshrender.hip).  Many small triangles in, exact visibility, depth, face normals and uint8
 * frames out, from the cameras and in the pixel convention of the surfel rasteriser: a mesh frame and a surfel frame of one camera
 * register pixel for pixel.
 *
 * Inputs.  vertices [Nv][3] f32, triangles [T][3] i32, vertex_colors [Nv][3] f32 or NULL (NULL: the constant albedo);
 * viewmatrix / projmatrix [n_views][16] and campos [n_views][3] as lara_amd.cameras builds them for the rasteriser (row-vector
 * convention: clip = [x y z 1] M, M flat with element (a, j) at 4 a + j) -- except that `campos` is the camera's true position (the
 * eye), not the reference MiniCam's negated translation.  All device pointers; `shading` is a HOST pointer to
 * LARA_MESHRENDER_SHADING_FLOATS floats: albedo r g b, background r g b, ambient, diffuse.
 *
 * Stage V, one thread per (view, vertex), every operation fp32 in the order written, nothing fused:
 *     h_j  = ((M[0][j] x + M[1][j] y) + M[2][j] z) + M[3][j]        for j = 0 (x), 1 (y), 3 (w) of projmatrix
 *     z    = ((V[0][2] x + V[1][2] y) + V[2][2] z) + V[3][2]        of viewmatrix: the view-space depth
 *     pixel_x = (((h_0 / h_3) + 1) W - 1) / 2,  pixel_y likewise with H                   (sample points at integer pixels)
 *     snapped = rint(pixel * 256) as int32; LARA_MESHRENDER_FAR (2^30) where |pixel * 256| >= 2^30 or it is not a number
 * stored as the record {int32 x, int32 y, float z, int32 0} at workspace + 16 (view * Nv + vertex): the SNAP section.
 *
 * Stage R.  A triangle is DROPPED, and counted in `info`, by the first of these that holds: any vertex has z <= znear (behind);
 * any snapped coordinate lies beyond +-2^22 units (out of range); its integer area is zero (degenerate).  THERE IS NO CLIPPING: a
 * triangle that crosses the near plane disappears as a whole.  Turntable cameras stand outside the object; a caller who moves the
 * camera into the mesh reads the loss in info[1].  A triangle with an index outside [0, Nv) is dropped, counted nowhere, and sets
 * bit 0 of *err (`err`: one device int32 the caller zeroes and reads when it reads anything else; may be NULL).
 * Triangles are two-sided (no back-face culling).  Coverage is exact integer arithmetic on the snapped coordinates: with the
 * vertices ordered so that area = E(v0, v1, v2) > 0, E(a, b, p) = (bx - ax)(py - ay) - (by - ay)(px - ax) in int64, the sample
 * p = (256 px, 256 py) is covered when for each edge a -> b of (v1 v2, v2 v0, v0 v1) w = E(a, b, p) > 0, or w == 0 and the edge is a
 * top or a left one: by - ay < 0, or by == ay and bx - ax > 0.  (That is "p + (e, e^2) lies strictly inside" for e -> 0+, so two
 * triangles sharing an edge, or any fan around a vertex, cover each sample exactly once.)  The bounding box is clamped to the image.
 * Depth at a covered sample, perspective-correct (1/z is linear on the screen), fp32 in this order:
 *     r_i = 1 / z_i,  q_i = float(w_i) r_i,  s = (q_0 + q_1) + q_2,  depth = float(area) / s          (w_0 opposite v0, ...)
 * Visibility: key = (bits of depth << 32) | triangle id, combined by an unsigned 64-bit atomic minimum on the KEYS section
 * ([n_views][H][W] uint64 at workspace + keys offset, all ones = background).  The minimum is order independent and a depth tie
 * goes to the lower id: a call is bit-reproducible.  Two work shapes, chosen per triangle by the area of its clamped box: below
 * `wave_box_area` samples one thread walks the box; from there on the triangle goes into a compacted list (the LIST section) and a
 * 64-lane wave deals the box's samples across its lanes.  Both compute the same keys.  wave_box_area <= 0: the library's constant.
 *
 * Stage S, one thread per pixel: the key's triangle again, q_i as above, b_i = q_i / s;
 *     face_id [n][H][W] i32, -1 = background
 *     depth   [n][H][W] f32, the key's depth: view-space z, 0 = background (what TSDFVolume.integrate takes)
 *     normal  [n][H][W][3] f32: c / |c| for c = (p1 - p0) x (p2 - p0) of the ordered vertices, negated unless it faces the eye; the
 *             side is decided exactly: by the sign of the integer area and of det(projmatrix rows 0..2, columns x y w). 0 = background
 *     frames  [n][H][W][3] u8: clamp(rint(255 colour), 0, 255), ties to even (as lara_eval_quantize_frames), with
 *             colour = albedo (ambient + diffuse max(0, n . l)), l = (campos - P) / |campos - P|, P = sum b_i p_i (a head light),
 *             albedo = sum b_i colour_i or the constant; background pixels take the background colour
 *     info    [n][4] u32: triangles drawn (not dropped; they may still cover no sample), dropped behind znear, dropped as degenerate,
 *             dropped as out of range
 * Any output may be NULL.  Every element of a non-NULL output is written.
 *
 * Workspace (lara_meshrender_workspace_bytes; sections 256-byte aligned, in this order): SNAP n_views Nv 16 bytes; KEYS
 * n_views H W 8 bytes; LIST n_views T 4 bytes; COUNT n_views 8 bytes.  lara_meshrender_section_offsets writes the four offsets.
 *
 * T == 0 or Nv == 0: all background, stage R is not launched (stage V runs whenever Nv > 0).  Limits: n_views <= 65535, n_views H W < 2^31, Nv, T < 2^30,
 * znear >= 0.  Returns 0 or a negative LARA2DGS_E_* code; work is enqueued on `stream`, no host synchronisation.
 */
#ifndef LARA_MESHRENDER_H
#define LARA_MESHRENDER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LARA_MESHRENDER_SHADING_FLOATS 8
#define LARA_MESHRENDER_SUBPIXEL 256
#define LARA_MESHRENDER_RANGE (1 << 22)
#define LARA_MESHRENDER_FAR (1 << 30)

int64_t lara_meshrender_workspace_bytes(int32_t n_views, int32_t H, int32_t W, int32_t Nv, int32_t T);

int lara_meshrender_section_offsets(int32_t n_views, int32_t H, int32_t W, int32_t Nv, int32_t T, int64_t *offsets4);

int lara_meshrender_views(int32_t n_views, int32_t H, int32_t W, int32_t Nv, int32_t T, const float *vertices,
                          const int32_t *triangles, const float *vertex_colors, const float *viewmatrix, const float *projmatrix,
                          const float *campos, float znear, const float *shading, int32_t wave_box_area, int32_t *face_id,
                          float *depth, float *normal, uint8_t *frames, uint32_t *info, int32_t *err, void *workspace,
                          void *stream);

#ifdef __cplusplus
}
#endif
#endif
