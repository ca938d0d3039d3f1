/*
 * lara_meshclean.h -- post-processing of an extracted mesh on the device (part of liblara2dgs.so).
 * SURVEY.md section 8f row 4, the step after `volume.extract_triangle_mesh()` in `MeshExtractor.extract`
 * (tools/meshExtractor.py:112-135): crop to the box, connected components of the triangles, keep the largest
 * clusters, drop the unreferenced vertices.  The reference runs these as Open3D calls on the CPU; Open3D is ABSENT from the
 * reference and from this image (its version is not pinned), so the semantics below are [RECALLED] from Open3D's
 * published `TriangleMesh` code and pinned by the numpy restatement tests/meshclean_restate.py, not by Open3D.
 *
 * Meshes: vertices [nv][3] fp32, triangles [T][3] int32 (0 <= index < nv; an index outside raises bit 0 of the caller's
 * `err` word and the triangle reads nothing).  All pointers are device pointers unless marked host; work is enqueued on
 * `stream`.  Every function returns 0 or a negative LARA2DGS_E_* code; a zero-sized call launches nothing.
 *
 *   crop       [RECALLED] meshExtractor.py:116-119 + `RemoveTrianglesByMask`: vertex inside iff lo <= (double)v <= hi on every
 *              axis (both bounds inclusive); a triangle survives iff its three vertices are inside.  The caller compacts the
 *              survivors in order (inclusive prefix sum of `keep` + lara_mesh_compact_rows).
 *   clusters   [RECALLED] `TriangleMesh::ClusterConnectedTriangles`: two triangles are adjacent iff they share an undirected
 *              edge (min(a,b), max(a,b)) of vertex indices (a shared vertex alone does not connect them; all triangles on a
 *              non-manifold edge are mutually adjacent).  Open3D numbers clusters in the order of its BFS over t = 0 .. T-1,
 *              i.e. by their smallest triangle index; `lara_mesh_cluster_labels` gives every triangle the smallest
 *              triangle index of its component, which is unique whatever order the unions land in: the caller's roots
 *              (label[t] == t) in increasing t are clusters 0, 1, ...
 *   stats      cluster_n_triangles [C] int64 (integer atomics) and cluster_area [C] fp64, the sum over the cluster of
 *              0.5 |(v1 - v0) x (v2 - v0)| in double.  The sum is exact in 128-bit fixed point (2^-96 units; two 64-bit
 *              integer atomics with a carry per triangle), then rounded to double once: bitwise reproducible, within
 *              1e-15 relative of any double sum.  Total area per cluster < 2^31.
 *   keep       meshExtractor.py:128-133: with n = sort(counts)[-min(C, keep)] (the caller's `threshold`), triangles of
 *              clusters with fewer than n triangles are dropped -- ties at the threshold stay, so more than `keep` clusters
 *              can survive.  The referenced vertices are flagged for `RemoveUnreferencedVertices` ([RECALLED]: the kept
 *              vertices keep their order, the triangles are remapped).
 *
 * Deterministic: every output is a function of the input alone (no float atomics; labels are minima).  Bounded: every
 * hash probe stops at the table's capacity, every root walk at 64 steps, the union rounds at 2 ceil(log2 T) + 8; a bound
 * that is reached is reported as LARA2DGS_E_LAUNCH, never spun on.  Cross-workgroup reads inside a launch go through
 * agent-scope atomics; everything else is read across a kernel boundary.
 */
#ifndef LARA_MESHCLEAN_H
#define LARA_MESHCLEAN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* keep [T] int32 = 1 iff the triangle's three vertices lie in box = (lo x, lo y, lo z, hi x, hi y, hi z) (host, double). */
int lara_mesh_crop(int64_t nv, int64_t T, const float *vertices, const int32_t *triangles, const double *box /* host [6] */,
                   int32_t *keep, int32_t *err, void *stream);

/* Order-preserving compaction of n rows of `width` 32-bit words: keep[i] != 0 -> dst row ends[i] - 1 = src row i, where
 * ends is the inclusive prefix sum of (keep != 0) as int64 (the caller's scan). */
int lara_mesh_compact_rows(int64_t n, int32_t width, const void *src, const int32_t *keep, const int64_t *ends, void *dst,
                           void *stream);

/* label [T] int32 = the smallest triangle index of the triangle's edge-connected component.  Scratch: keys [capacity]
 * (64-bit), owner [capacity] int32, adj [3 T] int32, work [2] int32; capacity a power of two >= 6 T (the edge table is
 * at least twice the number of edges).  Host reads: ONE per union round (a changed word and an error word, 8 bytes; a
 * connected mesh takes a few rounds), after a stream synchronisation -- `rounds` (host, may be null) receives their
 * number. */
int lara_mesh_cluster_labels(int64_t T, const int32_t *triangles, int64_t capacity, uint64_t *keys, int32_t *owner,
                             int32_t *adj, int32_t *label, int32_t *work, int32_t *rounds /* host */, void *stream);

/* clusters [T] int32 = root_ends[label[t]] - 1 (root_ends: inclusive prefix sum of label[t] == t, int64), counts [C] int64
 * and area [C] fp64.  counts and area_acc [2 C] (64-bit scratch) are zero-filled by the caller. */
int lara_mesh_cluster_stats(int64_t nv, int64_t T, const float *vertices, const int32_t *triangles, const int32_t *label,
                            const int64_t *root_ends, int64_t C, int32_t *clusters, int64_t *counts, uint64_t *area_acc,
                            double *area, int32_t *err, void *stream);

/* keep [T] int32 = counts[clusters[t]] >= *threshold (device int64 [1]); referenced [nv] int32 (caller zero-fills) = 1
 * for every vertex of a kept triangle. */
int lara_mesh_keep_clusters(int64_t nv, int64_t T, const int32_t *triangles, const int32_t *clusters, const int64_t *counts,
                            const int64_t *threshold, int32_t *keep, int32_t *referenced, int32_t *err, void *stream);

/* out [T][3] int32 = vertex_ends[triangles] - 1 (vertex_ends: inclusive prefix sum of `referenced`, int64). */
int lara_mesh_remap(int64_t nv, int64_t T, const int32_t *triangles, const int64_t *vertex_ends, int32_t *out, int32_t *err,
                    void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LARA_MESHCLEAN_H */
