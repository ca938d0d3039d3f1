/*
 * meshsimplify/lara_meshsimplify.h -- vertex-clustering simplification of a triangle mesh on the device, with quadric or mean
 * placement of the cluster vertices (part of liblara2dgs.so; opt-in, python side: lara_amd/meshsimplify.py; kernels:
 * csrc/meshsimplify.hip).  All pointers are device pointers.  Returns 0 or a negative LARA2DGS_E_* code.  Work is enqueued on
 * `stream`; no entry point waits for it or reads anything back.  Bad input is reported through the int32 error word `err`
 * (bits below, OR-ed by the kernels; the caller zeroes it and reads it with the sizes), never by a fault.  Built with
 * -ffp-contract=off: the sequences written here are the instructions.
 *
 * The caller (lara_amd/meshsimplify.py) owns the prefix sums between the stages (inclusive, int64, as lara_meshclean.h's
 * `ends` arrays) and the host reads of the sizes.
 *
 * ---- cells -------------------------------------------------------------------------------------------------------------------
 * vertices [Nv][3] f32, h > 0 f32, origin [3] f32 (device).  cell_a = floorf((v_a - origin_a) / h): an fp32 subtract, an fp32
 * divide.  A non-finite coordinate raises ERR_NONFINITE, a negative cell ERR_NEGATIVE, a cell >= 2^21 ERR_EXTENT; such a
 * vertex gets slot -1.  Every other vertex is inserted under the key (cx << 42 | cy << 21 | cz) into an open-addressing table
 * (compare-and-swap on the key, atomic min of the vertex index on the slot's leader word): slot [Nv] receives its slot,
 * is_leader [Nv] = 1 for the smallest vertex of each occupied cell (else 0).  A probe sequence that runs through the whole
 * table raises ERR_PROBE.  Workspace (lara_meshsimplify_cells_workspace_bytes(Nv)): the table; it is read again by
 * lara_meshsimplify_clusters.
 *
 * ---- clusters ----------------------------------------------------------------------------------------------------------------
 * leader_ends [Nv] i64 = the inclusive prefix sum of is_leader: clusters are numbered by ascending smallest member.
 * vertex_cluster [Nv] i32 = the cluster of every vertex, leader_vertex [n_cells] i32 = the smallest member of every cluster.
 *
 * ---- triangles ---------------------------------------------------------------------------------------------------------------
 * triangles [T][3] i32 -> mapped [T][3] i32: the corners' clusters, rotated so that the smallest comes first (-1 -1 -1 and
 * ERR_INDEX for an index outside [0, Nv) or a cluster outside [0, n_cells)).  keep [T] i32 = 1 for a triangle whose three clusters differ and that is the
 * smallest triangle with its oriented triple (a table of triangle indices: compare-and-swap of the slot's representative,
 * equality of the mapped triples, atomic min of the owner), else 0.  referenced [n_cells] i32 (zeroed by the caller) = 1 for
 * every cluster a kept triangle uses.  counters[LARA_MESHSIMPLIFY_N_DEGENERATE] and [.._N_DUPLICATE] are incremented.
 * Workspace (lara_meshsimplify_triangles_workspace_bytes(T)): the table and one slot word per triangle.
 *
 * ---- corner keys -------------------------------------------------------------------------------------------------------------
 * c = (p1 - p0) x (p2 - p0) in double from the fp32 vertices.  corner_key [3T] i32 = the cluster of every corner of a triangle
 * with finite non-zero |c|^2, -1 for the corners of every other triangle (counted in counters[.._N_ZERO_AREA]).
 *
 * ---- buckets -----------------------------------------------------------------------------------------------------------------
 * lara_meshsimplify_bucket_count: count [n_keys] i32 = the number of items i in [0, n) with key[i] == k (a negative key is in no
 * bucket).  lara_meshsimplify_bucket_fill, with ends [n_keys] i64 = the inclusive prefix sum of count: items [ends[n_keys-1]]
 * i32 = the items of bucket k at [ends[k-1], ends[k]) in ASCENDING order (an atomic-cursor scatter, then every item counts the
 * smaller items of its bucket: the order of the scatter does not reach the output).
 * Workspace (lara_meshsimplify_bucket_workspace_bytes(n, n_keys)): the cursors and the unordered copy.
 *
 * ---- sums --------------------------------------------------------------------------------------------------------------------
 * One 64-lane wave per cluster g, double sums in a fixed order: lane l adds the items l, l + 64, ... of the bucket (ascending
 * vertex; ascending 3 t + corner) serially, the 64 partials are added by the xor butterfly (distance 32, 16, ..., 1):
 *   mean [n_cells][3] f64 = (sum of the members' positions) / count;  color_out [n_cells][3] f32 likewise from colors (may both
 *   be NULL);  with quadric != 0, for every corner in g's bucket, n = c / |c|, w = |c| / 2, d = n . (p0 - mean_g):
 *   Ab [n_cells][9] f64 = {Axx, Axy, Axz, Ayy, Ayz, Azz, bx, by, bz},  A += w n n^T,  b += (w d) n.
 *
 * ---- solve -------------------------------------------------------------------------------------------------------------------
 * out [n_cells][3] f32.  quadric == 0, or trace(A) == 0: out = float(mean).  Otherwise mu = 2^-10 trace(A), (A + mu I) y = b by
 * Cholesky in double, x = mean + y clamped per coordinate to [origin_a + i_a h, origin_a + (i_a + 1) h] (double; i = the cell
 * of leader_vertex[g], recomputed as above); counters[.._N_CLAMPED] counts the clusters with referenced[g] != 0 that a clamp moved.
 *
 * ---- vertex map --------------------------------------------------------------------------------------------------------------
 * out [Nv] i32 = referenced[g] ? cluster_ends[g] - 1 : -1 for g = vertex_cluster[v] (cluster_ends = prefix sum of referenced).
 *
 * Limits: Nv < 2^31, 3 T < 2^31.  Counts of zero are no-ops.
 */
#ifndef LARA_MESHSIMPLIFY_H
#define LARA_MESHSIMPLIFY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LARA_MESHSIMPLIFY_ERR_INDEX 1
#define LARA_MESHSIMPLIFY_ERR_PROBE 2
#define LARA_MESHSIMPLIFY_ERR_NONFINITE 4
#define LARA_MESHSIMPLIFY_ERR_NEGATIVE 8
#define LARA_MESHSIMPLIFY_ERR_EXTENT 16
#define LARA_MESHSIMPLIFY_MAX_CELL (1 << 21)

#define LARA_MESHSIMPLIFY_N_DEGENERATE 0
#define LARA_MESHSIMPLIFY_N_DUPLICATE 1
#define LARA_MESHSIMPLIFY_N_ZERO_AREA 2
#define LARA_MESHSIMPLIFY_N_CLAMPED 3
#define LARA_MESHSIMPLIFY_COUNTERS 4

int64_t lara_meshsimplify_cells_workspace_bytes(int64_t Nv);

int lara_meshsimplify_cells(int64_t Nv, const float *vertices, float h, const float *origin, int32_t *slot, int32_t *is_leader,
                            void *workspace, int32_t *err, void *stream);

int lara_meshsimplify_clusters(int64_t Nv, const int32_t *slot, const int64_t *leader_ends, const void *workspace,
                               int32_t *vertex_cluster, int32_t *leader_vertex, void *stream);

int64_t lara_meshsimplify_triangles_workspace_bytes(int64_t T);

int lara_meshsimplify_triangles(int64_t Nv, int64_t T, int64_t n_cells, const int32_t *triangles, const int32_t *vertex_cluster,
                                int32_t *mapped, int32_t *keep, int32_t *referenced, int32_t *counters, void *workspace, int32_t *err, void *stream);

int lara_meshsimplify_corner_keys(int64_t Nv, int64_t T, const float *vertices, const int32_t *triangles,
                                  const int32_t *vertex_cluster, int32_t *corner_key, int32_t *counters, void *stream);

int lara_meshsimplify_bucket_count(int64_t n, int64_t n_keys, const int32_t *key, int32_t *count, void *stream);

int64_t lara_meshsimplify_bucket_workspace_bytes(int64_t n, int64_t n_keys);

int lara_meshsimplify_bucket_fill(int64_t n, int64_t n_keys, const int32_t *key, const int64_t *ends, int32_t *items,
                                  void *workspace, void *stream);

int lara_meshsimplify_sums(int64_t Nv, int64_t T, int64_t n_cells, const float *vertices, const float *colors,
                           const int32_t *triangles, const int64_t *vertex_ends, const int32_t *vertex_items,
                           const int64_t *corner_ends, const int32_t *corner_items, int32_t quadric, double *mean, float *color_out,
                           double *Ab, void *stream);

int lara_meshsimplify_solve(int64_t Nv, int64_t n_cells, int32_t quadric, const double *mean, const double *Ab, const float *vertices,
                            const int32_t *leader_vertex, float h, const float *origin, const int32_t *referenced, float *out,
                            int32_t *counters, void *stream);

int lara_meshsimplify_vertex_map(int64_t Nv, int64_t n_cells, const int32_t *vertex_cluster, const int32_t *referenced,
                                 const int64_t *cluster_ends, int32_t *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
