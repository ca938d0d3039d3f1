/*
 * meshtopo/lara_meshtopo.h -- the connectivity of a triangle mesh on the device: the unique undirected edges with their incident
 * faces, the report that says whether the surface is closed and consistently oriented, the vertex->vertex and vertex->face adjacency
 * in a fixed order, and the two per-vertex functions that walk them: vertex normals and the Laplacian smoothing step (part of
 * liblara2dgs.so; opt-in, python side: lara_amd/meshtopo.py; kernels: csrc/meshtopo.hip; the two per-vertex functions, for the device
 * and the host: csrc/meshtopo_ops.h).  All pointers are device pointers unless a function's name ends in _host.  Returns 0 or a
 * negative LARA2DGS_E_* code.  Work is enqueued on `stream`; no entry point reads anything back to the host; a zero-sized call
 * launches nothing.  Sorting is the caller's (a library sort between two calls, as for meshbvh/lara_meshbvh.h).  Built with
 * -ffp-contract=off: the sequences written here are the instructions.  Open3D's filter_smooth_laplacian / filter_smooth_taubin and
 * compute_vertex_normals are [RECALLED]; Open3D is absent, and tests/meshtopo_restate.py pins what is written here.
 *
 * ---- definitions -------------------------------------------------------------------------------------------------------------------------
 * vertices [Nv][3] f32, triangles [T][3] i32, Nv < 2^31, 3 T < 2^31.
 * An index outside [0, Nv) raises bit 0 of the caller's `err` word (lara_meshtopo_halfedge_keys); the triangle is then ignored.
 * A triangle is VALID when its three indices are in range and pairwise distinct.  In range with a repeated index it is DEGENERATE:
 * counted and skipped, not an error.  A triangle without area whose indices are distinct is valid.
 * Half-edge h = 3 t + k runs from tri[t][k] to tri[t][(k + 1) % 3].
 * LARA_MESHTOPO_SENTINEL (the largest int64) is the key of what is skipped; it sorts behind every key.
 *
 * ---- the edge table ----------------------------------------------------------------------------------------------------------------------
 * lara_meshtopo_halfedge_keys: keys [3T] i64, keys[h] = (min(a, b) << 32) | max(a, b) of half-edge h of a valid triangle, else the
 *     sentinel.  The caller sorts (keys, h) by key, STABLY: the half-edges of an edge then stand in ascending h, so in ascending
 *     triangle id (a valid triangle has at most one half-edge on an edge).
 * lara_meshtopo_edge_heads: sorted keys [n] -> heads [n] i32, 1 where a key is not the sentinel and differs from the one before it.
 *     The caller's inclusive prefix sum `ends` [n] i64 gives the edge id ends[i] - 1 of position i, and E = ends[n - 1].
 * lara_meshtopo_edge_rows: sorted keys [n], order [n] i64 (the half-edge at each sorted position), heads, ends, triangles -> for
 *     every unique edge e, in ascending (lo, hi):
 *         edges [E][2] i32       (lo, hi)
 *         edge_n [E] i32         the incident valid triangles
 *         edge_fwd [E] i32       the incident half-edges directed lo -> hi
 *         edge_face [E][2] i32   the two smallest incident triangle ids, -1 where absent
 *     and tri_edge [T][3] i32, the edge id of every half-edge, -1 for a triangle that is not valid.  n = 3 T.  The call sets all five
 *     itself (memsets on `stream`, then one kernel, one thread per sorted position).  edge_n and edge_fwd are integer atomic
 *     counts, whose result does not depend on their order; a run may have any length and span workgroups.  Everything else is
 *     written by the one thread that owns it.
 *
 * ---- lara_meshtopo_report ----------------------------------------------------------------------------------------------------------------
 * -> out [LARA_MESHTOPO_REPORT] i64, set by the call itself; work [2 Nv] i32 is scratch the call clears.
 *     out[0] n_vertices = Nv            out[1] n_referenced: vertices of a valid triangle      out[2] n_triangles = T
 *     out[3] n_valid                    out[4] n_degenerate                                    out[5] n_edges = E
 *     out[6] n_boundary: edge_n == 1    out[7] n_manifold: edge_n == 2                         out[8] n_nonmanifold: edge_n >= 3
 *     out[9] n_inconsistent: edge_n == 2 and edge_fwd != 1
 *     out[10] n_boundary_vertices: vertices of an edge with edge_n == 1
 *     out[11] max_degree: the largest number of unique neighbours (= incident edges) of a vertex
 * Integer sums (a wave's butterfly, one 64-bit integer atomic per wave and count), integer or-flags and an integer maximum: exact,
 * whatever the order.
 * lara_meshtopo_boundary_vertices: flag [Nv] i32 = 1 for a vertex of an edge with edge_n == 1, else 0 (set by the call).
 *
 * ---- adjacency: two CSR tables ---------------------------------------------------------------------------------------------------------
 * lara_meshtopo_pair_keys: edges [E][2] -> keys [2E] i64: (lo << 32) | hi and (hi << 32) | lo of every edge.  All different.
 * lara_meshtopo_corner_keys: keys [3T] i64, keys[h] = (tri[t][k] << 32) | h for a valid triangle, else the sentinel.  All different.
 * lara_meshtopo_csr: n sorted keys WITHOUT sentinels (the caller passes the sorted array's front) -> offsets [Nv + 1] i64, the number
 *     of keys below v << 32 (a binary search per vertex), and values:
 *         mode LARA_MESHTOPO_CSR_NEIGHBORS (0): values [n] i32 = the key's low word: the unique neighbours of each vertex in ascending
 *             vertex id, n = 2 E
 *         mode LARA_MESHTOPO_CSR_FACES (1): values [n][2] i32 = (low word / 3, low word % 3): the valid triangles around each vertex in
 *             ascending triangle id, each with the corner the vertex is, n = 3 n_valid
 *
 * ---- the per-vertex functions (csrc/meshtopo_ops.h, the single definition of both answers) ----------------------------------------------
 * All arithmetic is double on the fp32 inputs; one rounding to fp32 at the end.
 * lara_meshtopo_normal, vertex v, over its row of the face table in the stored order:
 *     u = p1 - p0, w = p2 - p0 with p0, p1, p2 = the triangle's corners in the triangle's own order (whichever corner v is);
 *     c = (u_y w_z - u_z w_y, u_z w_x - u_x w_z, u_x w_y - u_y w_x)
 *     weighting LARA_MESHTOPO_WEIGHT_AREA (0): the term is c.  LARA_MESHTOPO_WEIGHT_UNIFORM (1): l = sqrt((c_x c_x + c_y c_y) + c_z c_z),
 *         a face with l == 0 is skipped, the term is (c_x / l, c_y / l, c_z / l)
 *     s += term, component by component;  L = sqrt((s_x s_x + s_y s_y) + s_z s_z)
 *     L > 0 and L < inf: normal = fl32(s / L).  Otherwise (zero, inf or NaN; a vertex without a face): (0, 0, 0), and counted.
 * lara_meshtopo_smooth, vertex v with position x, over its row of the neighbour table in the stored order:
 *     m += (double)src[neighbour], component by component;  m = m / (double)degree;  x' = fl32(x + s (m - x))
 *     A vertex of degree 0, and a vertex with fixed[v] != 0, keeps its bits.  NaN and inf propagate and are not checked.
 *
 * lara_meshtopo_vertex_normals: one kernel, one thread per vertex -> normals [Nv][3] f32, zero_count [1] i64 (set by the call).
 * lara_meshtopo_smooth_pass: one kernel, one thread per vertex: a Jacobi step that reads src [Nv][3] and writes dst [Nv][3], which must
 *     not overlap.  s is the step (lambda, or Taubin's negative mu).  fixed [Nv] i32 or NULL.
 * A row is walked by its one thread from its first entry to its last: the order of the double sum is the contract.
 * lara_meshtopo_normals_host, lara_meshtopo_smooth_host: the same functions over the same arrays in HOST memory; no device is touched.
 */
#ifndef LARA_MESHTOPO_H
#define LARA_MESHTOPO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LARA_MESHTOPO_SENTINEL 0x7fffffffffffffffll
#define LARA_MESHTOPO_REPORT 12
#define LARA_MESHTOPO_CSR_NEIGHBORS 0
#define LARA_MESHTOPO_CSR_FACES 1
#define LARA_MESHTOPO_WEIGHT_AREA 0
#define LARA_MESHTOPO_WEIGHT_UNIFORM 1

int lara_meshtopo_halfedge_keys(int32_t Nv, int32_t T, const int32_t *triangles, int64_t *keys, int32_t *err, void *stream);

int lara_meshtopo_edge_heads(int64_t n, const int64_t *keys, int32_t *heads, void *stream);

int lara_meshtopo_edge_rows(int64_t n, int64_t E, const int64_t *keys, const int64_t *order, const int32_t *heads, const int64_t *ends,
                            const int32_t *triangles, int32_t *edges, int32_t *edge_n, int32_t *edge_fwd, int32_t *edge_face,
                            int32_t *tri_edge, void *stream);

int lara_meshtopo_report(int32_t Nv, int32_t T, int64_t E, const int32_t *triangles, const int32_t *edges, const int32_t *edge_n,
                         const int32_t *edge_fwd, int32_t *work, int64_t *out, void *stream);

int lara_meshtopo_boundary_vertices(int32_t Nv, int64_t E, const int32_t *edges, const int32_t *edge_n, int32_t *flag, void *stream);

int lara_meshtopo_pair_keys(int64_t E, const int32_t *edges, int64_t *keys, void *stream);

int lara_meshtopo_corner_keys(int32_t Nv, int32_t T, const int32_t *triangles, int64_t *keys, void *stream);

int lara_meshtopo_csr(int32_t Nv, int64_t n, const int64_t *keys, int32_t mode, int64_t *offsets, int32_t *values, void *stream);

int lara_meshtopo_vertex_normals(int32_t Nv, const float *vertices, const int32_t *triangles, const int64_t *offsets,
                                 const int32_t *faces, int32_t weighting, float *normals, int64_t *zero_count, void *stream);

int lara_meshtopo_smooth_pass(int32_t Nv, const float *src, float *dst, const int64_t *offsets, const int32_t *neighbors, double s,
                              const int32_t *fixed, void *stream);

int lara_meshtopo_normals_host(int32_t Nv, const float *vertices, const int32_t *triangles, const int64_t *offsets,
                               const int32_t *faces, int32_t weighting, float *normals, int64_t *zero_count);

int lara_meshtopo_smooth_host(int32_t Nv, const float *src, float *dst, const int64_t *offsets, const int32_t *neighbors, double s,
                              const int32_t *fixed);

#ifdef __cplusplus
}
#endif
#endif
