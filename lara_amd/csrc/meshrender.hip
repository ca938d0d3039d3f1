// meshrender.hip -- z-buffer triangle rasteriser for the extracted mesh's turntable on gfx950: ~0.5 M marching-cubes triangles of
// one to four pixels each per 512 x 512 view.  Interface, layouts, the fill rule and every formula in
// include/lara_meshrender.h.
//
//   mr_fill_kernel     keys <- all ones, info / list counters <- 0
//   mr_snap_kernel     stage V: one thread per (view, vertex) -> {snapped x, y, view z}
//   mr_raster_kernel   stage R, small boxes: one thread per (view, triangle) classifies the triangle, counts a DROPPED one (one atomic
//                      per wave and class; the drawn ones are what is left of T, written by the resolve kernel), walks its clamped box, or appends it to the view's list when the box holds >= wave_box_area samples
//   mr_raster_wave_kernel  stage R, listed triangles: a wave per triangle, the box's samples dealt across the 64 lanes
//   mr_resolve_kernel  stage S: one thread per pixel unpacks the key, recomputes the winner's barycentrics, writes the outputs
// Views in grid z.  Coverage is int64 arithmetic, visibility one 64-bit unsigned atomicMin per covered sample (a vector global
// atomic; order independent): two runs give the same bits.  Built with -ffp-contract=off: the fp32 sequences of the header are the
// instructions.
#include "common.h"
#include "wave.h"
#include "../../include/lara_meshrender.h"

namespace {

// A thread walks boxes below this many samples itself; from here on the triangle goes to a wave.  Chosen from the lane count: at
// 64 samples every lane of the wave gets at least one sample of its triangle, below it part of the wave would idle through the
// setup while a lone thread's walk stays shorter than one wave's setup-plus-trip.  Marching-cubes triangles at 512 x 512 have
// boxes of 1 to 9 samples, so the list stays (nearly) empty there; tools/meshrender_bench.py reports both stages' times.
constexpr int MR_WAVE_BOX_AREA = 64;
constexpr unsigned long long MR_EMPTY = ~0ull;

struct MrArgs {
    int n, H, W, Nv, T;
    const float *vertices;
    const int *triangles;
    const float *colors, *view, *proj, *campos;
    float znear;
    int wave_box_area;
    float albedo[3], background[3], ambient, diffuse;
    int4 *snap;
    unsigned long long *keys;
    int *list;
    unsigned *count;       // [n] list lengths, then [n] triangles with an index out of range
    int mesh;              // stage R ran
    int *face_id;
    float *depth, *normal;
    uint8_t *frames;
    unsigned *info;
    int *err;
};

enum { MR_DRAWN = 0, MR_BEHIND = 1, MR_DEGENERATE = 2, MR_RANGE = 3, MR_BAD_INDEX = 4, MR_NONE = 5 };

struct MrTri {
    int idx[3];            // vertex indices, ordered so that area > 0
    int x[3], y[3];
    float r[3];            // 1 / z
    long long area;
    bool own[3];           // edge i (opposite vertex i) is a top or a left edge
    int bx0, bx1, by0, by1;   // clamped box, inclusive; empty when bx1 < bx0 or by1 < by0
};

__device__ __forceinline__ int mr_snap(const float v) {
    if (!(fabsf(v) < (float)LARA_MESHRENDER_FAR)) return LARA_MESHRENDER_FAR;
    return (int)__builtin_rintf(v);
}

__device__ __forceinline__ long long mr_edge(const int ax, const int ay, const int bx, const int by, const long long px, const long long py) {
    return (long long)(bx - ax) * (py - ay) - (long long)(by - ay) * (px - ax);
}
__device__ __forceinline__ bool mr_owns(const int ax, const int ay, const int bx, const int by) {
    return by - ay < 0 || (by == ay && bx - ax > 0);
}

// the triangle's class; for MR_DRAWN `tr` is complete
__device__ __forceinline__ int mr_setup(const MrArgs &p, const int view, const int t, MrTri &tr) {
    int i0 = p.triangles[3 * (size_t)t], i1 = p.triangles[3 * (size_t)t + 1], i2 = p.triangles[3 * (size_t)t + 2];
    if ((unsigned)i0 >= (unsigned)p.Nv || (unsigned)i1 >= (unsigned)p.Nv || (unsigned)i2 >= (unsigned)p.Nv) return MR_BAD_INDEX;
    const int4 *snap = p.snap + (size_t)view * p.Nv;
    const int4 a = snap[i0];
    int4 b = snap[i1], c = snap[i2];
    const float za = __int_as_float(a.z), zb = __int_as_float(b.z), zc = __int_as_float(c.z);
    if (!(za > p.znear) || !(zb > p.znear) || !(zc > p.znear)) return MR_BEHIND;
    const int R = LARA_MESHRENDER_RANGE;
    if (abs(a.x) > R || abs(a.y) > R || abs(b.x) > R || abs(b.y) > R || abs(c.x) > R || abs(c.y) > R) return MR_RANGE;
    long long area = mr_edge(a.x, a.y, b.x, b.y, c.x, c.y);
    if (area == 0) return MR_DEGENERATE;
    if (area < 0) {
        const int4 sw = b; b = c; c = sw;
        const int si = i1; i1 = i2; i2 = si;
        area = -area;
    }
    tr.idx[0] = i0; tr.idx[1] = i1; tr.idx[2] = i2;
    tr.x[0] = a.x; tr.x[1] = b.x; tr.x[2] = c.x;
    tr.y[0] = a.y; tr.y[1] = b.y; tr.y[2] = c.y;
    tr.r[0] = 1.0f / __int_as_float(a.z); tr.r[1] = 1.0f / __int_as_float(b.z); tr.r[2] = 1.0f / __int_as_float(c.z);
    tr.area = area;
    tr.own[0] = mr_owns(b.x, b.y, c.x, c.y);
    tr.own[1] = mr_owns(c.x, c.y, a.x, a.y);
    tr.own[2] = mr_owns(a.x, a.y, b.x, b.y);
    const int xmin = min(a.x, min(b.x, c.x)), xmax = max(a.x, max(b.x, c.x));
    const int ymin = min(a.y, min(b.y, c.y)), ymax = max(a.y, max(b.y, c.y));
    // ceil and floor of snapped / 256 by arithmetic shifts (|snapped| <= 2^22)
    tr.bx0 = max((xmin + LARA_MESHRENDER_SUBPIXEL - 1) >> 8, 0);
    tr.bx1 = min(xmax >> 8, p.W - 1);
    tr.by0 = max((ymin + LARA_MESHRENDER_SUBPIXEL - 1) >> 8, 0);
    tr.by1 = min(ymax >> 8, p.H - 1);
    return MR_DRAWN;
}

// the three edge functions at sample (px, py); covered?
__device__ __forceinline__ bool mr_cover(const MrTri &tr, const int px, const int py, long long w[3]) {
    const long long X = (long long)px * LARA_MESHRENDER_SUBPIXEL, Y = (long long)py * LARA_MESHRENDER_SUBPIXEL;
    w[0] = mr_edge(tr.x[1], tr.y[1], tr.x[2], tr.y[2], X, Y);
    w[1] = mr_edge(tr.x[2], tr.y[2], tr.x[0], tr.y[0], X, Y);
    w[2] = mr_edge(tr.x[0], tr.y[0], tr.x[1], tr.y[1], X, Y);
    return (w[0] > 0 || (w[0] == 0 && tr.own[0])) && (w[1] > 0 || (w[1] == 0 && tr.own[1])) && (w[2] > 0 || (w[2] == 0 && tr.own[2]));
}

// q_i = float(w_i) r_i, s = (q0 + q1) + q2, depth = float(area) / s
__device__ __forceinline__ float mr_depth(const MrTri &tr, const long long w[3], float q[3], float &s) {
    q[0] = (float)w[0] * tr.r[0];
    q[1] = (float)w[1] * tr.r[1];
    q[2] = (float)w[2] * tr.r[2];
    s = (q[0] + q[1]) + q[2];
    return (float)tr.area / s;
}

__device__ __forceinline__ void mr_sample(const MrArgs &p, const MrTri &tr, const int view, const int t, const int px, const int py) {
    long long w[3];
    if (!mr_cover(tr, px, py, w)) return;
    float q[3], s;
    const float d = mr_depth(tr, w, q, s);
    const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)t;
    atomicMin(p.keys + ((size_t)view * p.H + py) * p.W + px, key);
}

__global__ void __launch_bounds__(256)
mr_fill_kernel(const MrArgs p) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, pixels = (size_t)p.n * p.H * p.W;
    if (i < pixels) p.keys[i] = MR_EMPTY;
    if (i < (size_t)p.n * 4 && p.info) p.info[i] = 0u;
    if (i < (size_t)p.n * 2) p.count[i] = 0u;
}

__global__ void __launch_bounds__(256)
mr_snap_kernel(const MrArgs p) {
    const int i = blockIdx.x * 256 + threadIdx.x, view = blockIdx.z;
    if (i >= p.Nv) return;
    const float *m = p.proj + 16 * view, *vm = p.view + 16 * view;
    const float x = p.vertices[3 * (size_t)i], y = p.vertices[3 * (size_t)i + 1], z = p.vertices[3 * (size_t)i + 2];
    const float hx = ((m[0] * x + m[4] * y) + m[8] * z) + m[12];
    const float hy = ((m[1] * x + m[5] * y) + m[9] * z) + m[13];
    const float hw = ((m[3] * x + m[7] * y) + m[11] * z) + m[15];
    const float vz = ((vm[2] * x + vm[6] * y) + vm[10] * z) + vm[14];
    const float px = (((hx / hw) + 1.0f) * (float)p.W - 1.0f) * 0.5f;
    const float py = (((hy / hw) + 1.0f) * (float)p.H - 1.0f) * 0.5f;
    p.snap[(size_t)view * p.Nv + i] = make_int4(mr_snap(px * (float)LARA_MESHRENDER_SUBPIXEL), mr_snap(py * (float)LARA_MESHRENDER_SUBPIXEL),
                                                __float_as_int(vz), 0);
}

__global__ void __launch_bounds__(256)
mr_raster_kernel(const MrArgs p) {
    const int t = blockIdx.x * 256 + threadIdx.x, view = blockIdx.z;
    MrTri tr;
    const int cls = t < p.T ? mr_setup(p, view, t, tr) : MR_NONE;
    // (every lane of the wave is here: one atomic per wave and class)
    const int lane = threadIdx.x & 63;
    // the dropped classes are rare; the drawn triangles -- nearly all -- are counted by subtraction in mr_resolve_kernel: an atomic
    // per wave on one word per view was a same-address chain of 9 k atomics per view, 7 of the 11 ms of a 120-frame turntable
#pragma unroll
    for (int c = MR_BEHIND; c <= MR_BAD_INDEX; c++) {
        const unsigned long long m = __ballot(cls == c);
        if (lane == 0 && m) {
            if (c == MR_BAD_INDEX) atomicAdd(p.count + p.n + view, (unsigned)__popcll(m));
            else if (p.info) atomicAdd(p.info + 4 * view + c, (unsigned)__popcll(m));
        }
    }
    if (cls == MR_BAD_INDEX && p.err) atomicOr(p.err, 1);
    if (cls != MR_DRAWN || tr.bx1 < tr.bx0 || tr.by1 < tr.by0) return;
    const int bw = tr.bx1 - tr.bx0 + 1, bh = tr.by1 - tr.by0 + 1;
    if ((long long)bw * bh >= p.wave_box_area) {
        const unsigned slot = atomicAdd(p.count + view, 1u);
        p.list[(size_t)view * p.T + slot] = t;          // (slot < T: every triangle is appended at most once)
        return;
    }
    for (int py = tr.by0; py <= tr.by1; py++)
        for (int px = tr.bx0; px <= tr.bx1; px++) mr_sample(p, tr, view, t, px, py);
}

__global__ void __launch_bounds__(256)
mr_raster_wave_kernel(const MrArgs p) {
    const int view = blockIdx.z, lane = threadIdx.x & 63;
    const unsigned waves = gridDim.x * 4u, n = min(p.count[view], (unsigned)p.T);
    for (unsigned i = blockIdx.x * 4u + (threadIdx.x >> 6); i < n; i += waves) {
        const int t = p.list[(size_t)view * p.T + i];
        MrTri tr;
        if ((unsigned)t >= (unsigned)p.T || mr_setup(p, view, t, tr) != MR_DRAWN) continue;      // (cannot happen: the list holds drawn triangles)
        const int bw = tr.bx1 - tr.bx0 + 1, bh = tr.by1 - tr.by0 + 1, samples = bw * bh;          // <= H W < 2^31
        for (int k = lane; k < samples; k += 64) {
            const int row = k / bw;
            mr_sample(p, tr, view, t, tr.bx0 + (k - row * bw), tr.by0 + row);
        }
    }
}

__device__ __forceinline__ uint8_t mr_u8(const float colour) {      // rint: ties to even, as np.round (evalscores.hip: ev_colour)
    return (uint8_t)fminf(fmaxf(__builtin_rintf(colour * 255.0f), 0.0f), 255.0f);
}

__global__ void __launch_bounds__(256)
mr_resolve_kernel(const MrArgs p) {
    const int pix = blockIdx.x * 256 + threadIdx.x, view = blockIdx.z, HW = p.H * p.W;
    if (pix == 0 && p.info && p.mesh)       // (stage R's launches are complete: the stream orders this kernel behind them)
        p.info[4 * view] = (unsigned)p.T - p.info[4 * view + 1] - p.info[4 * view + 2] - p.info[4 * view + 3] - p.count[p.n + view];
    if (pix >= HW) return;
    const size_t o = (size_t)view * HW + pix;
    const unsigned long long key = p.keys[o];
    if (key == MR_EMPTY) {
        if (p.face_id) p.face_id[o] = -1;
        if (p.depth) p.depth[o] = 0.0f;
        if (p.normal) { p.normal[3 * o] = 0.0f; p.normal[3 * o + 1] = 0.0f; p.normal[3 * o + 2] = 0.0f; }
        if (p.frames) { p.frames[3 * o] = mr_u8(p.background[0]); p.frames[3 * o + 1] = mr_u8(p.background[1]); p.frames[3 * o + 2] = mr_u8(p.background[2]); }
        return;
    }
    const int t = (int)(unsigned)(key & 0xffffffffu);
    if (p.face_id) p.face_id[o] = t;
    if (p.depth) p.depth[o] = __uint_as_float((unsigned)(key >> 32));
    if (!p.normal && !p.frames) return;
    MrTri tr;
    if (mr_setup(p, view, t, tr) != MR_DRAWN) return;                // (cannot happen: the key came from a drawn triangle)
    const float *v0 = p.vertices + 3 * (size_t)tr.idx[0], *v1 = p.vertices + 3 * (size_t)tr.idx[1], *v2 = p.vertices + 3 * (size_t)tr.idx[2];
    const float p0[3] = {v0[0], v0[1], v0[2]}, p1[3] = {v1[0], v1[1], v1[2]}, p2[3] = {v2[0], v2[1], v2[2]};
    const float ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
    const float bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
    float cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
    const float len = sqrtf((cx * cx + cy * cy) + cz * cz);
    // the ordered triangle has positive area on the screen: its normal faces the eye iff the projection reverses orientation
    const float *m = p.proj + 16 * view;
    const float det = (m[0] * (m[5] * m[11] - m[7] * m[9]) - m[1] * (m[4] * m[11] - m[7] * m[8])) + m[3] * (m[4] * m[9] - m[5] * m[8]);
    const float sgn = det < 0.0f ? 1.0f : -1.0f;
    const float nx = sgn * (cx / len), ny = sgn * (cy / len), nz = sgn * (cz / len);
    if (p.normal) { p.normal[3 * o] = nx; p.normal[3 * o + 1] = ny; p.normal[3 * o + 2] = nz; }
    if (!p.frames) return;
    const int py = pix / p.W, px = pix - py * p.W;
    long long w[3];
    mr_cover(tr, px, py, w);
    float q[3], s;
    mr_depth(tr, w, q, s);
    const float b0 = q[0] / s, b1 = q[1] / s, b2 = q[2] / s;
    const float *eye = p.campos + 3 * view;
    const float lx = eye[0] - ((b0 * p0[0] + b1 * p1[0]) + b2 * p2[0]);
    const float ly = eye[1] - ((b0 * p0[1] + b1 * p1[1]) + b2 * p2[1]);
    const float lz = eye[2] - ((b0 * p0[2] + b1 * p1[2]) + b2 * p2[2]);
    const float ll = sqrtf((lx * lx + ly * ly) + lz * lz);
    const float ndl = (nx * (lx / ll) + ny * (ly / ll)) + nz * (lz / ll);
    const float shade = p.ambient + p.diffuse * fmaxf(ndl, 0.0f);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float alb = p.albedo[c];
        if (p.colors) alb = (b0 * p.colors[3 * (size_t)tr.idx[0] + c] + b1 * p.colors[3 * (size_t)tr.idx[1] + c]) + b2 * p.colors[3 * (size_t)tr.idx[2] + c];
        p.frames[3 * o + c] = mr_u8(alb * shade);
    }
}

struct MrLayout { int64_t snap, keys, list, count, total; };
bool mr_layout(int n, int H, int W, int Nv, int T, MrLayout *L) {
    if (n < 0 || n > 65535 || H <= 0 || W <= 0 || Nv < 0 || T < 0 || Nv >= (1 << 30) || T >= (1 << 30) || (long long)n * H * W >= (1ll << 31)) return false;
    int64_t o = 0;
    L->snap = o;   o = align_up(o + (int64_t)n * Nv * 16, 256);
    L->keys = o;   o = align_up(o + (int64_t)n * H * W * 8, 256);
    L->list = o;   o = align_up(o + (int64_t)n * T * 4, 256);
    L->count = o;  o = align_up(o + (int64_t)n * 8, 256);
    L->total = o + 256;
    return true;
}

}  // namespace

extern "C" {

int64_t lara_meshrender_workspace_bytes(int32_t n_views, int32_t H, int32_t W, int32_t Nv, int32_t T) {
    MrLayout L;
    return mr_layout(n_views, H, W, Nv, T, &L) ? L.total : (int64_t)LARA2DGS_E_INVALID;
}

int lara_meshrender_section_offsets(int32_t n_views, int32_t H, int32_t W, int32_t Nv, int32_t T, int64_t *offsets4) {
    MrLayout L;
    if (!offsets4 || !mr_layout(n_views, H, W, Nv, T, &L)) return LARA2DGS_E_INVALID;
    offsets4[0] = L.snap; offsets4[1] = L.keys; offsets4[2] = L.list; offsets4[3] = L.count;
    return LARA2DGS_OK;
}

int lara_meshrender_views(int32_t n_views, int32_t H, int32_t W, int32_t Nv, int32_t T, const float *vertices,
                          const int32_t *triangles, const float *vertex_colors, const float *viewmatrix, const float *projmatrix,
                          const float *campos, float znear, const float *shading, int32_t wave_box_area, int32_t *face_id,
                          float *depth, float *normal, uint8_t *frames, uint32_t *info, int32_t *err, void *workspace,
                          void *stream) {
    MrLayout L;
    if (!mr_layout(n_views, H, W, Nv, T, &L) || !workspace || !shading || !(znear >= 0.0f)) return LARA2DGS_E_INVALID;
    if (n_views == 0) return LARA2DGS_OK;
    const bool mesh = Nv > 0 && T > 0;
    if (Nv > 0 && (!vertices || !viewmatrix || !projmatrix)) return LARA2DGS_E_INVALID;
    if (mesh && (!triangles || !campos)) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    MrArgs p;
    p.n = n_views; p.H = H; p.W = W; p.Nv = Nv; p.T = T;
    p.vertices = vertices; p.triangles = triangles; p.colors = vertex_colors; p.view = viewmatrix; p.proj = projmatrix; p.campos = campos;
    p.znear = znear;
    p.mesh = mesh ? 1 : 0;
    p.wave_box_area = wave_box_area > 0 ? wave_box_area : MR_WAVE_BOX_AREA;
    for (int c = 0; c < 3; c++) { p.albedo[c] = shading[c]; p.background[c] = shading[3 + c]; }
    p.ambient = shading[6]; p.diffuse = shading[7];
    char *ws = (char *)workspace;
    p.snap = (int4 *)(ws + L.snap); p.keys = (unsigned long long *)(ws + L.keys); p.list = (int *)(ws + L.list); p.count = (unsigned *)(ws + L.count);
    p.face_id = face_id; p.depth = depth; p.normal = normal; p.frames = frames; p.info = info; p.err = err;
    const long long pixels = (long long)n_views * H * W;
    const long long fill = pixels > 4ll * n_views ? pixels : 4ll * n_views;
    L2D_LAUNCH_IN_SCOPE(s, mr_fill_kernel, dim3((unsigned)((fill + 255) / 256)), dim3(256), 0, p);
    if (Nv > 0) L2D_LAUNCH_IN_SCOPE(s, mr_snap_kernel, dim3((unsigned)((Nv + 255) / 256), 1, (unsigned)n_views), dim3(256), 0, p);
    if (mesh) {
        const unsigned tblocks = (unsigned)((T + 255) / 256);
        L2D_LAUNCH_IN_SCOPE(s, mr_raster_kernel, dim3(tblocks, 1, (unsigned)n_views), dim3(256), 0, p);
        // a wave per listed triangle, grid-strided: the list's length stays on the device
        const unsigned wblocks = (unsigned)(((long long)T + 3) / 4 < 2048 ? ((long long)T + 3) / 4 : 2048);
        L2D_LAUNCH_IN_SCOPE(s, mr_raster_wave_kernel, dim3(wblocks, 1, (unsigned)n_views), dim3(256), 0, p);
    }
    if (face_id || depth || normal || frames || (info && mesh))
        L2D_LAUNCH_IN_SCOPE(s, mr_resolve_kernel, dim3((unsigned)(((long long)H * W + 255) / 256), 1, (unsigned)n_views), dim3(256), 0, p);
    return LARA2DGS_OK;
}

}  // extern "C"
