// trimesh.h -- what the searches over a mesh's triangles share (meshdist.hip: the grid; meshbvh.hip: the hierarchy; meshray.hip:
// the rays on it; meshmetrics.hip and unigrid.h for the box and the candidate): the validity rule of a triangle, the 48-byte record
// {p0, p1, p2, id or -1}, the reduction of a box to part[block][6] and its gather, the candidate with the tie rule, and the write
// of a settled query.  One definition each, so the grid and the hierarchy return the same bits by construction.  Everything sits
// in an unnamed namespace and is __forceinline__: each unit that includes this header owns its copies.  Include it from units built
// with -ffp-contract=off only.
#pragma once
#include "common.h"
#include "wave.h"
#include "tridist.h"

#include <cmath>

namespace {

constexpr int NEAREST_NONE = 0x7fffffff;      // the id of "no candidate at all"

// ---- the triangle and its record ------------------------------------------------------------------------------------------------

// the three vertices of triangle i; false: an index outside [0, Nv) or a coordinate that is not finite (p is then zero)
__device__ __forceinline__ bool tri_fetch(const int Nv, const float *__restrict__ v, const int *__restrict__ t, const long long i,
                                          float p[3][3]) {
    const int id[3] = {t[3 * i], t[3 * i + 1], t[3 * i + 2]};
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; k++) ok = ok && id[k] >= 0 && id[k] < Nv;
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            p[k][j] = v[3 * (size_t)(ok ? id[k] : 0) + j];
            ok = ok && fabsf(p[k][j]) < INFINITY;
        }
    if (!ok) {
#pragma unroll
        for (int k = 0; k < 3; k++)
#pragma unroll
            for (int j = 0; j < 3; j++) p[k][j] = 0.0f;
    }
    return ok;
}

// a query point the searches take: every coordinate finite
__device__ __forceinline__ bool tri_point_finite(const float p[3]) {
    return fabsf(p[0]) < INFINITY && fabsf(p[1]) < INFINITY && fabsf(p[2]) < INFINITY;
}

struct TriRec { float p[3][3]; int id; };
__device__ __forceinline__ TriRec tri_unpack(const float4 a, const float4 b, const float4 c) {
    TriRec r;
    r.p[0][0] = a.x; r.p[0][1] = a.y; r.p[0][2] = a.z;
    r.p[1][0] = a.w; r.p[1][1] = b.x; r.p[1][2] = b.y;
    r.p[2][0] = b.z; r.p[2][1] = b.w; r.p[2][2] = c.x;
    r.id = __float_as_int(c.y);
    return r;
}
__device__ __forceinline__ TriRec tri_load(const float4 *__restrict__ rec, const int i) {
    return tri_unpack(rec[3 * (size_t)i], rec[3 * (size_t)i + 1], rec[3 * (size_t)i + 2]);
}
__device__ __forceinline__ void tri_store(float4 *rec, const size_t j, const float (&p)[3][3], const int id) {
    rec[3 * j] = make_float4(p[0][0], p[0][1], p[0][2], p[1][0]);
    rec[3 * j + 1] = make_float4(p[1][1], p[1][2], p[2][0], p[2][1]);
    rec[3 * j + 2] = make_float4(p[2][2], __int_as_float(id), 0.0f, 0.0f);
}

// ---- boxes ----------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ void box_grow(float (&lo)[3], float (&hi)[3], const float (&p)[3][3]) {
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            lo[j] = fminf(lo[j], p[k][j]);
            hi[j] = fmaxf(hi[j], p[k][j]);
        }
}

// a workgroup of 256: part[block][6] = min x y z, max x y z over its threads' boxes
__device__ __forceinline__ void box_block_partial(float (&lo)[3], float (&hi)[3], float *part) {
    __shared__ float red[6][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        lo[j] = wave_min(lo[j]);
        hi[j] = wave_max(hi[j]);
        if (lane == 0) { red[j][wave] = lo[j]; red[3 + j][wave] = hi[j]; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int j = threadIdx.x;
        const float a = red[j][0], b = red[j][1], c = red[j][2], d = red[j][3];
        part[blockIdx.x * 6 + j] = j < 3 ? fminf(fminf(a, b), fminf(c, d)) : fmaxf(fmaxf(a, b), fmaxf(c, d));
    }
}

// one wave: the box lo, hi (the caller's empty box) grown by all partials, in every lane
__device__ __forceinline__ void box_gather_partials(const int blocks, const float *part, float (&lo)[3], float (&hi)[3]) {
    for (int b = threadIdx.x; b < blocks; b += 64)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            lo[j] = fminf(lo[j], part[b * 6 + j]);
            hi[j] = fmaxf(hi[j], part[b * 6 + 3 + j]);
        }
#pragma unroll
    for (int j = 0; j < 3; j++) {
        lo[j] = wave_min(lo[j]);
        hi[j] = wave_max(hi[j]);
    }
}

// ---- the candidate --------------------------------------------------------------------------------------------------------------

// the best candidate so far.  The tie rule: the smaller value wins, and of two equal values the smaller id
template <class D>
struct Nearest {
    D d2;
    int id;
    __device__ __forceinline__ bool take(const D d, const int i) {      // true: (d, i) is the candidate now
        if (d < d2 || (d == d2 && i < id)) { d2 = d; id = i; return true; }
        return false;
    }
};

// dist, face and the closest point of a settled query (id = NEAREST_NONE: no candidate at all); pos = the winner's record
__device__ __forceinline__ void tri_write_result(const int i, const float q[3], const Nearest<double> &best,
                                                 const float4 *rec, const int pos, float *dist, int *face, float *closest) {
    const bool none = best.id == NEAREST_NONE;
    dist[i] = none ? INFINITY : (float)sqrt(best.d2);
    face[i] = none ? -1 : best.id;
    if (!closest) return;
    double c[3] = {NAN, NAN, NAN};
    if (!none) {
        const TriRec m = tri_load(rec, pos);
        lara_tridist(q, m.p[0], m.p[1], m.p[2], c);
    }
#pragma unroll
    for (int j = 0; j < 3; j++) closest[3 * (size_t)i + j] = (float)c[j];
}

}  // namespace
