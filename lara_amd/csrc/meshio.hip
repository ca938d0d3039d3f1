// meshio.hip -- the extracted mesh as file bytes on gfx950: OBJ text and binary PLY rows.  Interface, the text's definition and the
// limits in include/lara_meshio.h; the number formatting (exact "%.9g", integer arithmetic) in fmt9g.h.
//
//   mio_obj_lengths_kernel<FACE>   one thread per line, 256 lines per workgroup: the line's tokens are decomposed only for their
//                                  lengths, the workgroup adds them up and stores one int64 total
//   mio_obj_emit_kernel<FACE>      the same mapping: lengths, an in-block exclusive scan, every thread writes its line into LDS at its
//                                  offset, the workgroup copies the span to out + block_offsets[b]
//   mio_ply_pack_kernel<FACE>      packed rows of 12 / 15 / 24 / 27 or 13 bytes through LDS in the same way; closed-form offsets
//   mio_copy_span                  LDS -> global: the span sits in LDS at the destination's offset within its 16-byte line, so both
//                                  sides of the 16-byte copies are aligned; byte stores for the head and the tail only
// A line never reaches HBM as scattered per-thread byte stores.  An index out of range is written as 0 in every kernel, so lengths
// and emitted bytes agree whatever the input holds, and sets the error word.
#include "common.h"
#include "wave.h"
#include "fmt9g.h"
#include "../../include/lara_meshio.h"

namespace {

constexpr int MIO_BLOCK = LARA_MESHIO_BLOCK_LINES;
constexpr int MIO_WAVES = MIO_BLOCK / 64;
static_assert(LARA_MESHIO_MAX_F32_TOKEN == LARA_FMT9G_MAX_TOKEN && LARA_MESHIO_MAX_U32_TOKEN == LARA_FMT_U32_MAX_TOKEN, "token lengths");
static_assert(LARA_MESHIO_MAX_VERTEX_LINE == 1 + 6 * (1 + LARA_MESHIO_MAX_F32_TOKEN) + 1, "vertex line");
static_assert(LARA_MESHIO_MAX_FACE_LINE == 1 + 3 * (1 + LARA_MESHIO_MAX_U32_TOKEN) + 1, "face line");

int64_t mio_blocks(const int64_t n) { return (n + MIO_BLOCK - 1) / MIO_BLOCK; }
bool mio_sizes_ok(const int64_t nv, const int64_t nt) {
    return nv >= 0 && nv <= LARA_MESHIO_MAX_VERTICES && nt >= 0 && nt <= LARA_MESHIO_MAX_TRIANGLES;
}

// index j of the triangle array (int32 or int64); out of range: 0 and `bad` set
__device__ __forceinline__ uint32_t mio_index(const void *tri, const int index_bytes, const long long j, bool &bad) {
    const long long v = index_bytes == 8 ? ((const long long *)tri)[j] : (long long)((const int *)tri)[j];
    if (v < 0 || v > (long long)LARA_MESHIO_MAX_INDEX) {
        bad = true;
        return 0u;
    }
    return (uint32_t)v;
}

// the sum of v over the workgroup, in every thread (tot: MIO_WAVES ints of LDS), and the exclusive prefix of the caller's v
__device__ __forceinline__ int mio_block_scan(const int v, int *tot, int &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int incl = wave_inclusive_scan(v, lane);
    if (lane == 63) tot[wave] = incl;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < MIO_WAVES; ++w) {
        const int t = tot[w];
        if (w < wave) before += t;
        total += t;
    }
    return before + incl - v;
}

// span[shift .. shift + total) -> dst[0 .. total), shift = dst's offset within its 16-byte line; the whole workgroup
__device__ __forceinline__ void mio_copy_span(const unsigned char *span, unsigned char *dst, const int shift, const int total) {
    unsigned char *base = dst - shift;      // 16-byte aligned
    const int end = shift + total;
    for (int c = threadIdx.x * 16; c < end; c += MIO_BLOCK * 16) {
        if (c >= shift && c + 16 <= end) {
            *(uint4 *)(base + c) = *(const uint4 *)(span + c);
        } else {
            const int lo = c > shift ? c : shift, hi = c + 16 < end ? c + 16 : end;
            for (int j = lo; j < hi; ++j) base[j] = span[j];
        }
    }
}

struct MioLine {      // one line's numbers, decomposed
    lara_dec9 f[6];
    uint32_t idx[3];
    int len;
};

template <bool FACE>
__device__ __forceinline__ MioLine mio_line(const long long line, const float *vertices, const float *colors, const void *tri,
                                            const int index_bytes, bool &bad) {
    MioLine L;
    L.len = 2;      // the letter and the newline
    if (FACE) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            L.idx[j] = mio_index(tri, index_bytes, 3 * line + j, bad) + 1u;
            L.len += 1 + lara_fmt_digits_u32(L.idx[j]);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            L.f[j] = lara_fmt9g_decompose(vertices[3 * line + j]);
            L.len += 1 + lara_fmt9g_len(L.f[j]);
        }
        if (colors) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                L.f[3 + j] = lara_fmt9g_decompose(colors[3 * line + j]);
                L.len += 1 + lara_fmt9g_len(L.f[3 + j]);
            }
        }
    }
    return L;
}

template <bool FACE>
__global__ __launch_bounds__(MIO_BLOCK) void mio_obj_lengths_kernel(const long long n, const float *__restrict__ vertices,
                                                                    const float *__restrict__ colors, const void *__restrict__ tri,
                                                                    const int index_bytes, long long *__restrict__ totals,
                                                                    unsigned long long *__restrict__ err) {
    __shared__ int tot[MIO_WAVES];
    const long long line = (long long)blockIdx.x * MIO_BLOCK + threadIdx.x;
    bool bad = false;
    int len = 0;
    if (line < n) len = mio_line<FACE>(line, vertices, colors, tri, index_bytes, bad).len;
    const int sum = wave_sum(len);
    if ((threadIdx.x & 63) == 0) tot[threadIdx.x >> 6] = sum;
    if (bad) atomicOr(err, (unsigned long long)LARA_MESHIO_ERR_INDEX);
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < MIO_WAVES; ++w) t += tot[w];
        totals[blockIdx.x] = t;
    }
}

template <bool FACE>
__global__ __launch_bounds__(MIO_BLOCK) void mio_obj_emit_kernel(const long long n, const float *__restrict__ vertices,
                                                                 const float *__restrict__ colors, const void *__restrict__ tri,
                                                                 const int index_bytes, const long long *__restrict__ block_offsets,
                                                                 unsigned char *__restrict__ out) {
    constexpr int LINE = FACE ? LARA_MESHIO_MAX_FACE_LINE : LARA_MESHIO_MAX_VERTEX_LINE;
    __shared__ __attribute__((aligned(16))) unsigned char span[MIO_BLOCK * LINE + 16];
    __shared__ int tot[MIO_WAVES];
    const long long line = (long long)blockIdx.x * MIO_BLOCK + threadIdx.x;
    const bool active = line < n;
    bool bad = false;
    MioLine L;
    L.len = 0;
    if (active) L = mio_line<FACE>(line, vertices, colors, tri, index_bytes, bad);
    int total;
    const int offset = mio_block_scan(L.len, tot, total);      // total <= MIO_BLOCK * LINE: every line is at most LINE bytes
    unsigned char *dst = out + block_offsets[blockIdx.x];
    const int shift = (int)((uintptr_t)dst & 15);
    if (active) {
        unsigned char *p = span + shift + offset;
        *p++ = FACE ? 'f' : 'v';
        if (FACE) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                *p++ = ' ';
                p += lara_fmt_u32_write(L.idx[j], p);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                *p++ = ' ';
                p += lara_fmt9g_write(L.f[j], p);
            }
            if (colors) {
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    *p++ = ' ';
                    p += lara_fmt9g_write(L.f[3 + j], p);
                }
            }
        }
        *p = '\n';
    }
    __syncthreads();
    mio_copy_span(span, dst, shift, total);
}

__device__ __forceinline__ void mio_put32(unsigned char *p, const uint32_t v) {
    p[0] = (unsigned char)v, p[1] = (unsigned char)(v >> 8), p[2] = (unsigned char)(v >> 16), p[3] = (unsigned char)(v >> 24);
}

__device__ __forceinline__ unsigned char mio_color_u8(const float c) {
    if (!(c == c)) return 0;
    const float x = c < 0.0f ? 0.0f : (c > 1.0f ? 1.0f : c);
    return (unsigned char)(int)floor(255.0 * (double)x + 0.5);
}

template <bool FACE>
__global__ __launch_bounds__(MIO_BLOCK) void mio_ply_pack_kernel(const long long n, const float *__restrict__ vertices,
                                                                 const float *__restrict__ normals, const float *__restrict__ colors,
                                                                 const void *__restrict__ tri, const int index_bytes, const int row_bytes,
                                                                 unsigned char *__restrict__ out, unsigned long long *__restrict__ err) {
    constexpr int ROW = FACE ? LARA_MESHIO_PLY_FACE_ROW : 27;
    __shared__ __attribute__((aligned(16))) unsigned char span[MIO_BLOCK * ROW + 16];
    const long long first = (long long)blockIdx.x * MIO_BLOCK, row = first + threadIdx.x;
    const long long left = n - first;
    const int rows = left < MIO_BLOCK ? (int)left : MIO_BLOCK;
    unsigned char *dst = out + first * row_bytes;
    const int shift = (int)((uintptr_t)dst & 15);
    if (row < n) {
        unsigned char *p = span + shift + (int)threadIdx.x * row_bytes;
        if (FACE) {
            bool bad = false;
            *p++ = 3;
#pragma unroll
            for (int j = 0; j < 3; ++j) mio_put32(p + 4 * j, mio_index(tri, index_bytes, 3 * row + j, bad));
            if (bad) atomicOr(err, (unsigned long long)LARA_MESHIO_ERR_INDEX);
        } else {
#pragma unroll
            for (int j = 0; j < 3; ++j) mio_put32(p + 4 * j, __float_as_uint(vertices[3 * row + j]));
            p += 12;
            if (normals) {
#pragma unroll
                for (int j = 0; j < 3; ++j) mio_put32(p + 4 * j, __float_as_uint(normals[3 * row + j]));
                p += 12;
            }
            if (colors) {
#pragma unroll
                for (int j = 0; j < 3; ++j) p[j] = mio_color_u8(colors[3 * row + j]);
            }
        }
    }
    __syncthreads();
    mio_copy_span(span, dst, shift, rows * row_bytes);
}

int mio_row_bytes(const int has_normals, const int has_colors) { return 12 + (has_normals ? 12 : 0) + (has_colors ? 3 : 0); }

}  // namespace

extern "C" {

int64_t lara_meshio_obj_workspace_bytes(int64_t nv, int64_t nt) {
    if (!mio_sizes_ok(nv, nt)) return LARA2DGS_E_INVALID;
    return 8 * (mio_blocks(nv) + mio_blocks(nt) + 1);
}

int lara_meshio_obj_lengths(int64_t nv, const float *vertices, const float *colors, int64_t nt, const void *triangles,
                            int32_t index_bytes, void *workspace, void *stream) {
    if (!mio_sizes_ok(nv, nt) || (index_bytes != 4 && index_bytes != 8)) return LARA2DGS_E_INVALID;
    if (nv == 0 && nt == 0) return LARA2DGS_OK;
    if ((nv > 0 && !vertices) || (nt > 0 && !triangles) || !workspace || ((uintptr_t)workspace & 7)) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const int64_t bv = mio_blocks(nv), bt = mio_blocks(nt);
    long long *totals = (long long *)workspace;
    unsigned long long *err = (unsigned long long *)(totals + bv + bt);
    L2D_HIP(hipMemsetAsync(err, 0, 8, s));
    if (nv > 0)
        L2D_LAUNCH_IN_SCOPE(s, mio_obj_lengths_kernel<false>, dim3((unsigned)bv), dim3(MIO_BLOCK), 0, (long long)nv, vertices,
                   colors, triangles, (int)index_bytes, totals, err);
    if (nt > 0)
        L2D_LAUNCH_IN_SCOPE(s, mio_obj_lengths_kernel<true>, dim3((unsigned)bt), dim3(MIO_BLOCK), 0, (long long)nt, vertices,
                   colors, triangles, (int)index_bytes, totals + bv, err);
    return LARA2DGS_OK;
}

int lara_meshio_obj_emit(int64_t nv, const float *vertices, const float *colors, int64_t nt, const void *triangles, int32_t index_bytes,
                         const int64_t *block_offsets, uint8_t *out, void *stream) {
    if (!mio_sizes_ok(nv, nt) || (index_bytes != 4 && index_bytes != 8)) return LARA2DGS_E_INVALID;
    if (nv == 0 && nt == 0) return LARA2DGS_OK;
    if ((nv > 0 && !vertices) || (nt > 0 && !triangles) || !block_offsets || !out) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const int64_t bv = mio_blocks(nv), bt = mio_blocks(nt);
    const long long *off = (const long long *)block_offsets;
    if (nv > 0)
        L2D_LAUNCH_IN_SCOPE(s, mio_obj_emit_kernel<false>, dim3((unsigned)bv), dim3(MIO_BLOCK), 0, (long long)nv, vertices, colors,
                   triangles, (int)index_bytes, off, (unsigned char *)out);
    if (nt > 0)
        L2D_LAUNCH_IN_SCOPE(s, mio_obj_emit_kernel<true>, dim3((unsigned)bt), dim3(MIO_BLOCK), 0, (long long)nt, vertices, colors,
                   triangles, (int)index_bytes, off + bv, (unsigned char *)out);
    return LARA2DGS_OK;
}

int64_t lara_meshio_ply_body_bytes(int64_t nv, int64_t nt, int32_t has_normals, int32_t has_colors) {
    if (!mio_sizes_ok(nv, nt)) return LARA2DGS_E_INVALID;
    return nv * mio_row_bytes(has_normals, has_colors) + nt * LARA_MESHIO_PLY_FACE_ROW;
}

int64_t lara_meshio_ply_workspace_bytes(void) { return 8; }

int lara_meshio_ply_pack(int64_t nv, const float *vertices, const float *normals, const float *colors, int64_t nt, const void *triangles,
                         int32_t index_bytes, uint8_t *out, void *workspace, void *stream) {
    if (!mio_sizes_ok(nv, nt) || (index_bytes != 4 && index_bytes != 8)) return LARA2DGS_E_INVALID;
    if (nv == 0 && nt == 0) return LARA2DGS_OK;
    if ((nv > 0 && !vertices) || (nt > 0 && !triangles) || !out || !workspace || ((uintptr_t)workspace & 7)) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    unsigned long long *err = (unsigned long long *)workspace;
    const int rb = mio_row_bytes(normals != nullptr, colors != nullptr);
    L2D_HIP(hipMemsetAsync(err, 0, 8, s));
    if (nv > 0)
        L2D_LAUNCH_IN_SCOPE(s, mio_ply_pack_kernel<false>, dim3((unsigned)mio_blocks(nv)), dim3(MIO_BLOCK), 0, (long long)nv,
                   vertices, normals, colors, triangles, (int)index_bytes, rb, (unsigned char *)out, err);
    if (nt > 0)
        L2D_LAUNCH_IN_SCOPE(s, mio_ply_pack_kernel<true>, dim3((unsigned)mio_blocks(nt)), dim3(MIO_BLOCK), 0, (long long)nt,
                   vertices, normals, colors, triangles, (int)index_bytes, (int)LARA_MESHIO_PLY_FACE_ROW, (unsigned char *)out + nv * rb, err);
    return LARA2DGS_OK;
}

int lara_meshio_format_f32_host(int64_t n, const float *v, char *out, int *len) {
    if (n < 0 || (n > 0 && (!v || !out || !len))) return LARA2DGS_E_INVALID;
    for (int64_t i = 0; i < n; ++i) len[i] = lara_fmt9g(v[i], out + 16 * i);
    return LARA2DGS_OK;
}

int lara_meshio_format_u32_host(int64_t n, const uint32_t *v, char *out, int *len) {
    if (n < 0 || (n > 0 && (!v || !out || !len))) return LARA2DGS_E_INVALID;
    for (int64_t i = 0; i < n; ++i) len[i] = lara_fmt_u32(v[i], out + 10 * i);
    return LARA2DGS_OK;
}

}  // extern "C"
