// splatpack.hip -- packing a cloud of surfels for Gaussian-splat viewers and unpacking it again.  Interface, the formats and every
// formula: lara_splatpack.h; the per-row functions, shared with the host entries: splatpack_ops.h.
//
//   sp_bounds_kernel<DEG>      256 rows per workgroup, one thread per row: the row's validity byte, then the minimum and maximum of the valid
//                              centres and the count of invalid rows by wave butterflies and one LDS exchange across the four waves,
//                              stored as eight words per workgroup into the workspace.
//   sp_bounds_finish_kernel    ONE workgroup walks the partial rows with a stride of 256, reduces the same way and stores the box and the
//                              count.  Minimum and maximum of canonical words (no -0.0, no NaN) do not depend on the order.
//   sp_morton_kernel, sp_importance_kernel    one thread per row: its 64-bit sort key.
//   sp_encode_kernel<DEG>      one workgroup per chunk of 256 output rows.  A thread gathers its row through `order`, the 18 bounds are
//                              reduced by wave butterflies and one LDS exchange, 18 threads store the record; every thread then quantises
//                              its row against the record in LDS and stores its four words as one 16-byte store.  The chunk's SH bytes
//                              are written four to a dword, consecutive lanes consecutive dwords, where the array starts on a dword
//                              (a chunk's 256 rows of 9, 24 or 45 bytes always end on one); the last partial dword and unaligned arrays
//                              go byte by byte.
//   sp_decode_kernel<DEG>      one thread per row: one 16-byte load, its chunk's record (the same 72 bytes for 256 consecutive threads).
//   sp_splat_encode_kernel<DEG>, sp_splat_decode_kernel    one thread per row, the 32-byte row as two 16-byte stores / loads.
#include "common.h"
#include "wave.h"
#include "splatpack_ops.h"
#include "lara_splatpack.h"

namespace {

constexpr int SP_SPAN = LARA_SPLATPACK_SPAN;
constexpr int SP_F = LARA_SURFEL_FIELDS;
constexpr int SP_V = LARA_SPLATPACK_VALUES;
constexpr int SP_REC = LARA_SPLATPACK_RECORD;
constexpr int64_t SP_MAX_P = (int64_t)1 << 27;       // row indices fit the low 32 bits of a key, and an int in LDS
static_assert(SP_SPAN == LARA_SPLATPACK_ROWS && SP_SPAN == 256, "one thread per row of a chunk, four waves");

struct SpPlan {
    double v[LARA_SPLATPACK_PLAN];
};
struct SpIn {
    const float *p[SP_F];
};
struct SpOut {
    float *p[SP_F];
};

__device__ __forceinline__ float sp_inf() { return __int_as_float(0x7F800000); }

template <int DEG>
__global__ void __launch_bounds__(SP_SPAN)
sp_bounds_kernel(const long long P, const SpIn in, uint8_t *__restrict__ valid, float *__restrict__ partial) {
    __shared__ float part[4][8];
    const long long s = (long long)blockIdx.x * SP_SPAN + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool ok = false;
    if (s < P) {
        ok = lara_splatpack_row_valid(DEG, s, in.p);
        valid[s] = ok ? 1 : 0;
    }
    float lo[3], hi[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float v = ok ? lara_splatpack_canon(in.p[0][3 * s + a]) : 0.0f;
        lo[a] = wave_min(ok ? v : sp_inf());
        hi[a] = wave_max(ok ? v : -sp_inf());
    }
    const int gone = wave_sum((s < P && !ok) ? 1 : 0);
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) part[wave][a] = lo[a], part[wave][3 + a] = hi[a];
        part[wave][6] = __int_as_float(gone);
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < 7) {
        float r = part[0][t];
        if (t < 3)
            for (int w = 1; w < 4; ++w) r = fminf(r, part[w][t]);
        else if (t < 6)
            for (int w = 1; w < 4; ++w) r = fmaxf(r, part[w][t]);
        else
            r = __int_as_float(__float_as_int(part[0][6]) + __float_as_int(part[1][6]) + __float_as_int(part[2][6]) + __float_as_int(part[3][6]));
        partial[(long long)blockIdx.x * 8 + t] = r;
    }
}

__global__ void __launch_bounds__(SP_SPAN)
sp_bounds_finish_kernel(const long long blocks, const float *__restrict__ partial, float *__restrict__ box, long long *__restrict__ dropped) {
    __shared__ float part[4][6];
    __shared__ long long gone_of[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float lo[3] = {sp_inf(), sp_inf(), sp_inf()}, hi[3] = {-sp_inf(), -sp_inf(), -sp_inf()};
    long long gone = 0;
    for (long long b = threadIdx.x; b < blocks; b += SP_SPAN) {
        const float *row = partial + b * 8;
#pragma unroll
        for (int a = 0; a < 3; ++a) lo[a] = fminf(lo[a], row[a]), hi[a] = fmaxf(hi[a], row[3 + a]);
        gone += __float_as_int(row[6]);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) lo[a] = wave_min(lo[a]), hi[a] = wave_max(hi[a]);
    gone = wave_sum_xor(gone);
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) part[wave][a] = lo[a], part[wave][3 + a] = hi[a];
        gone_of[wave] = gone;
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < 3) box[t] = fminf(fminf(part[0][t], part[1][t]), fminf(part[2][t], part[3][t]));
    else if (t < 6) box[t] = fmaxf(fmaxf(part[0][t], part[1][t]), fmaxf(part[2][t], part[3][t]));
    else if (t == 6) *dropped = gone_of[0] + gone_of[1] + gone_of[2] + gone_of[3];
}

__global__ void __launch_bounds__(SP_SPAN)
sp_morton_kernel(const long long P, const float *__restrict__ centers, const uint8_t *__restrict__ valid, const float *__restrict__ box,
                 long long *__restrict__ keys) {
    const long long s = (long long)blockIdx.x * SP_SPAN + threadIdx.x;
    if (s >= P) return;
    float b[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) b[a] = box[a];
    keys[s] = lara_splatpack_morton_key(s, valid[s] != 0, centers + 3 * s, b);
}

__global__ void __launch_bounds__(SP_SPAN)
sp_importance_kernel(const SpPlan plan, const long long P, const float *__restrict__ opacity, const float *__restrict__ scales,
                     const uint8_t *__restrict__ valid, long long *__restrict__ keys) {
    const long long s = (long long)blockIdx.x * SP_SPAN + threadIdx.x;
    if (s >= P) return;
    keys[s] = lara_splatpack_importance_key(plan.v, s, valid[s] != 0, opacity[s], scales + 2 * s);
}

template <int DEG>
__global__ void __launch_bounds__(SP_SPAN)
sp_encode_kernel(const SpPlan plan, const long long P, const long long P_out, const SpIn in, const long long *__restrict__ order,
                 float *__restrict__ chunks, uint4 *__restrict__ words, uint8_t *__restrict__ sh) {
    constexpr int N = (DEG + 1) * (DEG + 1), W = 3 * (N - 1);
    __shared__ float part[4][SP_REC];
    __shared__ float rec[SP_REC];
    __shared__ int source[SP_SPAN];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long first = (long long)blockIdx.x * SP_SPAN, i = first + t;
    long long s = i < P_out ? order[i] : -1;
    const bool live = s >= 0 && s < P;
    s = live ? s : 0;
    source[t] = live ? (int)s : -1;
    float v[SP_V];
    if (live) lara_splatpack_values(plan.v, in.p[0] + 3 * s, in.p[1] + 3 * N * s, in.p[3] + 2 * s, v);
#pragma unroll
    for (int j = 0; j < SP_V; ++j) {
        const float lo = wave_min(live ? v[j] : sp_inf()), hi = wave_max(live ? v[j] : -sp_inf());
        if (lane == 0) part[wave][lara_splatpack_min_slot(j)] = lo, part[wave][lara_splatpack_max_slot(j)] = hi;
    }
    __syncthreads();
    if (t < SP_REC) {
        const bool is_min = t % 6 < 3;
        float r = part[0][t];
        for (int w = 1; w < 4; ++w) r = is_min ? fminf(r, part[w][t]) : fmaxf(r, part[w][t]);
        rec[t] = r;
        chunks[(long long)blockIdx.x * SP_REC + t] = r;
    }
    __syncthreads();
    if (i < P_out) {
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (live) {
            float r[SP_REC];
#pragma unroll
            for (int k = 0; k < SP_REC; ++k) r[k] = rec[k];
            lara_splatpack_row_words(v, r, in.p[2][s], in.p[4] + 4 * s, w);
        }
        words[i] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    if constexpr (W > 0) {
        const long long left = P_out - first;
        const int rows = left < SP_SPAN ? (int)left : SP_SPAN;
        const int bytes = rows * W;
        uint8_t *base = sh + first * W;
        const float *shs = in.p[1];
        auto code = [&](const int b) -> uint32_t {
            const int r = b / W, src = source[r];
            return src < 0 ? 0u : lara_splatpack_sh_byte(shs + (long long)3 * N * src, N, b - r * W);
        };
        const int whole = (((uintptr_t)sh & 3u) == 0) ? bytes / 4 : 0;      // (first W is a multiple of 4 bytes: 256 rows per chunk)
        for (int d = t; d < whole; d += SP_SPAN)
            ((uint32_t *)base)[d] = code(4 * d) | code(4 * d + 1) << 8 | code(4 * d + 2) << 16 | code(4 * d + 3) << 24;
        for (int b = 4 * whole + t; b < bytes; b += SP_SPAN) base[b] = (uint8_t)code(b);
    }
}

template <int DEG>
__global__ void __launch_bounds__(SP_SPAN)
sp_decode_kernel(const long long P_out, const float *__restrict__ chunks, const uint4 *__restrict__ words, const uint8_t *__restrict__ sh,
                 const SpOut out) {
    constexpr int N = (DEG + 1) * (DEG + 1), W = 3 * (N - 1);
    const long long i = (long long)blockIdx.x * SP_SPAN + threadIdx.x;
    if (i >= P_out) return;
    float rec[SP_REC];
#pragma unroll
    for (int k = 0; k < SP_REC; ++k) rec[k] = chunks[(long long)blockIdx.x * SP_REC + k];
    const uint4 q = words[i];
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
    lara_splatpack_unrow(rec, w, out.p[0] + 3 * i, out.p[1] + 3 * N * i, out.p[2] + i, out.p[3] + 2 * i, out.p[4] + 4 * i);
    if constexpr (W > 0)
        for (int j = 0; j < W; ++j) out.p[1][3 * N * i + 3 * (1 + j % (N - 1)) + j / (N - 1)] = lara_splatpack_sh_value(sh[i * W + j]);
}

template <int DEG>
__global__ void __launch_bounds__(SP_SPAN)
sp_splat_encode_kernel(const SpPlan plan, const long long P, const long long P_out, const SpIn in, const long long *__restrict__ order,
                       uint4 *__restrict__ rows) {
    constexpr int N = (DEG + 1) * (DEG + 1);
    const long long i = (long long)blockIdx.x * SP_SPAN + threadIdx.x;
    if (i >= P_out) return;
    const long long s = order[i];
    uint32_t w[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    if (s >= 0 && s < P) lara_splatpack_splat_row(plan.v, in.p[0] + 3 * s, in.p[1] + 3 * N * s, in.p[2][s], in.p[3] + 2 * s, in.p[4] + 4 * s, w);
    rows[2 * i] = make_uint4(w[0], w[1], w[2], w[3]);
    rows[2 * i + 1] = make_uint4(w[4], w[5], w[6], w[7]);
}

__global__ void __launch_bounds__(SP_SPAN)
sp_splat_decode_kernel(const long long P_out, const uint4 *__restrict__ rows, const SpOut out) {
    const long long i = (long long)blockIdx.x * SP_SPAN + threadIdx.x;
    if (i >= P_out) return;
    const uint4 a = rows[2 * i], b = rows[2 * i + 1];
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    lara_splatpack_splat_unrow(w, out.p[0] + 3 * i, out.p[1] + 3 * i, out.p[2] + i, out.p[3] + 2 * i, out.p[4] + 4 * i);
}

int64_t sp_blocks(const int64_t n) { return (n + SP_SPAN - 1) / SP_SPAN; }

bool sp_all(const void *const *ptrs, const int n) {
    for (int i = 0; i < n; ++i)
        if (!ptrs[i]) return false;
    return true;
}

// the sizes every entry takes: a grid of sp_blocks(rows) <= 2^19 workgroups always fits a launch, as does every array's index in int64
bool sp_sizes_ok(const int32_t sh_degree, const int64_t P, const int64_t P_out) {
    return sh_degree >= 0 && sh_degree <= 3 && P >= 0 && P <= SP_MAX_P && P_out >= 0 && P_out <= P && sp_blocks(P) <= 0x7fffffffll;
}

bool sp_aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

bool sp_fields_ok(const void *const *five) { return five && sp_all(five, SP_F); }

bool sp_encode_ok(const double *plan, const int32_t sh_degree, const int64_t P, const int64_t P_out, const float *const *in, const void *order,
                  const void *chunks, const void *words, const void *sh) {
    return plan && sp_sizes_ok(sh_degree, P, P_out) && sp_fields_ok((const void *const *)in) && order && chunks && words && sp_aligned16(words) &&
           (sh || sh_degree == 0);
}

bool sp_decode_ok(const int32_t sh_degree, const int64_t P_out, const void *chunks, const void *words, const void *sh, float *const *out) {
    return sp_sizes_ok(sh_degree, P_out, P_out) && chunks && words && sp_aligned16(words) && (sh || sh_degree == 0) &&
           sp_fields_ok((const void *const *)out);
}

SpIn sp_in(const float *const *in) {
    SpIn a;
    for (int f = 0; f < SP_F; ++f) a.p[f] = in[f];
    return a;
}

SpOut sp_out(float *const *out) {
    SpOut a;
    for (int f = 0; f < SP_F; ++f) a.p[f] = out[f];
    return a;
}

SpPlan sp_plan(const double *plan) {
    SpPlan a;
    for (int i = 0; i < LARA_SPLATPACK_PLAN; ++i) a.v[i] = plan[i];
    return a;
}

}  // namespace

#define SP_BY_DEGREE(degree, GO) \
    switch (degree) {            \
    case 0: GO(0); break;        \
    case 1: GO(1); break;        \
    case 2: GO(2); break;        \
    default: GO(3); break;       \
    }

extern "C" {

int64_t lara_splatpack_workspace_bytes(int64_t P) {
    if (P < 0 || P > SP_MAX_P) return LARA2DGS_E_INVALID;
    return (sp_blocks(P) * 8 + 64) * (int64_t)sizeof(float);
}

int lara_splatpack_bounds(int32_t sh_degree, int64_t P, const float *const *in, uint8_t *valid, float *box, int64_t *dropped, void *workspace,
                          void *stream) {
    if (!sp_sizes_ok(sh_degree, P, 0) || !sp_fields_ok((const void *const *)in) || !valid || !box || !dropped || !workspace) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const SpIn a = sp_in(in);
    const long long blocks = sp_blocks(P);
#define SP_GO(DEG) L2D_LAUNCH_IN_SCOPE(s, sp_bounds_kernel<DEG>, dim3((unsigned)blocks), dim3(SP_SPAN), 0, (long long)P, a, valid, (float *)workspace)
    if (P > 0) SP_BY_DEGREE(sh_degree, SP_GO)
#undef SP_GO
    L2D_LAUNCH_IN_SCOPE(s, sp_bounds_finish_kernel, dim3(1), dim3(SP_SPAN), 0, blocks, (const float *)workspace, box, (long long *)dropped);
    return LARA2DGS_OK;
}

int lara_splatpack_bounds_host(int32_t sh_degree, int64_t P, const float *const *in, uint8_t *valid, float *box, int64_t *dropped,
                               void *workspace) {
    (void)workspace;                                 // (not used here)
    if (!sp_sizes_ok(sh_degree, P, 0) || !sp_fields_ok((const void *const *)in) || !valid || !box || !dropped) return LARA2DGS_E_INVALID;
    lara_splatpack_host_bounds(sh_degree, P, in, valid, box, dropped);
    return LARA2DGS_OK;
}

int lara_splatpack_morton_keys(int64_t P, const float *centers, const uint8_t *valid, const float *box, int64_t *keys, void *stream) {
    if (!sp_sizes_ok(0, P, 0) || !centers || !valid || !box || !keys) return LARA2DGS_E_INVALID;
    if (P == 0) return LARA2DGS_OK;
    L2D_LAUNCH_IN_SCOPE((hipStream_t)stream, sp_morton_kernel, dim3((unsigned)sp_blocks(P)), dim3(SP_SPAN), 0, (long long)P, centers, valid, box,
                        (long long *)keys);
    return LARA2DGS_OK;
}

int lara_splatpack_morton_keys_host(int64_t P, const float *centers, const uint8_t *valid, const float *box, int64_t *keys) {
    if (!sp_sizes_ok(0, P, 0) || !centers || !valid || !box || !keys) return LARA2DGS_E_INVALID;
    lara_splatpack_host_morton_keys(P, centers, valid, box, keys);
    return LARA2DGS_OK;
}

int lara_splatpack_importance_keys(const double *plan, int64_t P, const float *opacity, const float *scales, const uint8_t *valid,
                                   int64_t *keys, void *stream) {
    if (!plan || !sp_sizes_ok(0, P, 0) || !opacity || !scales || !valid || !keys) return LARA2DGS_E_INVALID;
    if (P == 0) return LARA2DGS_OK;
    L2D_LAUNCH_IN_SCOPE((hipStream_t)stream, sp_importance_kernel, dim3((unsigned)sp_blocks(P)), dim3(SP_SPAN), 0, sp_plan(plan), (long long)P,
                        opacity, scales, valid, (long long *)keys);
    return LARA2DGS_OK;
}

int lara_splatpack_importance_keys_host(const double *plan, int64_t P, const float *opacity, const float *scales, const uint8_t *valid,
                                        int64_t *keys) {
    if (!plan || !sp_sizes_ok(0, P, 0) || !opacity || !scales || !valid || !keys) return LARA2DGS_E_INVALID;
    lara_splatpack_host_importance_keys(plan, P, opacity, scales, valid, keys);
    return LARA2DGS_OK;
}

int lara_splatpack_encode(const double *plan, int32_t sh_degree, int64_t P, int64_t P_out, const float *const *in, const int64_t *order,
                          float *chunks, uint32_t *words, uint8_t *sh, void *stream) {
    if (!sp_encode_ok(plan, sh_degree, P, P_out, in, order, chunks, words, sh)) return LARA2DGS_E_INVALID;
    if (P_out == 0) return LARA2DGS_OK;
    hipStream_t s = (hipStream_t)stream;
    const SpIn a = sp_in(in);
    const SpPlan row = sp_plan(plan);
#define SP_GO(DEG)                                                                                                                        \
    L2D_LAUNCH_IN_SCOPE(s, sp_encode_kernel<DEG>, dim3((unsigned)sp_blocks(P_out)), dim3(SP_SPAN), 0, row, (long long)P, (long long)P_out, a, \
                        (const long long *)order, chunks, (uint4 *)words, sh)
    SP_BY_DEGREE(sh_degree, SP_GO)
#undef SP_GO
    return LARA2DGS_OK;
}

int lara_splatpack_encode_host(const double *plan, int32_t sh_degree, int64_t P, int64_t P_out, const float *const *in, const int64_t *order,
                               float *chunks, uint32_t *words, uint8_t *sh) {
    if (!sp_encode_ok(plan, sh_degree, P, P_out, in, order, chunks, words, sh)) return LARA2DGS_E_INVALID;
    lara_splatpack_host_encode(plan, sh_degree, P, P_out, in, order, chunks, words, sh);
    return LARA2DGS_OK;
}

int lara_splatpack_decode(int32_t sh_degree, int64_t P_out, const float *chunks, const uint32_t *words, const uint8_t *sh, float *const *out,
                          void *stream) {
    if (!sp_decode_ok(sh_degree, P_out, chunks, words, sh, out)) return LARA2DGS_E_INVALID;
    if (P_out == 0) return LARA2DGS_OK;
    hipStream_t s = (hipStream_t)stream;
    const SpOut a = sp_out(out);
#define SP_GO(DEG) \
    L2D_LAUNCH_IN_SCOPE(s, sp_decode_kernel<DEG>, dim3((unsigned)sp_blocks(P_out)), dim3(SP_SPAN), 0, (long long)P_out, chunks, (const uint4 *)words, sh, a)
    SP_BY_DEGREE(sh_degree, SP_GO)
#undef SP_GO
    return LARA2DGS_OK;
}

int lara_splatpack_decode_host(int32_t sh_degree, int64_t P_out, const float *chunks, const uint32_t *words, const uint8_t *sh,
                               float *const *out) {
    if (!sp_decode_ok(sh_degree, P_out, chunks, words, sh, out)) return LARA2DGS_E_INVALID;
    lara_splatpack_host_decode(sh_degree, P_out, chunks, words, sh, out);
    return LARA2DGS_OK;
}

int lara_splatpack_splat_encode(const double *plan, int32_t sh_degree, int64_t P, int64_t P_out, const float *const *in, const int64_t *order,
                                uint32_t *rows, void *stream) {
    if (!plan || !sp_sizes_ok(sh_degree, P, P_out) || !sp_fields_ok((const void *const *)in) || !order || !rows || !sp_aligned16(rows))
        return LARA2DGS_E_INVALID;
    if (P_out == 0) return LARA2DGS_OK;
    hipStream_t s = (hipStream_t)stream;
    const SpIn a = sp_in(in);
    const SpPlan row = sp_plan(plan);
#define SP_GO(DEG)                                                                                                                              \
    L2D_LAUNCH_IN_SCOPE(s, sp_splat_encode_kernel<DEG>, dim3((unsigned)sp_blocks(P_out)), dim3(SP_SPAN), 0, row, (long long)P, (long long)P_out, a, \
                        (const long long *)order, (uint4 *)rows)
    SP_BY_DEGREE(sh_degree, SP_GO)
#undef SP_GO
    return LARA2DGS_OK;
}

int lara_splatpack_splat_encode_host(const double *plan, int32_t sh_degree, int64_t P, int64_t P_out, const float *const *in,
                                     const int64_t *order, uint32_t *rows) {
    if (!plan || !sp_sizes_ok(sh_degree, P, P_out) || !sp_fields_ok((const void *const *)in) || !order || !rows || !sp_aligned16(rows))
        return LARA2DGS_E_INVALID;
    lara_splatpack_host_splat_encode(plan, sh_degree, P, P_out, in, order, rows);
    return LARA2DGS_OK;
}

int lara_splatpack_splat_decode(int64_t P_out, const uint32_t *rows, float *const *out, void *stream) {
    if (!sp_sizes_ok(0, P_out, P_out) || !rows || !sp_aligned16(rows) || !sp_fields_ok((const void *const *)out)) return LARA2DGS_E_INVALID;
    if (P_out == 0) return LARA2DGS_OK;
    L2D_LAUNCH_IN_SCOPE((hipStream_t)stream, sp_splat_decode_kernel, dim3((unsigned)sp_blocks(P_out)), dim3(SP_SPAN), 0, (long long)P_out,
                        (const uint4 *)rows, sp_out(out));
    return LARA2DGS_OK;
}

int lara_splatpack_splat_decode_host(int64_t P_out, const uint32_t *rows, float *const *out) {
    if (!sp_sizes_ok(0, P_out, P_out) || !rows || !sp_aligned16(rows) || !sp_fields_ok((const void *const *)out)) return LARA2DGS_E_INVALID;
    lara_splatpack_host_splat_decode(P_out, rows, out);
    return LARA2DGS_OK;
}

}  // extern "C"
