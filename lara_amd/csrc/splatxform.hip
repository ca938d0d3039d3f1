// splatxform.hip -- a similarity applied to a cloud of surfels: centres, SH coefficients (bands 1..3 rotated in the rasteriser's basis),
// log scales and quaternions, in ONE streaming kernel.  Interface, the plan's layout and the operation order: lara_splatxform.h;
// the per-surfel function, shared with the host entry: splatxform_ops.h.
//
//   sx_apply_kernel<DEG>    one workgroup of 256 threads per span of 256 surfels.  The rows are array-of-structures with strides of
//                           12, 12 n, 4, 8 and 16 bytes, so a thread that loaded its own row would stride through memory; instead the
//                           workgroup moves each array's span as the contiguous bytes it is: 16-byte loads from the first 16-byte
//                           boundary on, lane i next to lane i + 1, single words before it and after the last whole vector (a span
//                           may start at any 4-byte address: out_row0, a tensor view).  In LDS a row of W words lies at a stride of
//                           W | 1 words, so the 32 lanes of a half wave that walk their rows word by word hit 32 banks.  Every
//                           thread transforms its row where it lies (splatxform_ops.h writes a group of outputs after it has read
//                           the group's inputs), and the span goes back as it came.  The span is read completely before the first
//                           store (two barriers), and no workgroup touches another's span: in place is safe.
//                           The plan's 100 doubles arrive by value in the kernel's arguments; every index into them is a
//                           compile-time constant after unrolling, so they are scalar loads, not a table in memory.
#include "common.h"
#include "splatxform_ops.h"
#include "../../include/lara_splatxform.h"

namespace {

constexpr int SX_SPAN = LARA_SPLATXFORM_SPAN;
static_assert(SX_SPAN == 256, "one thread per row of the span");

struct SxPlan { double v[LARA_SPLATXFORM_PLAN]; };

// where word w of a span of rows of W words lies in an LDS image with a row stride of S words
template <int W, int S>
__device__ __forceinline__ int sx_at(const int w) {
    return S == W ? w : (w / W) * S + (w % W);
}

// the n words at g -> the LDS image; g is 4-byte aligned, n <= 256 W
template <int W, int S>
__device__ __forceinline__ void sx_load(const float *g, const int n, float *image) {
    const int lead = (int)((4u - (unsigned)(((uintptr_t)g >> 2) & 3u)) & 3u);        // words before the first 16-byte boundary
    const int head = lead < n ? lead : n;
    const int nvec = (n - head) >> 2;
    const float4 *gv = (const float4 *)(g + head);
    for (int v = threadIdx.x; v < nvec; v += SX_SPAN) {
        const float4 x = gv[v];
        const int w = head + 4 * v;
        image[sx_at<W, S>(w)] = x.x;
        image[sx_at<W, S>(w + 1)] = x.y;
        image[sx_at<W, S>(w + 2)] = x.z;
        image[sx_at<W, S>(w + 3)] = x.w;
    }
    const int tail0 = head + 4 * nvec, singles = head + (n - tail0);               // at most 3 + 3 single words
    if ((int)threadIdx.x < singles) {
        const int w = (int)threadIdx.x < head ? (int)threadIdx.x : tail0 + ((int)threadIdx.x - head);
        image[sx_at<W, S>(w)] = g[w];
    }
}

// the LDS image -> the n words at g
template <int W, int S>
__device__ __forceinline__ void sx_store(float *g, const int n, const float *image) {
    const int lead = (int)((4u - (unsigned)(((uintptr_t)g >> 2) & 3u)) & 3u);
    const int head = lead < n ? lead : n;
    const int nvec = (n - head) >> 2;
    float4 *gv = (float4 *)(g + head);
    for (int v = threadIdx.x; v < nvec; v += SX_SPAN) {
        const int w = head + 4 * v;
        float4 x;
        x.x = image[sx_at<W, S>(w)];
        x.y = image[sx_at<W, S>(w + 1)];
        x.z = image[sx_at<W, S>(w + 2)];
        x.w = image[sx_at<W, S>(w + 3)];
        gv[v] = x;
    }
    const int tail0 = head + 4 * nvec, singles = head + (n - tail0);
    if ((int)threadIdx.x < singles) {
        const int w = (int)threadIdx.x < head ? (int)threadIdx.x : tail0 + ((int)threadIdx.x - head);
        g[w] = image[sx_at<W, S>(w)];
    }
}

// (the inputs and the outputs may be the same arrays: no __restrict__)
template <int DEG>
__global__ void __launch_bounds__(SX_SPAN)
sx_apply_kernel(const SxPlan plan, const long long P, const float *centers, const float *shs, const float *opacity, const float *scales,
                const float *rotations, float *out_centers, float *out_shs, float *out_opacity, float *out_scales, float *out_rotations,
                const long long out_row0) {
    constexpr int WS = 3 * (DEG + 1) * (DEG + 1);
    constexpr int SC = 3, SS = WS | 1, SO = 1, SK = 3, SQ = 5;                     // row strides in LDS, words
    __shared__ float image[SX_SPAN * (SC + SS + SO + SK + SQ)];
    float *const ic = image, *const is = ic + SX_SPAN * SC, *const io = is + SX_SPAN * SS, *const ik = io + SX_SPAN * SO,
                 *const iq = ik + SX_SPAN * SK;
    const long long row0 = (long long)blockIdx.x * SX_SPAN;
    const long long left = P - row0;
    if (left <= 0) return;
    const int rows = left < SX_SPAN ? (int)left : SX_SPAN;
    sx_load<3, SC>(centers + 3 * row0, 3 * rows, ic);
    sx_load<WS, SS>(shs + WS * row0, WS * rows, is);
    sx_load<1, SO>(opacity + row0, rows, io);
    sx_load<2, SK>(scales + 2 * row0, 2 * rows, ik);
    sx_load<4, SQ>(rotations + 4 * row0, 4 * rows, iq);
    __syncthreads();
    const int t = threadIdx.x;
    if (t < rows)
        lara_splatxform_surfel<DEG>(plan.v, ic + SC * t, is + SS * t, io + SO * t, ik + SK * t, iq + SQ * t, ic + SC * t, is + SS * t,
                                    io + SO * t, ik + SK * t, iq + SQ * t);
    __syncthreads();
    const long long o = out_row0 + row0;
    sx_store<3, SC>(out_centers + 3 * o, 3 * rows, ic);
    sx_store<WS, SS>(out_shs + WS * o, WS * rows, is);
    sx_store<1, SO>(out_opacity + o, rows, io);
    sx_store<2, SK>(out_scales + 2 * o, 2 * rows, ik);
    sx_store<4, SQ>(out_rotations + 4 * o, 4 * rows, iq);
}

bool sx_args_ok(const double *plan, const int32_t sh_degree, const int64_t P, const void *const *ptrs, const int64_t out_row0,
                const int64_t out_rows) {
    if (!plan || sh_degree < 0 || sh_degree > 3 || P < 0 || out_row0 < 0 || out_rows < 0 || P > out_rows || out_row0 > out_rows - P)
        return false;
    for (int i = 0; i < 10; ++i)
        if (!ptrs[i]) return false;
    return true;
}

}  // namespace

extern "C" {

int lara_splatxform_apply(const double *plan, int32_t sh_degree, int64_t P, const float *centers, const float *shs, const float *opacity,
                          const float *scales, const float *rotations, float *out_centers, float *out_shs, float *out_opacity,
                          float *out_scales, float *out_rotations, int64_t out_row0, int64_t out_rows, void *stream) {
    const void *const ptrs[10] = {centers, shs, opacity, scales, rotations, out_centers, out_shs, out_opacity, out_scales, out_rotations};
    if (!sx_args_ok(plan, sh_degree, P, ptrs, out_row0, out_rows)) return LARA2DGS_E_INVALID;
    if (P == 0) return LARA2DGS_OK;
    const int64_t blocks = (P + SX_SPAN - 1) / SX_SPAN;
    if (blocks > 0x7fffffffll) return LARA2DGS_E_INVALID;
    SxPlan pl;
    for (int i = 0; i < LARA_SPLATXFORM_PLAN; ++i) pl.v[i] = plan[i];
#define SX_GO(DEG)                                                                                                                      \
    L2D_LAUNCH_IN_SCOPE((hipStream_t)stream, sx_apply_kernel<DEG>, dim3((unsigned)blocks), dim3(SX_SPAN), 0, pl, (long long)P, centers, \
                        shs, opacity, scales, rotations, out_centers, out_shs, out_opacity, out_scales, out_rotations,                 \
                        (long long)out_row0)
    switch (sh_degree) {
    case 0: SX_GO(0); break;
    case 1: SX_GO(1); break;
    case 2: SX_GO(2); break;
    default: SX_GO(3); break;
    }
#undef SX_GO
    return LARA2DGS_OK;
}

int lara_splatxform_apply_host(const double *plan, int32_t sh_degree, int64_t P, const float *centers, const float *shs,
                               const float *opacity, const float *scales, const float *rotations, float *out_centers, float *out_shs,
                               float *out_opacity, float *out_scales, float *out_rotations, int64_t out_row0, int64_t out_rows) {
    const void *const ptrs[10] = {centers, shs, opacity, scales, rotations, out_centers, out_shs, out_opacity, out_scales, out_rotations};
    if (!sx_args_ok(plan, sh_degree, P, ptrs, out_row0, out_rows)) return LARA2DGS_E_INVALID;
    lara_splatxform_host_rows(plan, sh_degree, P, centers, shs, opacity, scales, rotations, out_centers, out_shs, out_opacity, out_scales,
                              out_rotations, out_row0);
    return LARA2DGS_OK;
}

}  // extern "C"
