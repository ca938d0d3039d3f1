// splatadam.hip -- one Adam step over the five tensors of a cloud of surfels (centres, SH coefficients, opacity, scales, quaternions)
// in ONE streaming kernel, with the visibility gate, the non-finite gate and the gradient zeroing of lara_splatadam.h.  Interface, the
// plan's layout and the operation order: lara_splatadam.h; the per-word function, shared with the host entry: splatadam_ops.h.
//
//   sa_step_kernel<DEG>     one thread per fp32 word, one workgroup of 256 threads per 256 consecutive words of ONE field.  The five
//                           fields are five segments of the grid: `first[f]` in the kernel's arguments is the field's first
//                           workgroup, so the field is a wave-uniform value found by four scalar compares, its four base pointers and
//                           its word count are scalar loads at constant offsets (the switch below, not an indexed read of the
//                           argument block), and its width is a compile-time constant (the surfel of a word is idx / width for the
//                           `visible` byte, the remainder picks the SH rate).  Lane i and lane i + 1 touch consecutive words of p, g,
//                           m and v: every access is 256 contiguous bytes per wave.  7 words move per parameter word (4 read, 3
//                           written), 8 with zero_grads.  The arithmetic is double (two divisions and a square root per word).
//                           The plan's 13 doubles arrive by value in the kernel's arguments.  The skipped count is one ballot per
//                           wave and one 64-bit integer atomic by the wave's first lane where the ballot is not empty.
#include "common.h"
#include "splatadam_ops.h"
#include "../../include/lara_splatadam.h"

namespace {

constexpr int SA_SPAN = LARA_SPLATADAM_SPAN;
constexpr int SA_F = LARA_SURFEL_FIELDS;
static_assert(SA_SPAN == 256 && SA_SPAN % 64 == 0, "whole waves");

struct SaArgs {
    double plan[LARA_SPLATADAM_PLAN];
    float *p[SA_F], *g[SA_F], *m[SA_F], *v[SA_F];
    long long words[SA_F];                   // fp32 words of each field
    unsigned first[SA_F + 1];                // the first workgroup of each field; first[5] is the grid
};

template <int F, int W>
__device__ __forceinline__ void sa_field(const SaArgs &a, const uint8_t *visible, const int zero_grads, unsigned long long *skipped) {
    const long long i = (long long)(blockIdx.x - a.first[F]) * SA_SPAN + threadIdx.x;
    int bad = 0;
    if (i < a.words[F]) {
        const long long s = i / W;
        const long long r = i - s * W;
        if (visible && !visible[s]) {
            if (zero_grads) a.g[F][i] = 0.0f;
        } else {
            bad = lara_splatadam_word(a.plan, lara_splatadam_rate(a.plan, F, r), a.p[F] + i, a.g[F] + i, a.m[F] + i, a.v[F] + i, zero_grads);
        }
    }
    const unsigned long long lanes = __ballot(bad);          // (every lane of the wave is here: nothing above returns)
    if (lanes != 0ull && (threadIdx.x & 63) == 0) atomicAdd(skipped, (unsigned long long)__popcll(lanes));
}

template <int DEG>
__global__ void __launch_bounds__(SA_SPAN)
sa_step_kernel(const SaArgs a, const uint8_t *visible, const int zero_grads, unsigned long long *skipped) {
    const unsigned b = blockIdx.x;
    int f = 0;
#pragma unroll
    for (int k = 1; k < SA_F; ++k) f += b >= a.first[k] ? 1 : 0;
    switch (f) {
    case 0: sa_field<0, 3>(a, visible, zero_grads, skipped); break;
    case 1: sa_field<1, 3 * (DEG + 1) * (DEG + 1)>(a, visible, zero_grads, skipped); break;
    case 2: sa_field<2, 1>(a, visible, zero_grads, skipped); break;
    case 3: sa_field<3, 2>(a, visible, zero_grads, skipped); break;
    default: sa_field<4, 4>(a, visible, zero_grads, skipped); break;
    }
}

bool sa_args_ok(const double *plan, const int32_t sh_degree, const int64_t P, const void *const *ptrs, const int64_t *skipped) {
    if (!plan || !skipped || sh_degree < 0 || sh_degree > 3 || P < 0 || P > ((int64_t)1 << 40)) return false;
    for (int i = 0; i < 4 * SA_F; ++i)
        if (!ptrs[i]) return false;
    return true;
}

}  // namespace

extern "C" {

int lara_splatadam_step(const double *plan, int32_t sh_degree, int64_t P, float *centers, float *shs, float *opacity, float *scales,
                        float *rotations, float *g_centers, float *g_shs, float *g_opacity, float *g_scales, float *g_rotations,
                        float *m_centers, float *m_shs, float *m_opacity, float *m_scales, float *m_rotations, float *v_centers,
                        float *v_shs, float *v_opacity, float *v_scales, float *v_rotations, const uint8_t *visible, int32_t zero_grads,
                        int64_t *skipped, void *stream) {
    float *const ptrs[4 * SA_F] = {centers,   shs,   opacity,   scales,   rotations,   g_centers, g_shs, g_opacity, g_scales, g_rotations,
                                   m_centers, m_shs, m_opacity, m_scales, m_rotations, v_centers, v_shs, v_opacity, v_scales, v_rotations};
    if (!sa_args_ok(plan, sh_degree, P, (const void *const *)ptrs, skipped)) return LARA2DGS_E_INVALID;
    if (P == 0) return LARA2DGS_OK;
    SaArgs a;
    for (int i = 0; i < LARA_SPLATADAM_PLAN; ++i) a.plan[i] = plan[i];
    for (int f = 0; f < SA_F; ++f) a.p[f] = ptrs[f], a.g[f] = ptrs[SA_F + f], a.m[f] = ptrs[2 * SA_F + f], a.v[f] = ptrs[3 * SA_F + f];
    if (!lara_surfel_grid(P, sh_degree, SA_SPAN, a.words, a.first)) return LARA2DGS_E_INVALID;
#define SA_GO(DEG)                                                                                                             \
    L2D_LAUNCH_IN_SCOPE((hipStream_t)stream, sa_step_kernel<DEG>, dim3(a.first[SA_F]), dim3(SA_SPAN), 0, a, visible, (int)zero_grads, \
                        (unsigned long long *)skipped)
    switch (sh_degree) {
    case 0: SA_GO(0); break;
    case 1: SA_GO(1); break;
    case 2: SA_GO(2); break;
    default: SA_GO(3); break;
    }
#undef SA_GO
    return LARA2DGS_OK;
}

int lara_splatadam_step_host(const double *plan, int32_t sh_degree, int64_t P, float *centers, float *shs, float *opacity, float *scales,
                             float *rotations, float *g_centers, float *g_shs, float *g_opacity, float *g_scales, float *g_rotations,
                             float *m_centers, float *m_shs, float *m_opacity, float *m_scales, float *m_rotations, float *v_centers,
                             float *v_shs, float *v_opacity, float *v_scales, float *v_rotations, const uint8_t *visible,
                             int32_t zero_grads, int64_t *skipped) {
    float *const ptrs[4 * SA_F] = {centers,   shs,   opacity,   scales,   rotations,   g_centers, g_shs, g_opacity, g_scales, g_rotations,
                                   m_centers, m_shs, m_opacity, m_scales, m_rotations, v_centers, v_shs, v_opacity, v_scales, v_rotations};
    if (!sa_args_ok(plan, sh_degree, P, (const void *const *)ptrs, skipped)) return LARA2DGS_E_INVALID;
    *skipped += lara_splatadam_host_words(plan, sh_degree, P, ptrs, ptrs + SA_F, ptrs + 2 * SA_F, ptrs + 3 * SA_F, visible, zero_grads);
    return LARA2DGS_OK;
}

}  // extern "C"
