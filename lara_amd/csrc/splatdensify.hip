// splatdensify.hip -- one densification round of a cloud of surfels under refinement: the statistics of a render call, the action of
// every surfel (keep, clone, split, prune) with the offsets of its output rows, and the new cloud with its Adam moments.  Interface, the
// plan's layout, the rules and the output order: lara_splatdensify.h; the per-row functions, shared with the host entries:
// splatdensify_ops.h.
//
//   sd_accumulate_kernel    one thread per surfel: its V radii (lane i and lane i + 1 read consecutive words of every view's row), its
//                           gradient row, its three statistics.
//   sd_decide_kernel        one thread per surfel: the action byte and the surfel's three flags, stored into `offset` at s, P + s and
//                           2 P + s.  The plan's 8 doubles arrive by value in the kernel's arguments.
//   mm_scan (unigrid.h)     the three-launch inclusive scan of the 3 P flags into the workspace: no wave waits for another wave.
//   sd_finish_kernel        one thread per flag: offset <- inclusive - flag, the exclusive scan; the thread of flag 0 reads the three
//                           segment ends and stores the five counts.
//   sd_rows_kernel          one thread per source surfel: row_source and row_child of its output rows, through `offset`.
//   sd_gather_kernel<DEG>   one thread per output word of a parameter, 256 words of ONE field per workgroup, the field found from a
//                           table of block offsets in the kernel's arguments as in splatadam.hip; the thread stores the parameter word
//                           and its two moment words.  Lanes of a wave store consecutive words; they read consecutive words wherever
//                           consecutive output rows have consecutive sources (every run of kept rows).
#include "common.h"
#include "unigrid.h"
#include "splatdensify_ops.h"
#include "../../include/lara_splatdensify.h"

namespace {

constexpr int SD_SPAN = LARA_SPLATDENSIFY_SPAN;
constexpr int SD_F = LARA_SURFEL_FIELDS;
constexpr int64_t SD_MAX_P = (int64_t)1 << 27;       // 9 P (a survivor and 8 children each) stays inside int32
static_assert(SD_SPAN == 256 && SD_SPAN % 64 == 0, "whole waves");

struct SdPlan {
    double v[LARA_SPLATDENSIFY_PLAN];
};

struct SdGather {
    double plan[LARA_SPLATDENSIFY_PLAN];
    const float *in[3 * SD_F];
    float *out[3 * SD_F];
    long long words[SD_F];                   // fp32 words of each field of the OUTPUT cloud
    unsigned first[SD_F + 1];                // the first workgroup of each field; first[5] is the grid
    long long P, P_out, survivors;
    const int32_t *row_source;
    const uint8_t *row_child;
    const float *noise;
    int n_split;
};

__global__ void __launch_bounds__(SD_SPAN)
sd_accumulate_kernel(const long long P, const int V, const float *__restrict__ grad, const int32_t *__restrict__ radii, float *grad_sum,
                     int32_t *seen, int32_t *max_radius) {
    const long long s = (long long)blockIdx.x * SD_SPAN + threadIdx.x;
    if (s >= P) return;
    lara_splatdensify_accumulate_row(P, V, s, grad + 3 * s, radii, grad_sum + s, seen + s, max_radius + s);
}

__global__ void __launch_bounds__(SD_SPAN)
sd_decide_kernel(const SdPlan plan, const long long P, const float *__restrict__ opacity, const float *__restrict__ scales,
                 const float *__restrict__ grad_sum, const int32_t *__restrict__ seen, const int32_t *__restrict__ max_radius,
                 uint8_t *__restrict__ action, int32_t *__restrict__ flags) {
    const long long s = (long long)blockIdx.x * SD_SPAN + threadIdx.x;
    if (s >= P) return;
    const int a = lara_splatdensify_action(plan.v, opacity[s], scales[2 * s], scales[2 * s + 1], grad_sum[s], seen[s], max_radius[s]);
    action[s] = (uint8_t)a;
    lara_splatdensify_flags(a, lara_splatdensify_children(plan.v), flags + s, flags + P + s, flags + 2 * P + s);
}

__global__ void __launch_bounds__(SD_SPAN)
sd_finish_kernel(const long long P, const int n_split, const int32_t *__restrict__ incl, int32_t *__restrict__ offset,
                 long long *__restrict__ counts) {
    const long long i = (long long)blockIdx.x * SD_SPAN + threadIdx.x;
    if (i >= 3 * P) return;
    offset[i] = incl[i] - offset[i];
    if (i == 0) {
        const long long a = incl[P - 1], b = incl[2 * P - 1], c = incl[3 * P - 1];
        int64_t five[5];
        lara_splatdensify_counts(P, n_split, a, b - a, c - b, five);
#pragma unroll
        for (int k = 0; k < 5; ++k) counts[k] = five[k];
    }
}

__global__ void __launch_bounds__(SD_SPAN)
sd_rows_kernel(const long long P, const int n_split, const uint8_t *__restrict__ action, const int32_t *__restrict__ offset,
               const long long P_out, int32_t *__restrict__ row_source, uint8_t *__restrict__ row_child) {
    const long long s = (long long)blockIdx.x * SD_SPAN + threadIdx.x;
    if (s >= P) return;
    lara_splatdensify_rows_of(P, n_split, s, action[s], offset, P_out, row_source, row_child);
}

template <int F, int W>
__device__ __forceinline__ void sd_field(const SdGather &a) {
    const long long i = (long long)(blockIdx.x - a.first[F]) * SD_SPAN + threadIdx.x;
    if (i >= a.words[F]) return;
    const long long o = i / W;
    const float *const in[3] = {a.in[F], a.in[SD_F + F], a.in[2 * SD_F + F]};
    float *const out[3] = {a.out[F], a.out[SD_F + F], a.out[2 * SD_F + F]};
    lara_splatdensify_word(a.plan, F, W, o, i - o * W, a.P, a.survivors, a.n_split, a.row_source, a.row_child, a.noise, a.in[0], a.in[3], a.in[4],
                           in, out);
}

template <int DEG>
__global__ void __launch_bounds__(SD_SPAN)
sd_gather_kernel(const SdGather a) {
    const unsigned b = blockIdx.x;
    int f = 0;
#pragma unroll
    for (int k = 1; k < SD_F; ++k) f += b >= a.first[k] ? 1 : 0;
    switch (f) {
    case 0: sd_field<0, 3>(a); break;
    case 1: sd_field<1, 3 * (DEG + 1) * (DEG + 1)>(a); break;
    case 2: sd_field<2, 1>(a); break;
    case 3: sd_field<3, 2>(a); break;
    default: sd_field<4, 4>(a); break;
    }
}

unsigned sd_blocks(const int64_t n) { return (unsigned)((n + SD_SPAN - 1) / SD_SPAN); }

bool sd_plan_ok(const double *plan) {
    if (!plan) return false;
    const double n = plan[LARA_SPLATDENSIFY_N], f = plan[LARA_SPLATDENSIFY_FLAGS];
    return n >= 1.0 && n <= 8.0 && n == (double)(int)n && f >= 0.0 && f <= 7.0 && f == (double)(int)f;
}

bool sd_accumulate_ok(const int64_t P, const int32_t V, const void *grad, const void *radii, const void *grad_sum, const void *seen,
                      const void *max_radius) {
    return P >= 0 && P <= SD_MAX_P && V >= 1 && V <= 4096 && grad && radii && grad_sum && seen && max_radius;
}

bool sd_decide_ok(const double *plan, const int64_t P, const void *const *ptrs, const int n) {
    if (!sd_plan_ok(plan) || P < 0 || P > SD_MAX_P) return false;
    for (int i = 0; i < n; ++i)
        if (!ptrs[i]) return false;
    return true;
}

bool sd_apply_ok(const double *plan, const int32_t sh_degree, const int64_t P, const int64_t P_out, const int64_t survivors,
                 const void *const *ptrs, const int n) {
    if (!sd_plan_ok(plan) || sh_degree < 0 || sh_degree > 3 || P < 0 || P > SD_MAX_P) return false;
    if (P_out < 0 || P_out > 9 * P || survivors < 0 || survivors > P_out || survivors > P) return false;
    for (int i = 0; i < n; ++i)
        if (!ptrs[i]) return false;
    return true;
}

}  // namespace

extern "C" {

int lara_splatdensify_accumulate(int64_t P, int32_t V, const float *grad_means2D, const int32_t *radii, float *grad_sum, int32_t *seen,
                                 int32_t *max_radius, void *stream) {
    if (!sd_accumulate_ok(P, V, grad_means2D, radii, grad_sum, seen, max_radius)) return LARA2DGS_E_INVALID;
    if (P == 0) return LARA2DGS_OK;
    L2D_LAUNCH_IN_SCOPE((hipStream_t)stream, sd_accumulate_kernel, dim3(sd_blocks(P)), dim3(SD_SPAN), 0, (long long)P, (int)V, grad_means2D,
                        radii, grad_sum, seen, max_radius);
    return LARA2DGS_OK;
}

int lara_splatdensify_accumulate_host(int64_t P, int32_t V, const float *grad_means2D, const int32_t *radii, float *grad_sum, int32_t *seen,
                                      int32_t *max_radius) {
    if (!sd_accumulate_ok(P, V, grad_means2D, radii, grad_sum, seen, max_radius)) return LARA2DGS_E_INVALID;
    lara_splatdensify_host_accumulate(P, V, grad_means2D, radii, grad_sum, seen, max_radius);
    return LARA2DGS_OK;
}

int64_t lara_splatdensify_workspace_bytes(int64_t P) {
    if (P < 0 || P > SD_MAX_P) return LARA2DGS_E_INVALID;
    const int64_t n = 3 * P, nb = (n + MM_SCAN_BLOCK - 1) / MM_SCAN_BLOCK;
    return (n + nb + 64) * (int64_t)sizeof(int32_t);
}

int lara_splatdensify_decide(const double *plan, int64_t P, const float *opacity, const float *scales, const float *grad_sum,
                             const int32_t *seen, const int32_t *max_radius, uint8_t *action, int32_t *offset, int64_t *counts,
                             void *workspace, void *stream) {
    const void *const ptrs[] = {opacity, scales, grad_sum, seen, max_radius, action, offset, counts, workspace};
    if (!sd_decide_ok(plan, P, ptrs, 9)) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    if (P == 0) {
        L2D_HIP(hipMemsetAsync(counts, 0, 5 * sizeof(int64_t), s));
        return LARA2DGS_OK;
    }
    SdPlan row;
    for (int i = 0; i < LARA_SPLATDENSIFY_PLAN; ++i) row.v[i] = plan[i];
    int32_t *incl = (int32_t *)workspace, *bsum = incl + 3 * P;
    L2D_LAUNCH_IN_SCOPE(s, sd_decide_kernel, dim3(sd_blocks(P)), dim3(SD_SPAN), 0, row, (long long)P, opacity, scales, grad_sum, seen, max_radius,
                        action, offset);
    L2D_TRY(mm_scan<int32_t>((const int32_t *)offset, incl, bsum, (long long)(3 * P), s));
    L2D_LAUNCH_IN_SCOPE(s, sd_finish_kernel, dim3(sd_blocks(3 * P)), dim3(SD_SPAN), 0, (long long)P, lara_splatdensify_children(plan),
                        (const int32_t *)incl, offset, (long long *)counts);
    return LARA2DGS_OK;
}

int lara_splatdensify_decide_host(const double *plan, int64_t P, const float *opacity, const float *scales, const float *grad_sum,
                                  const int32_t *seen, const int32_t *max_radius, uint8_t *action, int32_t *offset, int64_t *counts,
                                  void *workspace) {
    const void *const ptrs[] = {opacity, scales, grad_sum, seen, max_radius, action, offset, counts};      // (the workspace is not used here)
    (void)workspace;
    if (!sd_decide_ok(plan, P, ptrs, 8)) return LARA2DGS_E_INVALID;
    lara_splatdensify_host_decide(plan, P, opacity, scales, grad_sum, seen, max_radius, action, offset, counts);
    return LARA2DGS_OK;
}

int lara_splatdensify_apply(const double *plan, int32_t sh_degree, int64_t P, int64_t P_out, int64_t survivors, const uint8_t *action,
                            const int32_t *offset, const float *noise, const float *const *in, float *const *out, int32_t *row_source,
                            uint8_t *row_child, void *stream) {
    if (!in || !out) return LARA2DGS_E_INVALID;
    const void *ptrs[5 + 6 * SD_F] = {action, offset, noise, row_source, row_child};
    for (int i = 0; i < 3 * SD_F; ++i) ptrs[5 + i] = in[i], ptrs[5 + 3 * SD_F + i] = out[i];
    if (!sd_apply_ok(plan, sh_degree, P, P_out, survivors, ptrs, 5 + 6 * SD_F)) return LARA2DGS_E_INVALID;
    if (P == 0 || P_out == 0) return LARA2DGS_OK;
    hipStream_t s = (hipStream_t)stream;
    SdGather a;
    for (int i = 0; i < LARA_SPLATDENSIFY_PLAN; ++i) a.plan[i] = plan[i];
    for (int i = 0; i < 3 * SD_F; ++i) a.in[i] = in[i], a.out[i] = out[i];
    if (!lara_surfel_grid(P_out, sh_degree, SD_SPAN, a.words, a.first)) return LARA2DGS_E_INVALID;
    a.P = P, a.P_out = P_out, a.survivors = survivors;
    a.row_source = row_source, a.row_child = row_child, a.noise = noise;
    a.n_split = lara_splatdensify_children(plan);
    L2D_LAUNCH_IN_SCOPE(s, sd_rows_kernel, dim3(sd_blocks(P)), dim3(SD_SPAN), 0, (long long)P, a.n_split, action, offset, (long long)P_out,
                        row_source, row_child);
#define SD_GO(DEG) L2D_LAUNCH_IN_SCOPE(s, sd_gather_kernel<DEG>, dim3(a.first[SD_F]), dim3(SD_SPAN), 0, a)
    switch (sh_degree) {
    case 0: SD_GO(0); break;
    case 1: SD_GO(1); break;
    case 2: SD_GO(2); break;
    default: SD_GO(3); break;
    }
#undef SD_GO
    return LARA2DGS_OK;
}

int lara_splatdensify_apply_host(const double *plan, int32_t sh_degree, int64_t P, int64_t P_out, int64_t survivors, const uint8_t *action,
                                 const int32_t *offset, const float *noise, const float *const *in, float *const *out, int32_t *row_source,
                                 uint8_t *row_child) {
    if (!in || !out) return LARA2DGS_E_INVALID;
    const void *ptrs[5 + 6 * SD_F] = {action, offset, noise, row_source, row_child};
    for (int i = 0; i < 3 * SD_F; ++i) ptrs[5 + i] = in[i], ptrs[5 + 3 * SD_F + i] = out[i];
    if (!sd_apply_ok(plan, sh_degree, P, P_out, survivors, ptrs, 5 + 6 * SD_F)) return LARA2DGS_E_INVALID;
    if (P == 0 || P_out == 0) return LARA2DGS_OK;
    lara_splatdensify_host_apply(plan, sh_degree, P, P_out, survivors, action, offset, noise, in, out, row_source, row_child);
    return LARA2DGS_OK;
}

}  // extern "C"
