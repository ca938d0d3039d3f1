// vit.hip -- the DINO ViT image encoder (lightning/network.py:14-55 DinoWrapper: timm vit_base_patch16_224.dino, dynamic_img_size)
// as it runs under bf16 autocast, forward and backward.  include/lara_vit.h has the formulas and the contract.
//
// Forward:  patch_kernel (normalise, bf16 patch rows in the conv weight's (ch, ky, kx) order) -> lara_gemm_nt_bf16 -> tokens_kernel
//           ([cls | patches] + pos into the fp32 residual stream); per block: ln_fwd_kernel (bf16 rows) -> qkv product ->
//           qkv_split_kernel (bias, bf16, head-major q / k / v) -> attn_fwd_kernel (flash style, one wave per 16 queries) -> proj
//           product -> residual_kernel; ln_fwd_kernel -> fc1 product -> fc1_kernel (bias, bf16, erf GELU) -> fc2 product ->
//           residual_kernel; the final LayerNorm writes the fp32 patch tokens.
// Backward: the same products transposed (lara_gemm_nt_bf16 on per-call transposed bf16 weights for the input gradients,
//           lara_gemm_tn_bf16 for the weight gradients), fixed-order column sums for the biases, ln_bwd_kernel with per-block
//           gamma / beta partials added in block order, attn_dkv_kernel / attn_dq_kernel.  No float atomics anywhere.
//
// Attention tiles (mfma_f32_16x16x32_bf16; lane l, g = l >> 4): a wave holds S^T = K Q^T for 32 keys x 16 queries as two 16 x 16
// accumulators, so every lane owns one query column (l & 15) and 8 keys {4g + r, 16 + 4g + r}.  Those 8 values, rounded to bf16,
// are directly the B operand of O^T += V^T P^T when the A operand (V^T, read from a head-major transposed copy) takes its 8 k
// elements in the same permuted key order.  The softmax statistics of a query live in the 4 lanes l & 15 + 16 g' (two xor shuffles).
// The key-side backward is the mirror image: S = Q K^T with the key on the lane.
#include <algorithm>

#include "common.h"
#include "mfma_gemm.h"
#include "../../include/lara_vit.h"
#include "../../include/lara_groupattn.h"

namespace {

constexpr int VT_HD = 64;          // head width
constexpr int VT_PD = 768;         // 3 x 16 x 16 patch row
constexpr int VT_LNB = 256;        // ln_bwd_kernel blocks (gamma / beta partial rows)
constexpr int VT_CSP = 64;         // column-sum partial rows

inline int rup(int v, int m) { return (v + m - 1) / m * m; }

__device__ __forceinline__ bf16x8 as_frag(const uint4 u) {
    bf16x8 f;
    __builtin_memcpy(&f, &u, 16);
    return f;
}
__device__ __forceinline__ bf16x8 frag_2x4(const uint2 a, const uint2 b) {   // elements 0..3 from a, 4..7 from b
    return as_frag(make_uint4(a.x, a.y, b.x, b.y));
}
__device__ __forceinline__ bf16x8 frag_acc(const f32x4 a, const f32x4 b) {   // two accumulators, rounded, as one 8-element operand
    return as_frag(make_uint4(f2bf2(a[0], a[1]), f2bf2(a[2], a[3]), f2bf2(b[0], b[1]), f2bf2(b[2], b[3])));
}
__device__ __forceinline__ f32x4 mfma16(const bf16x8 a, const bf16x8 b, const f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
// ---------------------------------------------------------------------------------------------------------------------------
// weights: bf16 copy (row-major as given) or bf16 transpose
__global__ void __launch_bounds__(256) wcast_kernel(const float *__restrict__ src, const size_t n, unsigned short *__restrict__ dst) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = f2bf(src[i]);
}
// dst[c][r] = bf16(src[r][c]), src [R, Cc]
__global__ void __launch_bounds__(256) wtrans_kernel(const float *__restrict__ src, const int R, const int Cc, unsigned short *__restrict__ dst) {
    __shared__ float tile[32][33];
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int k = ty; k < 32; k += 8)
        if (r0 + k < R && c0 + tx < Cc) tile[k][tx] = src[(size_t)(r0 + k) * Cc + c0 + tx];
    __syncthreads();
    for (int k = ty; k < 32; k += 8)
        if (c0 + k < Cc && r0 + tx < R) dst[(size_t)(c0 + k) * R + r0 + tx] = f2bf(tile[tx][k]);
}

// ---------------------------------------------------------------------------------------------------------------------------
// patch rows: a[p][(ch, ky, kx)] (rows >= NP: zeros).  One thread per pair of kx.
struct PatchP {
    const float *img;
    long long s0, sv, s1, s2, s3;
    int NP, Pp, hw, w, views;
};
__global__ void __launch_bounds__(256) patch_kernel(const PatchP p, unsigned *__restrict__ a) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)p.Pp * (VT_PD / 2)) return;
    const int row = (int)(i / (VT_PD / 2)), e = (int)(i - (size_t)row * (VT_PD / 2)) * 2;
    if (row >= p.NP) { a[i] = 0u; return; }
    const int n = row / p.hw, pp = row - n * p.hw, py = pp / p.w, px = pp - py * p.w;
    const int ch = e >> 8, ky = (e >> 4) & 15, kx = e & 15;
    const float mean = ch == 0 ? 0.485f : ch == 1 ? 0.456f : 0.406f;
    const float sd = ch == 0 ? 0.229f : ch == 1 ? 0.224f : 0.225f;
    const int nb = n / p.views, nv = n - nb * p.views;
    const float *src = p.img + nb * p.s0 + nv * p.sv + ch * p.s1 + (long long)(16 * py + ky) * p.s2 + (long long)(16 * px + kx) * p.s3;
    a[i] = f2bf2((src[0] - mean) / sd, (src[p.s3] - mean) / sd);
}

// x0 rows: t = 0 cls + pos[0]; t = 1 + p: bf16(acc + bf16(b)) + pos[t]
__global__ void __launch_bounds__(256) tokens_kernel(const float *__restrict__ acc, const float *__restrict__ bias,
                                                     const float *__restrict__ cls, const float *__restrict__ pos, const int N,
                                                     const int T, const int C, float *__restrict__ x) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)N * T * C) return;
    const int c = (int)(i % C);
    const size_t r = i / C;
    const int n = (int)(r / T), t = (int)(r - (size_t)n * T);
    const float v = t == 0 ? cls[c] : bfr(acc[((size_t)n * (T - 1) + t - 1) * C + c] + bfr(bias[c]));
    x[i] = v + pos[(size_t)t * C + c];
}

// ---------------------------------------------------------------------------------------------------------------------------
// LayerNorm forward, one wave per row; lane channels c = 4 lane + 256 q (q < 4, valid while c < C).
// FINAL = false: bf16 rows [Mp, C] (rows >= M zeros); FINAL = true: fp32 [N, T - 1, C] (the class tokens dropped).
template <bool FINAL>
__global__ void __launch_bounds__(256) ln_fwd_kernel(const float *__restrict__ x, const float *__restrict__ gam, const float *__restrict__ bet,
                                                     const int M, const int Mp, const int T, const int C, const float eps,
                                                     void *__restrict__ out, float2 *__restrict__ stats) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= Mp) return;
    if (r >= M) {
        if (!FINAL)
            for (int c = 4 * lane; c < C; c += 256) *(uint2 *)((unsigned short *)out + (size_t)r * C + c) = make_uint2(0u, 0u);
        return;
    }
    if (FINAL && r % T == 0) return;
    float v[4][4];
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int c = 4 * lane + 256 * q;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < C) a = *(const float4 *)(x + (size_t)r * C + c);
        v[q][0] = a.x; v[q][1] = a.y; v[q][2] = a.z; v[q][3] = a.w;
        s += (a.x + a.y) + (a.z + a.w);
    }
    const float mean = wave_sum(s) / (float)C;
    float ss = 0.f;
#pragma unroll
    for (int q = 0; q < 4; q++)
        if (4 * lane + 256 * q < C)
#pragma unroll
            for (int i = 0; i < 4; i++) ss += (v[q][i] - mean) * (v[q][i] - mean);
    const float rstd = 1.f / sqrtf(wave_sum(ss) / (float)C + eps);
    if (lane == 0) stats[r] = make_float2(mean, rstd);
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int c = 4 * lane + 256 * q;
        if (c >= C) continue;
        const float4 gg = *(const float4 *)(gam + c), bb = *(const float4 *)(bet + c);
        const float y0 = (v[q][0] - mean) * rstd * gg.x + bb.x, y1 = (v[q][1] - mean) * rstd * gg.y + bb.y;
        const float y2 = (v[q][2] - mean) * rstd * gg.z + bb.z, y3 = (v[q][3] - mean) * rstd * gg.w + bb.w;
        if (FINAL) {
            const int n = r / T, t = r - n * T;
            *(float4 *)((float *)out + ((size_t)n * (T - 1) + t - 1) * C + c) = make_float4(y0, y1, y2, y3);
        } else {
            *(uint2 *)((unsigned short *)out + (size_t)r * C + c) = make_uint2(f2bf2(y0, y1), f2bf2(y2, y3));
        }
    }
}

// LayerNorm backward, one wave per row (rows gw, gw + 4 VT_LNB, ...): dres[r] (+)= dLN(dy);  per-block [dgamma | dbeta] partials.
// DYF = false: dy bf16 [Mp, C] rows, dres += dx;  DYF = true: dy fp32 [N, T - 1, C] (zero for the class tokens), dres = dx.
template <bool DYF>
__global__ void __launch_bounds__(256) ln_bwd_kernel(const void *__restrict__ dyp, const float *__restrict__ x, const float2 *__restrict__ stats,
                                                     const float *__restrict__ gam, const int M, const int T, const int C,
                                                     float *__restrict__ dres, float *__restrict__ part) {
    __shared__ float red[4][2 * LARA_VIT_MAX_C];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float pg[4][4], pb[4][4];
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int i = 0; i < 4; i++) pg[q][i] = pb[q][i] = 0.f;
    for (int r = blockIdx.x * 4 + wave; r < M; r += 4 * VT_LNB) {
        const int t = r % T;
        if (DYF && t == 0) {
            for (int c = 4 * lane; c < C; c += 256) *(float4 *)(dres + (size_t)r * C + c) = make_float4(0.f, 0.f, 0.f, 0.f);
            continue;
        }
        const float2 st = stats[r];
        float xh[4][4], dy[4][4], dxh[4][4];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int c = 4 * lane + 256 * q;
#pragma unroll
            for (int i = 0; i < 4; i++) xh[q][i] = dy[q][i] = dxh[q][i] = 0.f;
            if (c >= C) continue;
            const float4 xv = *(const float4 *)(x + (size_t)r * C + c);
            xh[q][0] = (xv.x - st.x) * st.y; xh[q][1] = (xv.y - st.x) * st.y;
            xh[q][2] = (xv.z - st.x) * st.y; xh[q][3] = (xv.w - st.x) * st.y;
            if (DYF) {
                const int n = r / T;
                const float4 d = *(const float4 *)((const float *)dyp + ((size_t)n * (T - 1) + t - 1) * C + c);
                dy[q][0] = d.x; dy[q][1] = d.y; dy[q][2] = d.z; dy[q][3] = d.w;
            } else {
                const uint2 d = *(const uint2 *)((const unsigned short *)dyp + (size_t)r * C + c);
                dy[q][0] = __uint_as_float(d.x << 16); dy[q][1] = __uint_as_float(d.x & 0xffff0000u);
                dy[q][2] = __uint_as_float(d.y << 16); dy[q][3] = __uint_as_float(d.y & 0xffff0000u);
            }
            const float4 gg = *(const float4 *)(gam + c);
            dxh[q][0] = dy[q][0] * gg.x; dxh[q][1] = dy[q][1] * gg.y; dxh[q][2] = dy[q][2] * gg.z; dxh[q][3] = dy[q][3] * gg.w;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                s1 += dxh[q][i];
                s2 += dxh[q][i] * xh[q][i];
                pg[q][i] += dy[q][i] * xh[q][i];
                pb[q][i] += dy[q][i];
            }
        }
        const float a = wave_sum(s1) / (float)C, b = wave_sum(s2) / (float)C;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int c = 4 * lane + 256 * q;
            if (c >= C) continue;
            float4 o = make_float4(st.y * (dxh[q][0] - a - xh[q][0] * b), st.y * (dxh[q][1] - a - xh[q][1] * b),
                                   st.y * (dxh[q][2] - a - xh[q][2] * b), st.y * (dxh[q][3] - a - xh[q][3] * b));
            float4 *dst = (float4 *)(dres + (size_t)r * C + c);
            if (!DYF) {
                const float4 prev = *dst;
                o.x += prev.x; o.y += prev.y; o.z += prev.z; o.w += prev.w;
            }
            *dst = o;
        }
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int c = 4 * lane + 256 * q;
        if (c >= C) continue;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            red[wave][c + i] = pg[q][i];
            red[wave][C + c + i] = pb[q][i];
        }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < 2 * C; j += 256)
        part[(size_t)blockIdx.x * 2 * C + j] = ((red[0][j] + red[1][j]) + red[2][j]) + red[3][j];
}

// out[i] = sum_k part[k][i] in k order (i < split: out0, else out1)
__global__ void __launch_bounds__(256) sum_parts_kernel(const float *__restrict__ part, const int nparts, const int width,
                                                        float *__restrict__ out0, float *__restrict__ out1, const int split) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= width) return;
    float a = 0.f;
    for (int k = 0; k < nparts; k++) a += part[(size_t)k * width + i];
    if (i < split) out0[i] = a;
    else out1[i - split] = a;
}

// column sums of bf16 rows [rows, ncol]: partial k covers rows [k chunk, (k + 1) chunk)
__global__ void __launch_bounds__(256) colsum_part_kernel(const unsigned short *__restrict__ src, const int rows, const int ncol,
                                                          float *__restrict__ part) {
    const int c = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (c >= ncol) return;
    const int chunk = (rows + VT_CSP - 1) / VT_CSP, r1 = min(rows, (k + 1) * chunk);
    float a = 0.f;
    for (int r = k * chunk; r < r1; r++) a += bf2f(src[(size_t)r * ncol + c]);
    part[(size_t)k * ncol + c] = a;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Linear epilogues
// qkv: bf16(acc + bf16(b)) -> q, k, v [NH, Tp, 64] (t >= T: zeros)
__global__ void __launch_bounds__(256) qkv_split_kernel(const float *__restrict__ acc, const float *__restrict__ bias, const int N,
                                                        const int T, const int Tp, const int C, unsigned short *__restrict__ q,
                                                        unsigned short *__restrict__ k, unsigned short *__restrict__ v) {
    const int heads = C / VT_HD;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, per = (size_t)N * heads * Tp * VT_HD;
    if (i >= 3 * per) return;
    const int which = (int)(i / per);
    const size_t j = i - which * per;
    const int d = (int)(j & 63);
    const size_t rt = j >> 6;
    const int t = (int)(rt % Tp);
    const int nh = (int)(rt / Tp), n = nh / heads, hh = nh - n * heads;
    unsigned short *dst = which == 0 ? q : which == 1 ? k : v;
    if (t >= T) { dst[j] = 0; return; }
    const int col = which * C + hh * VT_HD + d;
    dst[j] = f2bf(acc[((size_t)n * T + t) * 3 * C + col] + bfr(bias[col]));
}

// [NH, Tp, 64] -> [NH, 64, Tp]
__global__ void __launch_bounds__(256) head_t_kernel(const unsigned short *__restrict__ src, const int NH, const int Tp,
                                                     unsigned short *__restrict__ dst) {
    __shared__ unsigned short tile[64][65];
    const int nh = blockIdx.y, t0 = blockIdx.x * 64;
    const unsigned short *s = src + ((size_t)nh * Tp + t0) * VT_HD;
    for (int e = threadIdx.x; e < 64 * 64; e += 256) tile[e >> 6][e & 63] = s[e];   // [t][d]
    __syncthreads();
    unsigned short *o = dst + (size_t)nh * VT_HD * Tp + t0;
    for (int e = threadIdx.x; e < 64 * 64; e += 256) o[(size_t)(e >> 6) * Tp + (e & 63)] = tile[e & 63][e >> 6];
}

// merged bf16 rows [Mp, C] (head h: columns 64 h ..) -> head-major [NH, Tp, 64] (t >= T: zeros)
__global__ void __launch_bounds__(256) head_split_kernel(const unsigned short *__restrict__ src, const int N, const int T, const int Tp,
                                                         const int C, unsigned short *__restrict__ dst) {
    const int heads = C / VT_HD;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)N * heads * Tp * VT_HD) return;
    const int d = (int)(i & 63);
    const size_t rt = i >> 6;
    const int t = (int)(rt % Tp), nh = (int)(rt / Tp), n = nh / heads, hh = nh - n * heads;
    dst[i] = t < T ? src[((size_t)n * T + t) * C + hh * VT_HD + d] : (unsigned short)0;
}

// x_out = x_in + bf16(acc + bf16(b)), rows < M
__global__ void __launch_bounds__(256) residual_kernel(const float *__restrict__ acc, const float *__restrict__ bias, const float *__restrict__ xin,
                                                       const int M, const int C, float *__restrict__ xout) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)M * C) return;
    const int c = (int)(i % C);
    xout[i] = xin[i] + bfr(acc[i] + bfr(bias[c]));
}

__device__ __forceinline__ float gelu_exact(const float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }

// h = bf16(acc + bf16(b)), g = bf16(GELU(h)); rows >= M zeros
__global__ void __launch_bounds__(256) fc1_kernel(const float *__restrict__ acc, const float *__restrict__ bias, const int M, const int Mp,
                                                  const int F, unsigned short *__restrict__ h, unsigned short *__restrict__ g) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)Mp * F) return;
    if (i >= (size_t)M * F) {
        if (h) h[i] = 0;
        g[i] = 0;
        return;
    }
    const float hv = bfr(acc[i] + bfr(bias[i % F]));
    if (h) h[i] = f2bf(hv);
    g[i] = f2bf(gelu_exact(hv));
}

// g = bf16(GELU(h)) (the backward's recomputation of fc2's operand)
__global__ void __launch_bounds__(256) gelu_kernel(const unsigned short *__restrict__ h, const size_t n, unsigned short *__restrict__ g) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) g[i] = f2bf(gelu_exact(bf2f(h[i])));
}

// dh = bf16(dg * GELU'(h)) in place of dg
__global__ void __launch_bounds__(256) gelu_bwd_kernel(const unsigned short *__restrict__ h, const size_t n, unsigned short *__restrict__ dg) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float x = bf2f(h[i]);
    const float cdf = 0.5f * (1.f + erff(x * 0.70710678118654752f));
    const float pdf = expf(-0.5f * x * x) * 0.39894228040143268f;
    dg[i] = f2bf(bf2f(dg[i]) * (cdf + x * pdf));
}

// dy = bf16(dres) rows [Mp, C] (rows >= M zeros)
__global__ void __launch_bounds__(256) rows_bf16_kernel(const float *__restrict__ src, const int M, const int Mp, const int C,
                                                        unsigned short *__restrict__ dst) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)Mp * C) return;
    dst[i] = i < (size_t)M * C ? f2bf(src[i]) : (unsigned short)0;
}

// token-stage backward: dpos[t] = sum_n dres[n, t] (n order), dcls = dpos row 0's sum; dconv bf16 [Pp, C] = bf16(dres[n, 1 + p])
__global__ void __launch_bounds__(256) tokens_bwd_kernel(const float *__restrict__ dres, const int N, const int T, const int C,
                                                         float *__restrict__ dpos, float *__restrict__ dcls) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)T * C) return;
    float a = 0.f;
    for (int n = 0; n < N; n++) a += dres[(size_t)n * T * C + i];
    dpos[i] = a;
    if (i < (size_t)C) dcls[i] = a;
}
__global__ void __launch_bounds__(256) dconv_kernel(const float *__restrict__ dres, const int N, const int T, const int C, const int Pp,
                                                    unsigned short *__restrict__ dconv) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)Pp * C) return;
    const size_t p = i / C;
    const int c = (int)(i - p * C);
    if (p >= (size_t)N * (T - 1)) { dconv[i] = 0; return; }
    const size_t n = p / (T - 1), pp = p - n * (T - 1);
    dconv[i] = f2bf(dres[(n * T + 1 + pp) * C + c]);
}

// ---------------------------------------------------------------------------------------------------------------------------
// attention.  q, k, v, dO: [NH, Tp, 64] bf16; *t: [NH, 64, Tp]; rows t >= T are zeros.  Scale 1/8 (exact).
struct AttnP {
    const unsigned short *q, *k, *v, *qt, *kt, *vt, *doh, *dot;
    const float *lse_in, *dvec;
    unsigned short *o;       // merged [Mp, C] rows (forward)
    float *lse;              // [NH, Tp] (training forward)
    unsigned short *dqkv;    // merged [Mp, 3C] rows (backward)
    int T, Tp, C, heads;
};
constexpr float VT_SCALE = 0.125f;

__device__ __forceinline__ uint4 ld16(const unsigned short *p) { return *(const uint4 *)p; }
__device__ __forceinline__ uint2 ld8(const unsigned short *p) { return *(const uint2 *)p; }

// one wave per 16 queries; blocks of 4 waves (64 queries)
template <bool TRAIN>
__global__ void __launch_bounds__(256) attn_fwd_kernel(const AttnP p) {
    const int lane = threadIdx.x & 63, g = lane >> 4, col = lane & 15;
    const int nh = blockIdx.y, q0 = blockIdx.x * 64 + (threadIdx.x >> 6) * 16;
    if (q0 >= p.T) return;
    const size_t hb = (size_t)nh * p.Tp * VT_HD;
    const unsigned short *Q = p.q + hb, *K = p.k + hb, *Vt = p.vt + hb;
    bf16x8 qf[2];
#pragma unroll
    for (int kc = 0; kc < 2; kc++) qf[kc] = as_frag(ld16(Q + (size_t)(q0 + col) * VT_HD + kc * 32 + 8 * g));
    f32x4 acc[4];
#pragma unroll
    for (int dt = 0; dt < 4; dt++) acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;
    for (int kb = 0; kb < p.T; kb += 32) {
        f32x4 s[2];
#pragma unroll
        for (int i = 0; i < 2; i++) {
            s[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kc = 0; kc < 2; kc++)
                s[i] = mfma16(as_frag(ld16(K + (size_t)(kb + 16 * i + col) * VT_HD + kc * 32 + 8 * g)), qf[kc], s[i]);
        }
        float mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int key = kb + 16 * i + 4 * g + r;
                s[i][r] = key < p.T ? s[i][r] * VT_SCALE : -INFINITY;
                mx = fmaxf(mx, s[i][r]);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mn = fmaxf(m, mx);
        const float alpha = __expf(m - mn);
        float rs = 0.f;
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                s[i][r] = __expf(s[i][r] - mn);
                rs += s[i][r];
            }
        rs += __shfl_xor(rs, 16, 64);
        rs += __shfl_xor(rs, 32, 64);
        l = l * alpha + rs;
        m = mn;
        const bf16x8 pf = frag_acc(s[0], s[1]);
#pragma unroll
        for (int dt = 0; dt < 4; dt++) {
            const unsigned short *vr = Vt + (size_t)(dt * 16 + col) * p.Tp + kb + 4 * g;
            acc[dt] = acc[dt] * alpha;
            acc[dt] = mfma16(frag_2x4(ld8(vr), ld8(vr + 16)), pf, acc[dt]);
        }
    }
    const int qq = q0 + col;
    if (qq >= p.T) return;
    const int n = nh / p.heads, hh = nh - n * p.heads;
    const float inv = 1.f / l;
    unsigned short *orow = p.o + ((size_t)n * p.T + qq) * p.C + hh * VT_HD;
#pragma unroll
    for (int dt = 0; dt < 4; dt++)
        *(uint2 *)(orow + dt * 16 + 4 * g) = make_uint2(f2bf2(acc[dt][0] * inv, acc[dt][1] * inv), f2bf2(acc[dt][2] * inv, acc[dt][3] * inv));
    if (TRAIN && g == 0) p.lse[(size_t)nh * p.Tp + qq] = m + __logf(l);
}

// D[nh, t] = sum_d dO . O (bf16 values, fp32 sum); t >= T: 0
__global__ void __launch_bounds__(256) attn_dvec_kernel(const unsigned short *__restrict__ doh, const unsigned short *__restrict__ o,
                                                        const int NH, const int T, const int Tp, const int C, float *__restrict__ dvec) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)NH * Tp) return;
    const int heads = C / VT_HD, nh = (int)(i / Tp), t = (int)(i - (size_t)nh * Tp), n = nh / heads, hh = nh - n * heads;
    if (t >= T) { dvec[i] = 0.f; return; }
    const unsigned short *a = doh + i * VT_HD, *b = o + ((size_t)n * T + t) * C + hh * VT_HD;
    float s = 0.f;
    for (int d = 0; d < VT_HD; d++) s += bf2f(a[d]) * bf2f(b[d]);
    dvec[i] = s;
}

// dQ: one wave per 16 queries, a loop over all keys
__global__ void __launch_bounds__(256) attn_dq_kernel(const AttnP p) {
    const int lane = threadIdx.x & 63, g = lane >> 4, col = lane & 15;
    const int nh = blockIdx.y, q0 = blockIdx.x * 64 + (threadIdx.x >> 6) * 16;
    if (q0 >= p.T) return;
    const size_t hb = (size_t)nh * p.Tp * VT_HD;
    const unsigned short *Q = p.q + hb, *K = p.k + hb, *V = p.v + hb, *Kt = p.kt + hb, *dO = p.doh + hb;
    bf16x8 qf[2], df[2];
#pragma unroll
    for (int kc = 0; kc < 2; kc++) {
        qf[kc] = as_frag(ld16(Q + (size_t)(q0 + col) * VT_HD + kc * 32 + 8 * g));
        df[kc] = as_frag(ld16(dO + (size_t)(q0 + col) * VT_HD + kc * 32 + 8 * g));
    }
    const float lse = p.lse_in[(size_t)nh * p.Tp + q0 + col], D = p.dvec[(size_t)nh * p.Tp + q0 + col];
    const bool qok = q0 + col < p.T;
    f32x4 acc[4];
#pragma unroll
    for (int dt = 0; dt < 4; dt++) acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kb = 0; kb < p.T; kb += 32) {
        f32x4 s[2], dp[2];
#pragma unroll
        for (int i = 0; i < 2; i++) {
            s[i] = dp[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kc = 0; kc < 2; kc++) {
                const size_t off = (size_t)(kb + 16 * i + col) * VT_HD + kc * 32 + 8 * g;
                s[i] = mfma16(as_frag(ld16(K + off)), qf[kc], s[i]);
                dp[i] = mfma16(as_frag(ld16(V + off)), df[kc], dp[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int key = kb + 16 * i + 4 * g + r;
                const float pr = (key < p.T && qok) ? __expf(s[i][r] * VT_SCALE - lse) : 0.f;
                s[i][r] = pr * (dp[i][r] - D);
            }
        const bf16x8 sf = frag_acc(s[0], s[1]);
#pragma unroll
        for (int dt = 0; dt < 4; dt++) {
            const unsigned short *kr = Kt + (size_t)(dt * 16 + col) * p.Tp + kb + 4 * g;
            acc[dt] = mfma16(frag_2x4(ld8(kr), ld8(kr + 16)), sf, acc[dt]);
        }
    }
    if (!qok) return;
    const int n = nh / p.heads, hh = nh - n * p.heads;
    unsigned short *row = p.dqkv + ((size_t)n * p.T + q0 + col) * 3 * p.C + hh * VT_HD;
#pragma unroll
    for (int dt = 0; dt < 4; dt++)
        *(uint2 *)(row + dt * 16 + 4 * g) = make_uint2(f2bf2(acc[dt][0] * VT_SCALE, acc[dt][1] * VT_SCALE),
                                                      f2bf2(acc[dt][2] * VT_SCALE, acc[dt][3] * VT_SCALE));
}

// dK, dV: one wave per 16 keys, a loop over all queries
__global__ void __launch_bounds__(256) attn_dkv_kernel(const AttnP p) {
    const int lane = threadIdx.x & 63, g = lane >> 4, col = lane & 15;
    const int nh = blockIdx.y, k0 = blockIdx.x * 64 + (threadIdx.x >> 6) * 16;
    if (k0 >= p.T) return;
    const size_t hb = (size_t)nh * p.Tp * VT_HD;
    const unsigned short *Q = p.q + hb, *K = p.k + hb, *V = p.v + hb, *Qt = p.qt + hb, *dO = p.doh + hb, *dOt = p.dot + hb;
    const float *lse = p.lse_in + (size_t)nh * p.Tp, *Dv = p.dvec + (size_t)nh * p.Tp;
    bf16x8 kf[2], vf[2];
#pragma unroll
    for (int kc = 0; kc < 2; kc++) {
        kf[kc] = as_frag(ld16(K + (size_t)(k0 + col) * VT_HD + kc * 32 + 8 * g));
        vf[kc] = as_frag(ld16(V + (size_t)(k0 + col) * VT_HD + kc * 32 + 8 * g));
    }
    f32x4 dk[4], dv[4];
#pragma unroll
    for (int dt = 0; dt < 4; dt++) dk[dt] = dv[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int qb = 0; qb < p.T; qb += 32) {
        f32x4 s[2], dp[2];
#pragma unroll
        for (int i = 0; i < 2; i++) {
            s[i] = dp[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kc = 0; kc < 2; kc++) {
                const size_t off = (size_t)(qb + 16 * i + col) * VT_HD + kc * 32 + 8 * g;
                s[i] = mfma16(as_frag(ld16(Q + off)), kf[kc], s[i]);
                dp[i] = mfma16(as_frag(ld16(dO + off)), vf[kc], dp[i]);
            }
        }
        float ds[2][4];
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int qr = qb + 16 * i + 4 * g;
            const float4 L = *(const float4 *)(lse + qr), Dq = *(const float4 *)(Dv + qr);
            const float Ls[4] = {L.x, L.y, L.z, L.w}, Ds[4] = {Dq.x, Dq.y, Dq.z, Dq.w};
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float pr = qr + r < p.T ? __expf(s[i][r] * VT_SCALE - Ls[r]) : 0.f;
                s[i][r] = pr;
                ds[i][r] = pr * (dp[i][r] - Ds[r]);
            }
        }
        const bf16x8 pf = frag_acc(s[0], s[1]);
        const bf16x8 sf = frag_acc(f32x4{ds[0][0], ds[0][1], ds[0][2], ds[0][3]}, f32x4{ds[1][0], ds[1][1], ds[1][2], ds[1][3]});
#pragma unroll
        for (int dt = 0; dt < 4; dt++) {
            const unsigned short *orr = dOt + (size_t)(dt * 16 + col) * p.Tp + qb + 4 * g;
            const unsigned short *qr = Qt + (size_t)(dt * 16 + col) * p.Tp + qb + 4 * g;
            dv[dt] = mfma16(frag_2x4(ld8(orr), ld8(orr + 16)), pf, dv[dt]);
            dk[dt] = mfma16(frag_2x4(ld8(qr), ld8(qr + 16)), sf, dk[dt]);
        }
    }
    if (k0 + col >= p.T) return;
    const int n = nh / p.heads, hh = nh - n * p.heads;
    unsigned short *row = p.dqkv + ((size_t)n * p.T + k0 + col) * 3 * p.C + hh * VT_HD;
#pragma unroll
    for (int dt = 0; dt < 4; dt++) {
        *(uint2 *)(row + p.C + dt * 16 + 4 * g) = make_uint2(f2bf2(dk[dt][0] * VT_SCALE, dk[dt][1] * VT_SCALE),
                                                            f2bf2(dk[dt][2] * VT_SCALE, dk[dt][3] * VT_SCALE));
        *(uint2 *)(row + 2 * p.C + dt * 16 + 4 * g) = make_uint2(f2bf2(dv[dt][0], dv[dt][1]), f2bf2(dv[dt][2], dv[dt][3]));
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// host side
struct Geo {
    int N, views, H, W, C, heads, F, depth, h, w, hw, T, M, Mp, Tp, NP, Pp, NH;
    float eps;
    long long s[5];
};

bool make_geo(const lara_vit_dims *d, Geo &g) {
    if (!d) return false;
    if (d->N < 1 || d->views < 1 || d->N % d->views || d->H < 16 || d->W < 16 || (d->H & 15) || (d->W & 15)) return false;
    if (d->C < 64 || d->C > LARA_VIT_MAX_C || (d->C & 63) || d->heads < 1 || d->C != VT_HD * d->heads) return false;
    if (d->F < 64 || d->F > LARA_VIT_MAX_F || (d->F & 63) || d->depth < 1 || d->depth > 64 || !(d->eps > 0.f)) return false;
    const long long T = 1 + (long long)(d->H / 16) * (d->W / 16);
    if (T > LARA_VIT_MAX_T || (long long)d->N * T > (1 << 20)) return false;
    g.N = d->N; g.views = d->views; g.H = d->H; g.W = d->W; g.C = d->C; g.heads = d->heads; g.F = d->F; g.depth = d->depth; g.eps = d->eps;
    g.h = d->H / 16; g.w = d->W / 16; g.hw = g.h * g.w; g.T = (int)T; g.M = g.N * g.T; g.Mp = rup(g.M, 128); g.Tp = rup(g.T, 64);
    g.NP = g.N * g.hw; g.Pp = rup(g.NP, 128); g.NH = g.N * g.heads;
    for (int i = 0; i < 5; i++) g.s[i] = d->img_stride[i];
    return true;
}

struct Alloc {
    size_t total = 0;
    size_t take(size_t bytes) { const size_t o = total; total += up256(bytes); return o; }
};

// what one block keeps for the backward
struct BlkOff { size_t xin, xn1, st1, q, k, v, o, lse, xmid, xn2, st2, h; };
BlkOff blk_layout(const Geo &g, Alloc &a) {
    BlkOff b;
    const size_t MC = (size_t)g.M * g.C, hd = (size_t)g.NH * g.Tp * VT_HD * 2;
    b.xin = a.take(MC * 4); b.xn1 = a.take((size_t)g.Mp * g.C * 2); b.st1 = a.take((size_t)g.M * 8);
    b.q = a.take(hd); b.k = a.take(hd); b.v = a.take(hd); b.o = a.take((size_t)g.Mp * g.C * 2); b.lse = a.take((size_t)g.NH * g.Tp * 4);
    b.xmid = a.take(MC * 4); b.xn2 = a.take((size_t)g.Mp * g.C * 2); b.st2 = a.take((size_t)g.M * 8); b.h = a.take((size_t)g.Mp * g.F * 2);
    return b;
}
struct SaveLay { size_t patches, xfin, stf, blk0, blk_bytes, total; BlkOff b; };
SaveLay save_layout(const Geo &g) {
    SaveLay s;
    Alloc a;
    s.patches = a.take((size_t)g.Pp * VT_PD * 2);
    s.xfin = a.take((size_t)g.M * g.C * 4);
    s.stf = a.take((size_t)g.M * 8);
    s.blk0 = a.total;
    Alloc ab;
    s.b = blk_layout(g, ab);
    s.blk_bytes = ab.total;
    s.total = s.blk0 + s.blk_bytes * g.depth;
    return s;
}
// forward workspace (inference: plus one block's save region, the patch rows, two residual buffers and the final statistics)
struct FwdLay { size_t wpatch, wq, wp, w1, w2, acc, vt, gb, blk, patches, xa, xb, stf, total; BlkOff b; };
FwdLay fwd_layout(const Geo &g, bool inference) {
    FwdLay f{};
    Alloc a;
    const size_t C = g.C, F = g.F;
    f.wpatch = a.take(C * VT_PD * 2); f.wq = a.take(3 * C * C * 2); f.wp = a.take(C * C * 2); f.w1 = a.take(F * C * 2); f.w2 = a.take(C * F * 2);
    f.acc = a.take(std::max((size_t)g.Mp * std::max(3 * C, F), (size_t)g.Pp * C) * 4);
    f.vt = a.take((size_t)g.NH * g.Tp * VT_HD * 2);
    f.gb = a.take((size_t)g.Mp * F * 2);
    if (inference) {
        Alloc ab;
        f.b = blk_layout(g, ab);
        f.blk = a.take(ab.total);
        f.patches = a.take((size_t)g.Pp * VT_PD * 2);
        f.xa = a.take((size_t)g.M * C * 4); f.xb = a.take((size_t)g.M * C * 4);
        f.stf = a.take((size_t)g.M * 8);
    }
    f.total = a.total;
    return f;
}
struct BwdLay { size_t wqT, wpT, w1T, w2T, dres, dy, dh, gb, dxn, dob, doh, dot, qt, kt, vt, dvec, dqkv, tn, part, dconv, total; };
BwdLay bwd_layout(const Geo &g) {
    BwdLay b{};
    Alloc a;
    const size_t C = g.C, F = g.F, hd = (size_t)g.NH * g.Tp * VT_HD * 2;
    b.wqT = a.take(3 * C * C * 2); b.wpT = a.take(C * C * 2); b.w1T = a.take(C * F * 2); b.w2T = a.take(F * C * 2);
    b.dres = a.take((size_t)g.M * C * 4); b.dy = a.take((size_t)g.Mp * C * 2); b.dh = a.take((size_t)g.Mp * F * 2);
    b.gb = a.take((size_t)g.Mp * F * 2); b.dxn = a.take((size_t)g.Mp * C * 2); b.dob = a.take((size_t)g.Mp * C * 2);
    b.doh = a.take(hd); b.dot = a.take(hd); b.qt = a.take(hd); b.kt = a.take(hd); b.vt = a.take(hd);
    b.dvec = a.take((size_t)g.NH * g.Tp * 4); b.dqkv = a.take((size_t)g.Mp * 3 * C * 2);
    b.tn = a.take((size_t)lara_gemm_tn_workspace_bytes());
    b.part = a.take(std::max((size_t)VT_LNB * 2 * C, (size_t)VT_CSP * std::max(3 * C, F)) * 4);
    b.dconv = a.take((size_t)g.Pp * C * 2);
    b.total = a.total;
    return b;
}

inline unsigned nblk(const size_t n) { return (unsigned)((n + 255) / 256); }

struct BlkPtr {
    float *xin, *xmid, *xout;
    unsigned short *xn1, *q, *k, *v, *o, *xn2, *h;
    float2 *st1, *st2;
    float *lse;
};
BlkPtr blk_ptrs(char *base, const BlkOff &b) {
    BlkPtr p;
    p.xin = (float *)(base + b.xin); p.xmid = (float *)(base + b.xmid); p.xout = nullptr;
    p.xn1 = (unsigned short *)(base + b.xn1); p.q = (unsigned short *)(base + b.q); p.k = (unsigned short *)(base + b.k);
    p.v = (unsigned short *)(base + b.v); p.o = (unsigned short *)(base + b.o); p.xn2 = (unsigned short *)(base + b.xn2);
    p.h = (unsigned short *)(base + b.h); p.st1 = (float2 *)(base + b.st1); p.st2 = (float2 *)(base + b.st2);
    p.lse = (float *)(base + b.lse);
    return p;
}

// a call that returns a LARA2DGS status, under its profile label
#define VT_PROF(name, call)                                   \
    do {                                                      \
        L2D_PROF(name, s);                                    \
        L2D_TRY(call);                                        \
    } while (0)

int cast_w(const float *src, size_t n, unsigned short *dst, hipStream_t s) {
    L2D_LAUNCH_IN_SCOPE(s, wcast_kernel, dim3(nblk(n)), dim3(256), 0, src, n, dst);
    return LARA2DGS_OK;
}
int trans_w(const float *src, int R, int Cc, unsigned short *dst, hipStream_t s) {
    L2D_LAUNCH_IN_SCOPE(s, wtrans_kernel, dim3((Cc + 31) / 32, (R + 31) / 32), dim3(256), 0, src, R, Cc, dst);
    return LARA2DGS_OK;
}
// bias gradient: fixed-order column sums of bf16 rows
int colsum(const unsigned short *src, int rows, int ncol, float *part, float *out, hipStream_t s) {
    L2D_LAUNCH_IN_SCOPE(s, colsum_part_kernel, dim3((ncol + 255) / 256, VT_CSP), dim3(256), 0, src, rows, ncol, part);
    L2D_LAUNCH_IN_SCOPE(s, sum_parts_kernel, dim3((ncol + 255) / 256), dim3(256), 0, (const float *)part, VT_CSP, ncol, out, out, ncol);
    return LARA2DGS_OK;
}
// dW [N, K] = dY^T X  (written)
int wgrad(int Mp, int N, int K, const unsigned short *dY, const unsigned short *X, float *dW, void *tn, hipStream_t s) {
    L2D_HIP(hipMemsetAsync(dW, 0, (size_t)N * K * 4, s));
    return lara_gemm_tn_bf16(Mp, N, K, dY, X, dW, tn, s);
}

const float *P(const float *const *params, int i) { return params[i]; }
inline int bp(int blk, int j) { return 4 + 12 * blk + j; }

}  // namespace

extern "C" {

int64_t lara_vit_save_bytes(const lara_vit_dims *d) {
    Geo g;
    if (!make_geo(d, g)) return LARA2DGS_E_INVALID;
    return (int64_t)save_layout(g).total;
}

int lara_vit_save_offsets(const lara_vit_dims *d, int64_t *offsets, int32_t n) {
    Geo g;
    if (!make_geo(d, g) || !offsets || n != 17) return LARA2DGS_E_INVALID;
    const SaveLay sl = save_layout(g);
    const BlkOff &b = sl.b;
    const size_t o[17] = {sl.patches, sl.xfin, sl.stf, sl.blk0, sl.blk_bytes, b.xin, b.xn1, b.st1, b.q, b.k, b.v, b.o, b.lse, b.xmid, b.xn2,
                          b.st2, b.h};
    for (int i = 0; i < 17; i++) offsets[i] = (int64_t)o[i];
    return LARA2DGS_OK;
}

int64_t lara_vit_workspace_bytes(const lara_vit_dims *d, int32_t training) {
    Geo g;
    if (!make_geo(d, g)) return LARA2DGS_E_INVALID;
    if (!training) return (int64_t)fwd_layout(g, true).total;
    return (int64_t)std::max(fwd_layout(g, false).total, bwd_layout(g).total);
}

int lara_vit_forward(const lara_vit_dims *d, const float *images, const float *const *params, float *out, void *save, void *workspace,
                     void *stream) {
    Geo g;
    if (!make_geo(d, g) || !images || !params || !out || !workspace) return LARA2DGS_E_INVALID;
    for (int i = 0; i < LARA_VIT_NPARAMS(g.depth); i++)
        if (!params[i]) return LARA2DGS_E_INVALID;
    const hipStream_t s = (hipStream_t)stream;
    const bool train = save != nullptr;
    const FwdLay fl = fwd_layout(g, !train);
    const SaveLay sl = save_layout(g);
    char *ws = (char *)workspace, *sv = (char *)save;
    const int C = g.C, F = g.F, depth = g.depth;
    unsigned short *wq = (unsigned short *)(ws + fl.wq), *wp = (unsigned short *)(ws + fl.wp);
    unsigned short *w1 = (unsigned short *)(ws + fl.w1), *w2 = (unsigned short *)(ws + fl.w2);
    unsigned short *vt = (unsigned short *)(ws + fl.vt), *gb = (unsigned short *)(ws + fl.gb);
    float *acc = (float *)(ws + fl.acc);
    unsigned short *patches = (unsigned short *)(train ? sv + sl.patches : ws + fl.patches);
    float2 *stf = (float2 *)(train ? sv + sl.stf : ws + fl.stf);
    float *x0 = train ? (float *)(sv + sl.blk0 + sl.b.xin) : (float *)(ws + fl.xa);
    {
        PatchP pp{images, g.s[0], g.s[1], g.s[2], g.s[3], g.s[4], g.NP, g.Pp, g.hw, g.w, g.views};
        L2D_LAUNCH("vit_elementwise", s, patch_kernel, dim3(nblk((size_t)g.Pp * VT_PD / 2)), dim3(256), 0, pp, (unsigned *)patches);
        VT_PROF("vit_elementwise", cast_w(P(params, 2), (size_t)C * VT_PD, (unsigned short *)(ws + fl.wpatch), s));
        VT_PROF("vit_products", lara_gemm_nt_bf16(g.Pp, C, VT_PD, patches, (const uint16_t *)(ws + fl.wpatch), acc, 1, s));
        L2D_LAUNCH("vit_elementwise", s, tokens_kernel, dim3(nblk((size_t)g.M * C)), dim3(256), 0, (const float *)acc, P(params, 3), P(params, 0),
                   P(params, 1), g.N, g.T, C, x0);
    }
    AttnP ap{};
    ap.T = g.T; ap.Tp = g.Tp; ap.C = C; ap.heads = g.heads; ap.vt = vt;
    const size_t mc = (size_t)g.M * C;
    for (int i = 0; i < depth; i++) {
        BlkPtr b;
        if (train) {
            b = blk_ptrs(sv + sl.blk0 + sl.blk_bytes * i, sl.b);
            b.xout = i + 1 < depth ? (float *)(sv + sl.blk0 + sl.blk_bytes * (i + 1) + sl.b.xin) : (float *)(sv + sl.xfin);
        } else {
            b = blk_ptrs(ws + fl.blk, fl.b);
            b.xin = (float *)(ws + ((i & 1) ? fl.xb : fl.xa));
            b.xout = (float *)(ws + ((i & 1) ? fl.xa : fl.xb));
        }
        VT_PROF("vit_elementwise", cast_w(P(params, bp(i, 2)), (size_t)3 * C * C, wq, s));
        VT_PROF("vit_elementwise", cast_w(P(params, bp(i, 4)), (size_t)C * C, wp, s));
        VT_PROF("vit_elementwise", cast_w(P(params, bp(i, 8)), (size_t)F * C, w1, s));
        VT_PROF("vit_elementwise", cast_w(P(params, bp(i, 10)), (size_t)C * F, w2, s));
        L2D_LAUNCH("vit_layernorm", s, ln_fwd_kernel<false>, dim3((g.Mp + 3) / 4), dim3(256), 0, (const float *)b.xin, P(params, bp(i, 0)),
                   P(params, bp(i, 1)), g.M, g.Mp, g.T, C, g.eps, (void *)b.xn1, b.st1);
        VT_PROF("vit_products", lara_gemm_nt_bf16(g.Mp, 3 * C, C, b.xn1, wq, acc, 1, s));
        L2D_LAUNCH("vit_attention", s, qkv_split_kernel, dim3(nblk((size_t)3 * g.NH * g.Tp * VT_HD)), dim3(256), 0, (const float *)acc,
                   P(params, bp(i, 3)), g.N, g.T, g.Tp, C, b.q, b.k, b.v);
        L2D_LAUNCH("vit_attention", s, head_t_kernel, dim3(g.Tp / 64, g.NH), dim3(256), 0, (const unsigned short *)b.v, g.NH, g.Tp, vt);
        if (g.Mp > g.M) L2D_HIP(hipMemsetAsync(b.o + mc, 0, (size_t)(g.Mp - g.M) * C * 2, s));
        ap.q = b.q; ap.k = b.k; ap.o = b.o; ap.lse = b.lse;
        if (train) L2D_LAUNCH("vit_attention", s, attn_fwd_kernel<true>, dim3(g.Tp / 64, g.NH), dim3(256), 0, ap);
        else L2D_LAUNCH("vit_attention", s, attn_fwd_kernel<false>, dim3(g.Tp / 64, g.NH), dim3(256), 0, ap);
        VT_PROF("vit_products", lara_gemm_nt_bf16(g.Mp, C, C, b.o, wp, acc, 1, s));
        L2D_LAUNCH("vit_elementwise", s, residual_kernel, dim3(nblk(mc)), dim3(256), 0, (const float *)acc, P(params, bp(i, 5)), (const float *)b.xin,
                   g.M, C, b.xmid);
        L2D_LAUNCH("vit_layernorm", s, ln_fwd_kernel<false>, dim3((g.Mp + 3) / 4), dim3(256), 0, (const float *)b.xmid, P(params, bp(i, 6)),
                   P(params, bp(i, 7)), g.M, g.Mp, g.T, C, g.eps, (void *)b.xn2, b.st2);
        VT_PROF("vit_products", lara_gemm_nt_bf16(g.Mp, F, C, b.xn2, w1, acc, 1, s));
        L2D_LAUNCH("vit_elementwise", s, fc1_kernel, dim3(nblk((size_t)g.Mp * F)), dim3(256), 0, (const float *)acc, P(params, bp(i, 9)), g.M, g.Mp, F,
                   train ? b.h : (unsigned short *)nullptr, gb);
        VT_PROF("vit_products", lara_gemm_nt_bf16(g.Mp, C, F, gb, w2, acc, 1, s));
        L2D_LAUNCH("vit_elementwise", s, residual_kernel, dim3(nblk(mc)), dim3(256), 0, (const float *)acc, P(params, bp(i, 11)), (const float *)b.xmid,
                   g.M, C, b.xout);
    }
    {
        const float *xf = train ? (const float *)(sv + sl.xfin) : (const float *)(ws + ((depth & 1) ? fl.xb : fl.xa));
        L2D_LAUNCH("vit_layernorm", s, ln_fwd_kernel<true>, dim3((g.M + 3) / 4), dim3(256), 0, xf, P(params, bp(depth, 0)), P(params, bp(depth, 1)),
                   g.M, g.M, g.T, C, g.eps, (void *)out, stf);
    }
    return LARA2DGS_OK;
}

int lara_vit_backward(const lara_vit_dims *d, const float *const *params, const void *save, const float *grad, float *const *grads,
                      void *workspace, void *stream) {
    Geo g;
    if (!make_geo(d, g) || !params || !save || !grad || !grads || !workspace) return LARA2DGS_E_INVALID;
    for (int i = 0; i < LARA_VIT_NPARAMS(g.depth); i++)
        if (!params[i] || !grads[i]) return LARA2DGS_E_INVALID;
    const hipStream_t s = (hipStream_t)stream;
    const SaveLay sl = save_layout(g);
    const BwdLay bl = bwd_layout(g);
    char *sv = (char *)save, *ws = (char *)workspace;
    const int C = g.C, F = g.F, depth = g.depth, M = g.M, Mp = g.Mp;
    auto u16 = [&](size_t off) { return (unsigned short *)(ws + off); };
    float *dres = (float *)(ws + bl.dres), *part = (float *)(ws + bl.part);
    unsigned short *dy = u16(bl.dy), *dh = u16(bl.dh), *gb = u16(bl.gb), *dxn = u16(bl.dxn), *dob = u16(bl.dob), *dqkv = u16(bl.dqkv);
    unsigned short *wqT = u16(bl.wqT), *wpT = u16(bl.wpT), *w1T = u16(bl.w1T), *w2T = u16(bl.w2T);
    void *tn = ws + bl.tn;
    const size_t hd = (size_t)g.NH * g.Tp * VT_HD;
    {
        L2D_LAUNCH("vit_layernorm", s, ln_bwd_kernel<true>, dim3(VT_LNB), dim3(256), 0, (const void *)grad, (const float *)(sv + sl.xfin),
                   (const float2 *)(sv + sl.stf), P(params, bp(depth, 0)), M, g.T, C, dres, part);
        L2D_LAUNCH("vit_layernorm", s, sum_parts_kernel, dim3((2 * C + 255) / 256), dim3(256), 0, (const float *)part, VT_LNB, 2 * C,
                   grads[bp(depth, 0)], grads[bp(depth, 1)], C);
        if (Mp > M) L2D_HIP(hipMemsetAsync(dqkv + (size_t)M * 3 * C, 0, (size_t)(Mp - M) * 3 * C * 2, s));
    }
    AttnP ap{};
    ap.T = g.T; ap.Tp = g.Tp; ap.C = C; ap.heads = g.heads;
    ap.doh = u16(bl.doh); ap.dot = u16(bl.dot); ap.qt = u16(bl.qt); ap.kt = u16(bl.kt); ap.vt = u16(bl.vt);
    ap.dvec = (const float *)(ws + bl.dvec); ap.dqkv = dqkv;
    for (int i = depth - 1; i >= 0; i--) {
        const BlkPtr b = blk_ptrs(sv + sl.blk0 + sl.blk_bytes * i, sl.b);
        VT_PROF("vit_elementwise", trans_w(P(params, bp(i, 2)), 3 * C, C, wqT, s));
        VT_PROF("vit_elementwise", trans_w(P(params, bp(i, 4)), C, C, wpT, s));
        VT_PROF("vit_elementwise", trans_w(P(params, bp(i, 8)), F, C, w1T, s));
        VT_PROF("vit_elementwise", trans_w(P(params, bp(i, 10)), C, F, w2T, s));
        // MLP half: x'' = x' + fc2(GELU(fc1(LN2(x'))))
        L2D_LAUNCH("vit_elementwise", s, rows_bf16_kernel, dim3(nblk((size_t)Mp * C)), dim3(256), 0, (const float *)dres, M, Mp, C, dy);
        VT_PROF("vit_elementwise", colsum(dy, Mp, C, part, grads[bp(i, 11)], s));
        L2D_LAUNCH("vit_elementwise", s, gelu_kernel, dim3(nblk((size_t)Mp * F)), dim3(256), 0, (const unsigned short *)b.h, (size_t)Mp * F, gb);
        VT_PROF("vit_products", wgrad(Mp, C, F, dy, gb, grads[bp(i, 10)], tn, s));
        VT_PROF("vit_products", lara_gemm_nt_bf16(Mp, F, C, dy, w2T, dh, 0, s));
        L2D_LAUNCH("vit_elementwise", s, gelu_bwd_kernel, dim3(nblk((size_t)Mp * F)), dim3(256), 0, (const unsigned short *)b.h, (size_t)Mp * F, dh);
        VT_PROF("vit_elementwise", colsum(dh, Mp, F, part, grads[bp(i, 9)], s));
        VT_PROF("vit_products", wgrad(Mp, F, C, dh, b.xn2, grads[bp(i, 8)], tn, s));
        VT_PROF("vit_products", lara_gemm_nt_bf16(Mp, C, F, dh, w1T, dxn, 0, s));
        L2D_LAUNCH("vit_layernorm", s, ln_bwd_kernel<false>, dim3(VT_LNB), dim3(256), 0, (const void *)dxn, (const float *)b.xmid,
                   (const float2 *)b.st2, P(params, bp(i, 6)), M, g.T, C, dres, part);
        L2D_LAUNCH("vit_layernorm", s, sum_parts_kernel, dim3((2 * C + 255) / 256), dim3(256), 0, (const float *)part, VT_LNB, 2 * C,
                   grads[bp(i, 6)], grads[bp(i, 7)], C);
        // attention half: x' = x + proj(attn(qkv(LN1(x))))
        L2D_LAUNCH("vit_elementwise", s, rows_bf16_kernel, dim3(nblk((size_t)Mp * C)), dim3(256), 0, (const float *)dres, M, Mp, C, dy);
        VT_PROF("vit_elementwise", colsum(dy, Mp, C, part, grads[bp(i, 5)], s));
        VT_PROF("vit_products", wgrad(Mp, C, C, dy, b.o, grads[bp(i, 4)], tn, s));
        VT_PROF("vit_products", lara_gemm_nt_bf16(Mp, C, C, dy, wpT, dob, 0, s));
        L2D_LAUNCH("vit_attention", s, head_split_kernel, dim3(nblk(hd)), dim3(256), 0, (const unsigned short *)dob, g.N, g.T, g.Tp, C, u16(bl.doh));
        L2D_LAUNCH("vit_attention", s, attn_dvec_kernel, dim3(nblk((size_t)g.NH * g.Tp)), dim3(256), 0, (const unsigned short *)u16(bl.doh),
                   (const unsigned short *)b.o, g.NH, g.T, g.Tp, C, (float *)(ws + bl.dvec));
        L2D_LAUNCH("vit_attention", s, head_t_kernel, dim3(g.Tp / 64, g.NH), dim3(256), 0, (const unsigned short *)u16(bl.doh), g.NH, g.Tp, u16(bl.dot));
        L2D_LAUNCH("vit_attention", s, head_t_kernel, dim3(g.Tp / 64, g.NH), dim3(256), 0, (const unsigned short *)b.q, g.NH, g.Tp, u16(bl.qt));
        L2D_LAUNCH("vit_attention", s, head_t_kernel, dim3(g.Tp / 64, g.NH), dim3(256), 0, (const unsigned short *)b.k, g.NH, g.Tp, u16(bl.kt));
        ap.q = b.q; ap.k = b.k; ap.v = b.v; ap.lse_in = b.lse;
        L2D_LAUNCH("vit_attention", s, attn_dq_kernel, dim3(g.Tp / 64, g.NH), dim3(256), 0, ap);
        L2D_LAUNCH("vit_attention", s, attn_dkv_kernel, dim3(g.Tp / 64, g.NH), dim3(256), 0, ap);
        VT_PROF("vit_elementwise", colsum(dqkv, Mp, 3 * C, part, grads[bp(i, 3)], s));
        VT_PROF("vit_products", wgrad(Mp, 3 * C, C, dqkv, b.xn1, grads[bp(i, 2)], tn, s));
        VT_PROF("vit_products", lara_gemm_nt_bf16(Mp, C, 3 * C, dqkv, wqT, dxn, 0, s));
        L2D_LAUNCH("vit_layernorm", s, ln_bwd_kernel<false>, dim3(VT_LNB), dim3(256), 0, (const void *)dxn, (const float *)b.xin,
                   (const float2 *)b.st1, P(params, bp(i, 0)), M, g.T, C, dres, part);
        L2D_LAUNCH("vit_layernorm", s, sum_parts_kernel, dim3((2 * C + 255) / 256), dim3(256), 0, (const float *)part, VT_LNB, 2 * C,
                   grads[bp(i, 0)], grads[bp(i, 1)], C);
    }
    {
        L2D_LAUNCH("vit_elementwise", s, tokens_bwd_kernel, dim3(nblk((size_t)g.T * C)), dim3(256), 0, (const float *)dres, g.N, g.T, C, grads[1], grads[0]);
        unsigned short *dconv = u16(bl.dconv);
        L2D_LAUNCH("vit_elementwise", s, dconv_kernel, dim3(nblk((size_t)g.Pp * C)), dim3(256), 0, (const float *)dres, g.N, g.T, C, g.Pp, dconv);
        VT_PROF("vit_elementwise", colsum(dconv, g.Pp, C, part, grads[3], s));
        VT_PROF("vit_products", wgrad(g.Pp, C, VT_PD, dconv, (const unsigned short *)(sv + sl.patches), grads[2], tn, s));
    }
    return LARA2DGS_OK;
}

}  // extern "C"
