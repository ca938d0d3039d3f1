// lpips.hip -- LPIPS forward (VGG-16 and AlexNet variants) on gfx950.  Interface, formulas and layouts in include/lara_lpips.h.
//
//   lp_conv_mfma_kernel<NT>  implicit-GEMM convolution on v_mfma_f32_32x32x2_f32 (exact fp32 products, one k-ordered fmaf chain per
//                            output): a workgroup owns 128 pixels x 64 NT output channels, a wave 64 x 32 NT (2 x NT accumulator
//                            tiles).  K runs tap by tap in chunks of 32 input channels; the im2col rows of a chunk (zeros where the
//                            window leaves the image) and the weight rows are gathered with 16-byte loads into registers while the
//                            previous chunk multiplies, then stored to LDS (rows of 36 floats).  Bias and ReLU in the epilogue.
//                            General in kernel size, stride and pad; M (pixels of the whole batch) is arbitrary.
//   lp_conv_image_kernel     the Cin = 3 first layer (K = 27 or 363): a vector kernel, one output pixel x 16 channels per thread,
//                            weights through wave-uniform (scalar) loads.  It reads the images through their strided views and
//                            applies in_mul x + in_add and the scaling layer on the way.  Why not a padded-K MFMA case: the layer is
//                            0.6 % (VGG) / 10 % (AlexNet) of its net's work, its operand is a 3-float pixel of a strided view, which
//                            has no 16-byte gather, and K = 27 would be padded to 32 with 16 % idle products.
//   lp_maxpool_kernel        floor-mode max pool, any window and stride, NHWC, four channels per thread.
//   lp_dist_kernel           one tap: a wave per pixel reads both images' channel vectors (contiguous), forms the two norms and the
//                            weighted squared difference; double sums per thread -> wave -> workgroup partial.
//   lp_finish_kernel         one workgroup per scene adds the partials of each tap in a fixed order, divides by the pixel count.
// No atomics: a call is bit-reproducible and a scene's row does not depend on the batch it is in.
#include "common.h"
#include "wave.h"
#include "../../include/lara_lpips.h"

namespace {

constexpr int LP_BM = 128, LP_BK = 32, LP_LD = 36;       // pixel tile, K chunk, LDS row length (floats; 16-byte aligned rows)
constexpr int LP_CO = 16;                                // output channels per thread of the first-layer kernel
constexpr int LP_DPIX = 256;                             // pixels per workgroup of the distance kernel (64 per wave)
constexpr int LP_MAXC = 512;                             // channels of a tap: at most 8 per lane

struct LpConv {
    const float *x, *w, *bias;
    float *y;
    int H, W, Cin, Cout, Ho, Wo, k, stride, pad, relu;
    long long M;                                         // N * Ho * Wo
};

template <int NT>
__global__ void __launch_bounds__(256)
lp_conv_mfma_kernel(const LpConv p) {
    constexpr int BN = 64 * NT;
    __shared__ __attribute__((aligned(16))) float As[LP_BM][LP_LD];
    __shared__ __attribute__((aligned(16))) float Bs[BN][LP_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave & 1, wn = wave >> 1;
    const int nct = p.Cout / BN;                         // channel tiles are the fast index: neighbours share their im2col rows in L2
    const int co0 = (int)(blockIdx.x % nct) * BN;
    const long long m0 = (long long)(blockIdx.x / nct) * LP_BM;
    const int c4 = (tid & 7) * 4, r0 = tid >> 3;         // this thread stages columns c4..c4+3 of rows r0 + 32 j

    const float *xrow[4];
    int iy0[4], ix0[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const long long m = m0 + r0 + 32 * j;
        if (m < p.M) {
            const long long hw = (long long)p.Ho * p.Wo, n = m / hw;
            const int rem = (int)(m - n * hw), oy = rem / p.Wo, ox = rem - oy * p.Wo;
            xrow[j] = p.x + (size_t)n * p.H * p.W * p.Cin + c4;
            iy0[j] = oy * p.stride - p.pad;
            ix0[j] = ox * p.stride - p.pad;
        } else {
            xrow[j] = nullptr;
            iy0[j] = ix0[j] = 0;
        }
    }
    const size_t wrow = (size_t)p.k * p.k * p.Cin;
    const float *wbase = p.w + (size_t)(co0 + r0) * wrow + c4;

    f32x4 ra[4], rb[2 * NT];
    int kh = 0, kw = 0, cc = 0;
#define LP_GATHER()                                                                                                              \
    do {                                                                                                                         \
        _Pragma("unroll") for (int j = 0; j < 4; j++) {                                                                          \
            const int iy = iy0[j] + kh, ix = ix0[j] + kw;                                                                        \
            const bool in = xrow[j] != nullptr && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;                                    \
            const f32x4 t4 = *(const f32x4 *)(in ? xrow[j] + ((size_t)iy * p.W + ix) * p.Cin + cc : p.x);                        \
            ra[j] = in ? t4 : (f32x4)(0.f);                                                                                      \
        }                                                                                                                        \
        const size_t wo = (size_t)(kh * p.k + kw) * p.Cin + cc;                                                                  \
        _Pragma("unroll") for (int j = 0; j < 2 * NT; j++) rb[j] = *(const f32x4 *)(wbase + (size_t)(32 * j) * wrow + wo);       \
    } while (0)

    f32x16 acc[2][NT];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < NT; b++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[a][b][r] = 0.f;

    const int nq = p.k * p.k * (p.Cin / LP_BK);
    const int li = lane & 31, lh = lane >> 5;
    LP_GATHER();
    for (int q = 0; q < nq; q++) {
#pragma unroll
        for (int j = 0; j < 4; j++) *(f32x4 *)&As[r0 + 32 * j][c4] = ra[j];
#pragma unroll
        for (int j = 0; j < 2 * NT; j++) *(f32x4 *)&Bs[r0 + 32 * j][c4] = rb[j];
        __syncthreads();
        if (q + 1 < nq) {                                // the next chunk's loads fly while this one multiplies
            cc += LP_BK;
            if (cc == p.Cin) { cc = 0; if (++kw == p.k) { kw = 0; kh++; } }
            LP_GATHER();
        }
#pragma unroll
        for (int kk = 0; kk < LP_BK / 2; kk++) {
            const int kcol = 2 * kk + lh;                // lane l holds A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]
            float a[2], b[NT];
#pragma unroll
            for (int t = 0; t < 2; t++) a[t] = As[wm * 64 + t * 32 + li][kcol];
#pragma unroll
            for (int t = 0; t < NT; t++) b[t] = Bs[wn * 32 * NT + t * 32 + li][kcol];
#pragma unroll
            for (int t = 0; t < 2; t++)
#pragma unroll
                for (int u = 0; u < NT; u++) acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b[u], acc[t][u], 0, 0, 0);
        }
        __syncthreads();
    }
#undef LP_GATHER
    // D[i][j]: j = lane & 31 (the channel: a wave-store covers 128 contiguous bytes per pixel), i = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int u = 0; u < NT; u++) {
        const int co = co0 + wn * 32 * NT + u * 32 + li;
        const float bias = p.bias[co];
#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const long long m = m0 + wm * 64 + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (m < p.M) {
                    const float v = acc[t][u][r] + bias;
                    p.y[(size_t)m * p.Cout + co] = p.relu ? fmaxf(v, 0.f) : v;
                }
            }
    }
}

struct LpView {       // value(n, c, y, x) = p[n sN + c sC + y sY + (x / Wv) sV + (x % Wv) sX]
    const float *p;
    long long sN, sC, sY, sV, sX;
    int Wv;
};

struct LpImage {
    LpView X, Y;      // images [0, B) come from X, [B, 2 B) from Y (Y.p null: all from X)
    int B;
    float mul, add, shift[3], scale[3];
    const float *w, *bias;
    float *y;
    int H, W, Cout, Ho, Wo, k, stride, pad, relu;
    long long M;
};

__global__ void __launch_bounds__(256)
lp_conv_image_kernel(const LpImage p) {
    const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
    const int co0 = blockIdx.y * LP_CO;
    if (m >= p.M) return;
    const long long hw = (long long)p.Ho * p.Wo, n = m / hw;
    const int rem = (int)(m - n * hw), oy = rem / p.Wo, ox = rem - oy * p.Wo;
    const bool second = p.Y.p != nullptr && n >= p.B;
    const LpView &v = second ? p.Y : p.X;
    const float *img = v.p + (second ? n - p.B : n) * v.sN;
    float acc[LP_CO];
#pragma unroll
    for (int c = 0; c < LP_CO; c++) acc[c] = p.bias[co0 + c];
    const size_t wrow = (size_t)p.k * p.k * 3;
    for (int kh = 0; kh < p.k; kh++) {
        const int iy = oy * p.stride - p.pad + kh;
        if (iy < 0 || iy >= p.H) continue;
        for (int kw = 0; kw < p.k; kw++) {
            const int ix = ox * p.stride - p.pad + kw;
            if (ix < 0 || ix >= p.W) continue;           // zero padding applies AFTER the scaling: the tap adds nothing
            const int xv = ix / v.Wv, xr = ix - xv * v.Wv;
            const float *px = img + iy * v.sY + xv * v.sV + xr * v.sX;
            float u[3];
#pragma unroll
            for (int c = 0; c < 3; c++) u[c] = (fmaf(px[c * v.sC], p.mul, p.add) - p.shift[c]) / p.scale[c];
            const float *wt = p.w + (size_t)co0 * wrow + (size_t)(kh * p.k + kw) * 3;      // wave-uniform
#pragma unroll
            for (int c = 0; c < LP_CO; c++) {
                acc[c] = fmaf(u[0], wt[c * wrow], acc[c]);
                acc[c] = fmaf(u[1], wt[c * wrow + 1], acc[c]);
                acc[c] = fmaf(u[2], wt[c * wrow + 2], acc[c]);
            }
        }
    }
    float4 *out = (float4 *)(p.y + (size_t)m * p.Cout + co0);
#pragma unroll
    for (int c = 0; c < LP_CO; c += 4) {
        float4 o = make_float4(acc[c], acc[c + 1], acc[c + 2], acc[c + 3]);
        if (p.relu) o = make_float4(fmaxf(o.x, 0.f), fmaxf(o.y, 0.f), fmaxf(o.z, 0.f), fmaxf(o.w, 0.f));
        out[c / 4] = o;
    }
}

__global__ void __launch_bounds__(256)
lp_maxpool_kernel(const float *__restrict__ x, float *__restrict__ y, const int H, const int W, const int C4, const int Ho,
                  const int Wo, const int k, const int s, const long long total) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const int c = (int)(g % C4);
    const long long pix = g / C4, hw = (long long)Ho * Wo, n = pix / hw;
    const int rem = (int)(pix - n * hw), oy = rem / Wo, ox = rem - oy * Wo;
    const float4 *src = (const float4 *)x + ((size_t)n * H * W) * C4 + c;
    float4 m = src[((size_t)(oy * s) * W + ox * s) * C4];      // floor mode: every window lies inside the image
    for (int dy = 0; dy < k; dy++)
        for (int dx = 0; dx < k; dx++) {
            const float4 v = src[((size_t)(oy * s + dy) * W + ox * s + dx) * C4];
            m = make_float4(fmaxf(m.x, v.x), fmaxf(m.y, v.y), fmaxf(m.z, v.z), fmaxf(m.w, v.w));
        }
    ((float4 *)y)[g] = m;
}

// partial[b * gridDim.x + block] = sum over the block's pixels of sum_c lin[c] (f0 / (|f0| + eps) - f1 / (|f1| + eps))^2
__global__ void __launch_bounds__(256)
lp_dist_kernel(const float *__restrict__ F, const int B, const long long HW, const int C, const float *__restrict__ lin,
               double *__restrict__ partial) {
    __shared__ double red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y, nj = C >> 6;
    const float *f0 = F + (size_t)b * HW * C, *f1 = F + (size_t)(B + b) * HW * C;
    float wl[LP_MAXC / 64];
#pragma unroll
    for (int j = 0; j < LP_MAXC / 64; j++) wl[j] = j < nj ? lin[lane + 64 * j] : 0.f;
    double acc = 0.0;
    const long long first = (long long)blockIdx.x * LP_DPIX + wave * (LP_DPIX / 4);
    for (int i = 0; i < LP_DPIX / 4; i++) {
        const long long pix = first + i;
        if (pix >= HW) break;                            // (wave-uniform)
        float a[LP_MAXC / 64], c[LP_MAXC / 64], sa = 0.f, sc = 0.f;
#pragma unroll
        for (int j = 0; j < LP_MAXC / 64; j++) {
            a[j] = j < nj ? f0[(size_t)pix * C + lane + 64 * j] : 0.f;
            c[j] = j < nj ? f1[(size_t)pix * C + lane + 64 * j] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < LP_MAXC / 64; j++) { sa = fmaf(a[j], a[j], sa); sc = fmaf(c[j], c[j], sc); }
        const float na = sqrtf(wave_sum(sa)) + 1e-10f, nc = sqrtf(wave_sum(sc)) + 1e-10f;
        float t = 0.f;
#pragma unroll
        for (int j = 0; j < LP_MAXC / 64; j++) {
            const float d = a[j] / na - c[j] / nc;
            t = fmaf(wl[j], d * d, t);
        }
        acc += (double)t;
    }
    acc = wave_sum(acc);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[(size_t)b * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

struct LpFinish {
    long long off[LARA_LPIPS_TAPS];      // first partial of tap k (of scene 0), in doubles
    int blocks[LARA_LPIPS_TAPS];
    double inv_pixels[LARA_LPIPS_TAPS];
};

__global__ void __launch_bounds__(256)
lp_finish_kernel(const double *__restrict__ partial, const LpFinish f, double *__restrict__ scores) {
    __shared__ double red[256];
    __shared__ double term[LARA_LPIPS_TAPS];
    const int b = blockIdx.x, tid = threadIdx.x;
    for (int k = 0; k < LARA_LPIPS_TAPS; k++) {
        const double *src = partial + f.off[k] + (size_t)b * f.blocks[k];
        double s = 0.0;
        for (int i = tid; i < f.blocks[k]; i += 256) s += src[i];
        red[tid] = s;
        __syncthreads();
        for (int d = 128; d > 0; d >>= 1) {
            if (tid < d) red[tid] += red[tid + d];
            __syncthreads();
        }
        if (tid == 0) term[k] = red[0] * f.inv_pixels[k];
        __syncthreads();
    }
    if (tid == 0) {
        double *row = scores + (size_t)b * LARA_LPIPS_ROW;
        double total = 0.0;
        for (int k = 0; k < LARA_LPIPS_TAPS; k++) { row[k] = term[k]; total += term[k]; }
        row[5] = total;
        row[6] = row[7] = 0.0;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------

int lp_out(int side, int k, int s, int pad) { return side + 2 * pad < k ? 0 : (side + 2 * pad - k) / s + 1; }
bool lp_mfma_ok(int Cin, int Cout) { return Cin > 0 && Cin % LP_BK == 0 && Cout > 0 && Cout % 64 == 0; }

struct LpPlan {      // sizes of every step of a network on [2 B, H, W] images
    int n_layers;
    int pool_h[LARA_LPIPS_MAX_LAYERS], pool_w[LARA_LPIPS_MAX_LAYERS];      // after the pool in front of layer i (= its input)
    int out_h[LARA_LPIPS_MAX_LAYERS], out_w[LARA_LPIPS_MAX_LAYERS];
    int tap_c[LARA_LPIPS_TAPS], tap_blocks[LARA_LPIPS_TAPS];
    long long tap_pixels[LARA_LPIPS_TAPS], part_off[LARA_LPIPS_TAPS];
    long long partials;       // doubles
    long long act_floats;     // the largest activation
};

bool lp_plan(const lara_lpips_net *net, int B, int H, int W, LpPlan *P) {
    if (!net || B <= 0 || B > 32767 || H <= 0 || W <= 0) return false;
    if (net->n_layers <= 0 || net->n_layers > LARA_LPIPS_MAX_LAYERS) return false;
    for (int c = 0; c < 3; c++)
        if (!(net->scale[c] != 0.0f)) return false;
    P->n_layers = net->n_layers;
    P->partials = 0;
    P->act_floats = 0;
    int h = H, w = W, ch = 3, taps = 0;
    for (int i = 0; i < net->n_layers; i++) {
        const lara_lpips_layer &L = net->layers[i];
        if (!L.w || !L.bias || L.cin != ch || L.k <= 0 || L.stride <= 0 || L.pad < 0 || L.pool_k < 0) return false;
        if (i == 0 ? (L.cin != 3 || L.cout % LP_CO != 0 || L.pool_k != 0) : !lp_mfma_ok(L.cin, L.cout)) return false;
        if (L.pool_k > 0) {
            if (L.pool_s <= 0) return false;
            h = lp_out(h, L.pool_k, L.pool_s, 0);
            w = lp_out(w, L.pool_k, L.pool_s, 0);
            if (h <= 0 || w <= 0) return false;
            const long long n = 2ll * B * h * w * ch;
            if (n > P->act_floats) P->act_floats = n;
        }
        P->pool_h[i] = h; P->pool_w[i] = w;
        h = lp_out(h, L.k, L.stride, L.pad);
        w = lp_out(w, L.k, L.stride, L.pad);
        if (h <= 0 || w <= 0) return false;
        P->out_h[i] = h; P->out_w[i] = w;
        ch = L.cout;
        const long long n = 2ll * B * h * w * ch;
        if (n > P->act_floats) P->act_floats = n;
        if (2ll * B * h * w / LP_BM * (ch / 64) >= (1ll << 31)) return false;      // 1-D grids
        if (L.tap) {
            if (taps == LARA_LPIPS_TAPS || !net->lin[taps] || ch % 64 != 0 || ch > LP_MAXC) return false;
            P->tap_c[taps] = ch;
            P->tap_pixels[taps] = (long long)h * w;
            P->tap_blocks[taps] = (int)(((long long)h * w + LP_DPIX - 1) / LP_DPIX);
            P->part_off[taps] = P->partials;
            P->partials += (long long)B * P->tap_blocks[taps];
            taps++;
        }
    }
    return taps == LARA_LPIPS_TAPS && net->layers[net->n_layers - 1].tap;
}

long long lp_align(long long x) { return (x + 255) / 256 * 256; }

bool lp_view_ok(const lara_image_view *v) {
    return v && v->p && v->Wv > 0 && v->sN >= 0 && v->sC >= 0 && v->sY >= 0 && v->sV >= 0 && v->sX >= 0;
}
LpView lp_from_c(const lara_image_view *v) {
    LpView m;
    m.p = v->p; m.sN = v->sN; m.sC = v->sC; m.sY = v->sY; m.sV = v->sV; m.sX = v->sX; m.Wv = v->Wv;
    return m;
}

int lp_launch_mfma(const LpConv &p, hipStream_t s) {
    const long long mt = (p.M + LP_BM - 1) / LP_BM;
    if (p.Cout % 128 == 0) L2D_LAUNCH_IN_SCOPE(s, lp_conv_mfma_kernel<2>, dim3((unsigned)(mt * (p.Cout / 128))), dim3(256), 0, p);
    else L2D_LAUNCH_IN_SCOPE(s, lp_conv_mfma_kernel<1>, dim3((unsigned)(mt * (p.Cout / 64))), dim3(256), 0, p);
    return LARA2DGS_OK;
}
int lp_launch_image(const LpImage &p, hipStream_t s) {
    L2D_LAUNCH_IN_SCOPE(s, lp_conv_image_kernel, dim3((unsigned)((p.M + 255) / 256), (unsigned)(p.Cout / LP_CO)), dim3(256), 0, p);
    return LARA2DGS_OK;
}
int lp_launch_pool(const float *x, float *y, int N, int H, int W, int C, int k, int st, hipStream_t s) {
    const int Ho = lp_out(H, k, st, 0), Wo = lp_out(W, k, st, 0);
    const long long total = (long long)N * Ho * Wo * (C / 4);
    L2D_LAUNCH_IN_SCOPE(s, lp_maxpool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, x, y, H, W, C / 4, Ho, Wo, k, st, total);
    return LARA2DGS_OK;
}

}  // namespace

extern "C" {

int64_t lara_lpips_workspace_bytes(const lara_lpips_net *net, int32_t B, int32_t H, int32_t W) {
    LpPlan P;
    if (!lp_plan(net, B, H, W, &P)) return LARA2DGS_E_INVALID;
    return lp_align(P.partials * 8) + 2 * lp_align(P.act_floats * 4);
}

int lara_lpips_forward(const lara_lpips_net *net, int32_t B, int32_t H, int32_t W, const lara_image_view *X,
                       const lara_image_view *Y, float in_mul, float in_add, double *scores, void *workspace, void *stream) {
    LpPlan P;
    if (!lp_plan(net, B, H, W, &P) || !lp_view_ok(X) || !lp_view_ok(Y) || !scores || !workspace) return LARA2DGS_E_INVALID;
    if (((uintptr_t)workspace & 255) != 0) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    double *partial = (double *)workspace;
    float *buf[2];
    buf[0] = (float *)((char *)workspace + lp_align(P.partials * 8));
    buf[1] = (float *)((char *)buf[0] + lp_align(P.act_floats * 4));
    int cur = 0, tap = 0;       // buf[cur] holds the current activation (once layer 0 has run)
    L2D_PROF("lpips_forward", s);
    for (int i = 0; i < net->n_layers; i++) {
        const lara_lpips_layer &L = net->layers[i];
        if (i == 0) {
            LpImage p;
            p.X = lp_from_c(X); p.Y = lp_from_c(Y); p.B = B; p.mul = in_mul; p.add = in_add;
            for (int c = 0; c < 3; c++) { p.shift[c] = net->shift[c]; p.scale[c] = net->scale[c]; }
            p.w = L.w; p.bias = L.bias; p.y = buf[cur];
            p.H = H; p.W = W; p.Cout = L.cout; p.Ho = P.out_h[0]; p.Wo = P.out_w[0]; p.k = L.k; p.stride = L.stride; p.pad = L.pad; p.relu = 1;
            p.M = 2ll * B * p.Ho * p.Wo;
            L2D_TRY(lp_launch_image(p, s));
        } else {
            if (L.pool_k > 0) {
                L2D_TRY(lp_launch_pool(buf[cur], buf[cur ^ 1], 2 * B, P.out_h[i - 1], P.out_w[i - 1], L.cin, L.pool_k, L.pool_s, s));
                cur ^= 1;
            }
            LpConv p;
            p.x = buf[cur]; p.w = L.w; p.bias = L.bias; p.y = buf[cur ^ 1];
            p.H = P.pool_h[i]; p.W = P.pool_w[i]; p.Cin = L.cin; p.Cout = L.cout; p.Ho = P.out_h[i]; p.Wo = P.out_w[i];
            p.k = L.k; p.stride = L.stride; p.pad = L.pad; p.relu = 1;
            p.M = 2ll * B * p.Ho * p.Wo;
            L2D_TRY(lp_launch_mfma(p, s));
            cur ^= 1;
        }
        if (L.tap) {
            L2D_LAUNCH_IN_SCOPE(s, lp_dist_kernel, dim3((unsigned)P.tap_blocks[tap], (unsigned)B), dim3(256), 0, (const float *)buf[cur], B,
                                P.tap_pixels[tap], P.tap_c[tap], net->lin[tap], partial + P.part_off[tap]);
            tap++;
        }
    }
    LpFinish f;
    for (int k = 0; k < LARA_LPIPS_TAPS; k++) {
        f.off[k] = P.part_off[k];
        f.blocks[k] = P.tap_blocks[k];
        f.inv_pixels[k] = 1.0 / (double)P.tap_pixels[k];
    }
    L2D_LAUNCH_IN_SCOPE(s, lp_finish_kernel, dim3((unsigned)B), dim3(256), 0, (const double *)partial, f, scores);
    return LARA2DGS_OK;
}

int lara_lpips_conv2d(int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t k, int32_t stride, int32_t pad,
                      int32_t relu, const float *x, const float *w, const float *bias, float *y, void *stream) {
    if (N <= 0 || H <= 0 || W <= 0 || k <= 0 || stride <= 0 || pad < 0 || !x || !w || !bias || !y) return LARA2DGS_E_INVALID;
    const int Ho = lp_out(H, k, stride, pad), Wo = lp_out(W, k, stride, pad);
    if (Ho <= 0 || Wo <= 0) return LARA2DGS_E_INVALID;
    const long long M = (long long)N * Ho * Wo;
    if (M / LP_BM * (Cout / 64 + 1) >= (1ll << 31)) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    L2D_PROF("lpips_conv2d", s);
    if (Cin == 3) {
        if (Cout <= 0 || Cout % LP_CO != 0) return LARA2DGS_E_INVALID;
        LpImage p;
        p.X.p = x; p.X.sN = (long long)H * W * 3; p.X.sC = 1; p.X.sY = (long long)W * 3; p.X.sV = 0; p.X.sX = 3; p.X.Wv = W;
        p.Y = p.X; p.Y.p = nullptr; p.B = N; p.mul = 1.f; p.add = 0.f;
        for (int c = 0; c < 3; c++) { p.shift[c] = 0.f; p.scale[c] = 1.f; }
        p.w = w; p.bias = bias; p.y = y;
        p.H = H; p.W = W; p.Cout = Cout; p.Ho = Ho; p.Wo = Wo; p.k = k; p.stride = stride; p.pad = pad; p.relu = relu;
        p.M = M;
        L2D_TRY(lp_launch_image(p, s));
    } else {
        if (!lp_mfma_ok(Cin, Cout)) return LARA2DGS_E_INVALID;
        const LpConv p{x, w, bias, y, H, W, Cin, Cout, Ho, Wo, k, stride, pad, relu, M};
        L2D_TRY(lp_launch_mfma(p, s));
    }
    return LARA2DGS_OK;
}

int lara_lpips_maxpool(int32_t N, int32_t H, int32_t W, int32_t C, int32_t k, int32_t s, const float *x, float *y, void *stream) {
    if (N <= 0 || C <= 0 || C % 4 != 0 || k <= 0 || s <= 0 || H < k || W < k || !x || !y) return LARA2DGS_E_INVALID;
    L2D_PROF("lpips_maxpool", (hipStream_t)stream);
    L2D_TRY(lp_launch_pool(x, y, N, H, W, C, k, s, (hipStream_t)stream));
    return LARA2DGS_OK;
}

}  // extern "C"
