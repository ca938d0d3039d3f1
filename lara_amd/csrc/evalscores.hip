// evalscores.hip -- what LaRa's evaluation loop computes per scene behind the forward (evaluation.py:75-111, :131-135) on gfx950:
// squared colour error + single-scale SSIM of the render against the targets, the masked depth scores, and the uint8 frames of
// the turntable video.  Interface, layouts and formulas in include/lara_eval.h.
//
//   eval_image_kernel     tile 32 x 32 of the SSIM map from a 42 x 42 input tile (10-pixel halo) in LDS, the three channels one
//                         after the other (the channel-last lines of the second and third channel hit L2: see msssim.hip, whose
//                         register-blocked separable filter this is); the squared error of the pixels the tile OWNS (every pixel
//                         of the strip belongs to exactly one tile) is taken from the same loads.  Per-workgroup partials, double.
//   eval_depth_kernel     streaming pass over [B, H, V*W]: masked count, sum |pred - gt|, counts below the thresholds.
//   eval_finish_kernel    one workgroup per scene adds the partials in a fixed order -> scores[b][16].
//   eval_quantize_kernel  float maps -> uint8 frames, four pixels per thread where the layout allows 16-byte accesses.
// No atomics: a call is bit-reproducible and a scene's row does not depend on the batch it is in.  HBM-bound: the image pass
// needs 24 bytes per pixel (two images, three floats), the depth pass 9 or 12.
#include "common.h"
#include "wave.h"
#include "../../include/lara_eval.h"

namespace {

constexpr int EV_WIN = 11, EV_T = 32, EV_IN = EV_T + EV_WIN - 1;      // 42
constexpr int EV_SW = EV_IN + 2, EV_HW = EV_T + 4;                    // LDS row lengths (floats): 44 and 36 (aligned float4 rows)
constexpr int EV_DPIX = 1024;                                         // depth pixels per workgroup (4 per thread)
constexpr int EV_DQ = 2 + LARA_EVAL_MAX_THRESHOLDS;                   // depth partials per workgroup
constexpr int EV_IQ = 4;                                              // image partials per workgroup: sq. error, ssim of 3 channels

struct EvWin { float w[EV_WIN]; };
struct EvShift { float half, k1, k0; };      // s/2, (s - 1)/2, s (s - 1)/4 for the window sum s (see eval_image_kernel)

struct EvView {       // value(n, c, y, x) = p[n sN + c sC + y sY + (x / Wv) sV + (x % Wv) sX]; offsets < 2^31 (checked)
    const float *p;
    int sN, sC, sY, sV, sX;
    int Wv;
};
// x >= x_of_v_base where v_base = x_of_v_base / Wv was divided once per tile: at most a few view crossings inside a tile
__device__ __forceinline__ int ev_at(const EvView &v, const int n, const int c, const int y, const int x, const int v_base,
                                     const int x_of_v_base) {
    int xv = v_base, xr = x - x_of_v_base;
    while (xr >= v.Wv) { xr -= v.Wv; xv++; }
    return n * v.sN + c * v.sC + y * v.sY + xv * v.sV + xr * v.sX;
}

// partial[(n * tiles + tile) * 4 + {0: sum (x - y)^2 over the owned pixels of all channels, 1 + c: sum of channel c's SSIM map}]
__global__ void __launch_bounds__(256)
eval_image_kernel(const EvView X, const EvView Y, const int H, const int W, const EvWin win, const EvShift sh, const float C1,
                  const float C2, double *__restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float sx[EV_IN][EV_SW], sy[EV_IN][EV_SW];
    __shared__ __attribute__((aligned(16))) float hh[5][EV_IN][EV_HW];
    __shared__ double red[EV_IQ][4];
    const int tid = threadIdx.x, n = blockIdx.z;
    const int ty0 = blockIdx.y * EV_T, tx0 = blockIdx.x * EV_T;
    const int Hb = H - (EV_WIN - 1), Wb = W - (EV_WIN - 1);
    const int vb = tx0 / X.Wv, vbx = vb * X.Wv;      // (X and Y share Wv: checked by the host)
    // a pixel of the strip is owned by the tile whose 32 x 32 block holds it; the last tile of a row / column also owns the
    // halo behind its block (the last block reaches Hb, so its 42 input rows reach H)
    const bool last_y = blockIdx.y + 1 == gridDim.y, last_x = blockIdx.x + 1 == gridDim.x;
    double sq = 0.0;
    for (int c = 0; c < 3; c++) {
    if (c) __syncthreads();
    {   // all of a thread's loads in flight before the first is used
        constexpr int NL = (EV_IN * EV_SW + 255) / 256;
        float lx[NL], ly[NL];
#pragma unroll
        for (int k = 0; k < NL; k++) {
            const int idx = tid + 256 * k, r = idx / EV_SW, cc = idx - r * EV_SW, y = ty0 + r, x = tx0 + cc;
            const bool in = idx < EV_IN * EV_SW && cc < EV_IN && y < H && x < W;
            lx[k] = in ? X.p[ev_at(X, n, c, y, x, vb, vbx)] : 0.5f;
            ly[k] = in ? Y.p[ev_at(Y, n, c, y, x, vb, vbx)] : 0.5f;
        }
        float e = 0.f;
#pragma unroll
        for (int k = 0; k < NL; k++) {
            const int idx = tid + 256 * k, r = idx / EV_SW, cc = idx - r * EV_SW;
            const bool own = idx < EV_IN * EV_SW && cc < EV_IN && ty0 + r < H && tx0 + cc < W && (r < EV_T || last_y) &&
                             (cc < EV_T || last_x);
            const float d = lx[k] - ly[k];
            e += own ? d * d : 0.f;
            // the filter runs on the values minus 1/2 (include/lara_eval.h); outside the strip: 0 (never reaches a valid output)
            if (idx < EV_IN * EV_SW) { sx[r][cc] = lx[k] - 0.5f; sy[r][cc] = ly[k] - 0.5f; }
        }
        sq += (double)e;
    }
    __syncthreads();
    for (int item = tid; item < EV_IN * (EV_T / 4); item += 256) {      // along the row: 4 outputs from 14 inputs
        const int r = item >> 3, c0 = (item & 7) * 4;
        float xv[16], yv[16];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const float4 a = *(const float4 *)&sx[r][c0 + 4 * q], b = *(const float4 *)&sy[r][c0 + 4 * q];
            xv[4 * q] = a.x; xv[4 * q + 1] = a.y; xv[4 * q + 2] = a.z; xv[4 * q + 3] = a.w;
            yv[4 * q] = b.x; yv[4 * q + 1] = b.y; yv[4 * q + 2] = b.z; yv[4 * q + 3] = b.w;
        }
        float o[5][4];
#pragma unroll
        for (int m = 0; m < 5; m++)
#pragma unroll
            for (int e = 0; e < 4; e++) o[m][e] = 0.f;
#pragma unroll
        for (int k = 0; k < 14; k++) {
            const float x1 = xv[k], y1 = yv[k], xx = x1 * x1, yy = y1 * y1, xy = x1 * y1;
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int t = k - e;
                if (t >= 0 && t < EV_WIN) {
                    const float w = win.w[t];
                    o[0][e] += w * x1; o[1][e] += w * y1; o[2][e] += w * xx; o[3][e] += w * yy; o[4][e] += w * xy;
                }
            }
        }
#pragma unroll
        for (int m = 0; m < 5; m++) *(float4 *)&hh[m][r][c0] = make_float4(o[m][0], o[m][1], o[m][2], o[m][3]);
    }
    __syncthreads();
    double s_ssim = 0.0;
    {                                                                   // down the column: 4 outputs from 14 rows, per map
        const int cc = tid & 31, r0 = (tid >> 5) * 4;
        float v[5][4];
#pragma unroll
        for (int m = 0; m < 5; m++) {
            float hv[14];
#pragma unroll
            for (int k = 0; k < 14; k++) hv[k] = hh[m][r0 + k][cc];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                float a = 0.f;
#pragma unroll
                for (int t = 0; t < EV_WIN; t++) a += win.w[t] * hv[e + t];
                v[m][e] = a;
            }
        }
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const bool valid = ty0 + r0 + e < Hb && tx0 + cc < Wb;
            // the filtered x - 1/2, y - 1/2 and their products back to those of x, y: with s = the 2-D window's sum (1 + 6e-8
            // for the fp32 taps) mu = m + s/2, and E[x y] - mu_x mu_y = (E[x' y'] - m_x m_y) - (s - 1)/2 (m_x + m_y) - s (s - 1)/4
            const float m1 = v[0][e], m2 = v[1][e];
            const float sxy = (v[4][e] - m1 * m2) - sh.k1 * (m1 + m2) - sh.k0;
            const float sxx = (v[2][e] - m1 * m1) - 2.0f * sh.k1 * m1 - sh.k0, syy = (v[3][e] - m2 * m2) - 2.0f * sh.k1 * m2 - sh.k0;
            const float A2 = 2.0f * sxy + C2, B2 = sxx + syy + C2;
            const float mu1 = m1 + sh.half, mu2 = m2 + sh.half;
            const float A1 = 2.0f * (mu1 * mu2) + C1, B1 = mu1 * mu1 + mu2 * mu2 + C1;
            const float ssim = (A1 / B1) * (A2 / B2);
            s_ssim += valid ? (double)ssim : 0.0;
        }
    }
    s_ssim = wave_sum(s_ssim);
    if ((tid & 63) == 0) red[1 + c][tid >> 6] = s_ssim;
    }   // channels
    sq = wave_sum(sq);
    if ((tid & 63) == 0) red[0][tid >> 6] = sq;
    __syncthreads();
    if (tid < EV_IQ) {
        const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x, tiles = (size_t)gridDim.x * gridDim.y;
        partial[((size_t)n * tiles + tile) * EV_IQ + tid] = ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
    }
}

struct EvDepth {
    int V, H, W;               // pixels of a scene: H * V * W  (< 2^31 for the whole batch: checked)
    const float *pred, *gt;
    const void *msk;
    int msk_bytes, n_thr;
    float thr[LARA_EVAL_MAX_THRESHOLDS];
};

// partial[(b * blocks + block) * EV_DQ + {0: masked pixels, 1: sum |pred - gt|, 2 + k: |pred - gt| < thr[k]}]
__global__ void __launch_bounds__(256)
eval_depth_kernel(const EvDepth p, double *__restrict__ partial) {
    __shared__ double red[EV_DQ][4];
    const int b = blockIdx.y, vw = p.V * p.W, npix = p.H * vw;
    int cnt = 0, below[LARA_EVAL_MAX_THRESHOLDS];
    double sum = 0.0;
#pragma unroll
    for (int k = 0; k < LARA_EVAL_MAX_THRESHOLDS; k++) below[k] = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int i = blockIdx.x * EV_DPIX + j * 256 + threadIdx.x;
        if (i >= npix) continue;
        const int y = i / vw, col = i - y * vw, v = col / p.W, x = col - v * p.W;
        const size_t t = (((size_t)b * p.V + v) * p.H + y) * p.W + x;
        const bool inside = p.msk_bytes == 1 ? ((const uint8_t *)p.msk)[t] != 0 : ((const float *)p.msk)[t] != 0.0f;
        if (!inside) continue;
        const float d = fabsf(p.pred[(size_t)b * npix + i] - p.gt[t]);
        cnt++;
        sum += (double)d;
#pragma unroll
        for (int k = 0; k < LARA_EVAL_MAX_THRESHOLDS; k++) below[k] += (k < p.n_thr && d < p.thr[k]) ? 1 : 0;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    cnt = wave_sum(cnt);
    sum = wave_sum(sum);
#pragma unroll
    for (int k = 0; k < LARA_EVAL_MAX_THRESHOLDS; k++) below[k] = wave_sum(below[k]);
    if (lane == 0) {
        red[0][wave] = (double)cnt;
        red[1][wave] = sum;
#pragma unroll
        for (int k = 0; k < LARA_EVAL_MAX_THRESHOLDS; k++) red[2 + k][wave] = (double)below[k];
    }
    __syncthreads();
    if (threadIdx.x < EV_DQ) {
        const int q = threadIdx.x;
        partial[((size_t)b * gridDim.x + blockIdx.x) * EV_DQ + q] = ((red[q][0] + red[q][1]) + red[q][2]) + red[q][3];
    }
}

// scores[b][:] from the scene's partials, added in a fixed order (thread t: items t, t + 256, ...; then a tree over the threads)
__global__ void __launch_bounds__(256)
eval_finish_kernel(const double *__restrict__ img_partial, const int tiles, const double img_elems, const double inv_map,
                   const double *__restrict__ dep_partial, const int blocks, double *__restrict__ scores) {
    __shared__ double red[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    double *row = scores + (size_t)b * LARA_EVAL_ROW;
    for (int q = 0; q < EV_IQ + EV_DQ; q++) {
        const bool img = q < EV_IQ;
        const double *src = img ? img_partial : dep_partial;
        const int items = img ? tiles : blocks, Q = img ? EV_IQ : EV_DQ, qq = img ? q : q - EV_IQ;
        double s = 0.0;
        if (src)
            for (int k = tid; k < items; k += 256) s += src[((size_t)b * items + k) * Q + qq];
        red[tid] = s;
        __syncthreads();
        for (int d = 128; d > 0; d >>= 1) {
            if (tid < d) red[tid] += red[tid + d];
            __syncthreads();
        }
        if (tid == 0) {
            const double total = red[0];
            if (q == 0) { row[0] = total; row[1] = src ? img_elems : 0.0; }
            else if (img) row[1 + q] = src ? total * inv_map : 0.0;
            else row[5 + qq] = total;
        }
        __syncthreads();
    }
    if (tid == 0) row[15] = 0.0;
}

__device__ __forceinline__ uint32_t ev_u8(const float v) {      // rint: ties to even, as np.round
    return (uint32_t)fminf(fmaxf(__builtin_rintf(v), 0.0f), 255.0f);
}
__device__ __forceinline__ uint32_t ev_colour(const float x) { return ev_u8(x * 255.0f); }
// (((n * a + 1 - a) + 1) / 2) * 255 as that sequence of fp32 operations (evaluation.py:135): the multiply must not fuse into the
// add behind it (the pragma travels with the instructions when this is inlined; the build's ISA holds no fma in this kernel)
__device__ __forceinline__ uint32_t ev_normal(const float nrm, const float a) {
#pragma clang fp contract(off)
    float t = nrm * a;
    t = t + 1.0f;
    t = t - a;
    t = t + 1.0f;
    t = t * 0.5f;
    return ev_u8(t * 255.0f);
}

struct EvQuant {
    int n, H, W;
    long long sV, sY;          // pixel strides of the inputs
    const float *image, *normal, *acc;
    uint8_t *frames, *nframes;
};

// VEC = 4: W % 4 == 0 and every pointer / stride allows float4 loads and uint32 stores of four pixels (12 floats in, 12 bytes out)
template <int VEC>
__global__ void __launch_bounds__(256)
eval_quantize_kernel(const EvQuant p) {
    const unsigned g = blockIdx.x * 256u + threadIdx.x, wg = (unsigned)(p.W / VEC), total = (unsigned)p.n * p.H * wg;   // < 2^31 (checked)
    if (g >= total) return;
    const unsigned row = g / wg;                                    // v * H + y
    const int x = (int)(g - row * wg) * VEC, v = (int)(row / (unsigned)p.H), y = (int)(row - (unsigned)v * p.H);
    const long long in = (long long)v * p.sV + (long long)y * p.sY + x, out = ((long long)row * p.W + x) * 3;
    if (VEC == 4) {
        if (p.frames) {
            const float4 *s = (const float4 *)(p.image + in * 3);
            const float4 a = s[0], b = s[1], c = s[2];
            uint32_t *d = (uint32_t *)(p.frames + out);
            d[0] = ev_colour(a.x) | ev_colour(a.y) << 8 | ev_colour(a.z) << 16 | ev_colour(a.w) << 24;
            d[1] = ev_colour(b.x) | ev_colour(b.y) << 8 | ev_colour(b.z) << 16 | ev_colour(b.w) << 24;
            d[2] = ev_colour(c.x) | ev_colour(c.y) << 8 | ev_colour(c.z) << 16 | ev_colour(c.w) << 24;
        }
        if (p.nframes) {
            const float4 *s = (const float4 *)(p.normal + in * 3);
            const float4 a = s[0], b = s[1], c = s[2], al = *(const float4 *)(p.acc + in);
            uint32_t *d = (uint32_t *)(p.nframes + out);
            d[0] = ev_normal(a.x, al.x) | ev_normal(a.y, al.x) << 8 | ev_normal(a.z, al.x) << 16 | ev_normal(a.w, al.y) << 24;
            d[1] = ev_normal(b.x, al.y) | ev_normal(b.y, al.y) << 8 | ev_normal(b.z, al.z) << 16 | ev_normal(b.w, al.z) << 24;
            d[2] = ev_normal(c.x, al.z) | ev_normal(c.y, al.w) << 8 | ev_normal(c.z, al.w) << 16 | ev_normal(c.w, al.w) << 24;
        }
    } else {
        if (p.frames)
#pragma unroll
            for (int c = 0; c < 3; c++) p.frames[out + c] = (uint8_t)ev_colour(p.image[in * 3 + c]);
        if (p.nframes) {
            const float al = p.acc[in];
#pragma unroll
            for (int c = 0; c < 3; c++) p.nframes[out + c] = (uint8_t)ev_normal(p.normal[in * 3 + c], al);
        }
    }
}

// (element offsets are 32-bit in the image kernel: the largest offset a view can produce must stay below 2^31)
bool ev_view_ok(const lara_image_view *v, int N, int H, int W) {
    if (!v || !v->p || v->Wv <= 0 || v->sN < 0 || v->sC < 0 || v->sY < 0 || v->sV < 0 || v->sX < 0) return false;
    const long long top = (long long)(N - 1) * v->sN + 2 * v->sC + (long long)(H - 1) * v->sY + (long long)((W - 1) / v->Wv) * v->sV +
                          (long long)(v->Wv - 1) * v->sX;
    return top < (1ll << 31);
}
EvView ev_from_c(const lara_image_view *v) {
    EvView m;
    m.p = v->p; m.sN = (int)v->sN; m.sC = (int)v->sC; m.sY = (int)v->sY; m.sV = (int)v->sV; m.sX = (int)v->sX; m.Wv = v->Wv;
    return m;
}
int ev_tiles(int side) { return (side - (EV_WIN - 1) + EV_T - 1) / EV_T; }
bool ev_image_dims_ok(int H, int W) { return H >= EV_WIN && W >= EV_WIN && (long long)ev_tiles(H) <= 65535; }
bool ev_depth_dims_ok(int B, int V, int H, int W) {
    return V > 0 && H > 0 && W > 0 && (long long)B * V * H * W < (1ll << 31) && B <= 65535;
}
int ev_depth_blocks(int V, int H, int W) { return (int)(((long long)V * H * W + EV_DPIX - 1) / EV_DPIX); }
constexpr float EV_C1 = 0.01f * 0.01f, EV_C2 = 0.03f * 0.03f;

}  // namespace

extern "C" {

int64_t lara_eval_workspace_doubles(int32_t B, int32_t H, int32_t W, int32_t Vd, int32_t Hd, int32_t Wd) {
    if (B <= 0 || B > 65535) return LARA2DGS_E_INVALID;
    int64_t n = 0;
    if (H > 0 || W > 0) {
        if (!ev_image_dims_ok(H, W)) return LARA2DGS_E_INVALID;
        n += (int64_t)B * ev_tiles(H) * ev_tiles(W) * EV_IQ;
    }
    if (Vd > 0 || Hd > 0 || Wd > 0) {
        if (!ev_depth_dims_ok(B, Vd, Hd, Wd)) return LARA2DGS_E_INVALID;
        n += (int64_t)B * ev_depth_blocks(Vd, Hd, Wd) * EV_DQ;
    }
    return n + 1;
}

int lara_eval_scores(int32_t B, int32_t H, int32_t W, const lara_image_view *X, const lara_image_view *Y, const float *window11,
                     int32_t Vd, int32_t Hd, int32_t Wd, const float *depth_pred, const float *tar_dep, const void *tar_msk,
                     int32_t msk_elem_bytes, int32_t n_thr, const double *thresholds, double *scores, double *workspace,
                     void *stream) {
    if (B <= 0 || B > 65535 || !scores || !workspace) return LARA2DGS_E_INVALID;
    if (n_thr < 0 || n_thr > LARA_EVAL_MAX_THRESHOLDS || (n_thr > 0 && !thresholds)) return LARA2DGS_E_INVALID;
    const bool image = X != nullptr, depth = depth_pred && tar_dep && tar_msk;
    if (image) {
        if (!ev_image_dims_ok(H, W)) return LARA2DGS_E_INVALID;        // (a side below 11 holds no window)
        if (!Y || !window11 || !ev_view_ok(X, B, H, W) || !ev_view_ok(Y, B, H, W) || X->Wv != Y->Wv) return LARA2DGS_E_INVALID;
    }
    if (depth && (!ev_depth_dims_ok(B, Vd, Hd, Wd) || (msk_elem_bytes != 1 && msk_elem_bytes != 4))) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const int tx = image ? ev_tiles(W) : 0, ty = image ? ev_tiles(H) : 0, tiles = tx * ty;
    const int blocks = depth ? ev_depth_blocks(Vd, Hd, Wd) : 0;
    double *img_partial = workspace, *dep_partial = workspace + (size_t)B * tiles * EV_IQ;
    L2D_PROF("eval_scores", s);
    if (image) {
        EvWin win;
        double w1 = 0.0;
        for (int t = 0; t < EV_WIN; t++) { win.w[t] = window11[t]; w1 += (double)window11[t]; }
        const double ws = w1 * w1;
        const EvShift sh{(float)(0.5 * ws), (float)(0.5 * (ws - 1.0)), (float)(0.25 * ws * (ws - 1.0))};
        L2D_LAUNCH_IN_SCOPE(s, eval_image_kernel, dim3(tx, ty, (unsigned)B), dim3(256), 0, ev_from_c(X), ev_from_c(Y), H, W, win, sh,
                            EV_C1, EV_C2, img_partial);
    }
    if (depth) {
        EvDepth p;
        p.V = Vd; p.H = Hd; p.W = Wd; p.pred = depth_pred; p.gt = tar_dep; p.msk = tar_msk; p.msk_bytes = msk_elem_bytes; p.n_thr = n_thr;
        for (int k = 0; k < LARA_EVAL_MAX_THRESHOLDS; k++) p.thr[k] = k < n_thr ? (float)thresholds[k] : 0.0f;
        L2D_LAUNCH_IN_SCOPE(s, eval_depth_kernel, dim3(blocks, (unsigned)B), dim3(256), 0, p, dep_partial);
    }
    L2D_LAUNCH_IN_SCOPE(s, eval_finish_kernel, dim3((unsigned)B), dim3(256), 0, image ? (const double *)img_partial : (const double *)nullptr,
                        tiles, 3.0 * (double)H * (double)W,
                        image ? 1.0 / ((double)(H - (EV_WIN - 1)) * (double)(W - (EV_WIN - 1))) : 0.0,
                        depth ? (const double *)dep_partial : (const double *)nullptr, blocks, scores);
    return LARA2DGS_OK;
}

int lara_eval_quantize_frames(int32_t n, int32_t H, int32_t W, int64_t pix_sV, int64_t pix_sY, const float *image,
                              const float *rend_normal, const float *acc_map, uint8_t *frames, uint8_t *normal_frames,
                              void *stream) {
    if (n < 0 || H <= 0 || W <= 0 || pix_sV < 0 || pix_sY < 0) return LARA2DGS_E_INVALID;
    if ((frames && !image) || (normal_frames && (!rend_normal || !acc_map))) return LARA2DGS_E_INVALID;
    const long long pixels = (long long)n * H * W;
    if (pixels == 0 || (!frames && !normal_frames)) return LARA2DGS_OK;
    if (pixels >= (1ll << 31)) return LARA2DGS_E_INVALID;      // (32-bit pixel indices in the kernel; a caller chunks its views)
    hipStream_t s = (hipStream_t)stream;
    const EvQuant p{n, H, W, pix_sV, pix_sY, image, rend_normal, acc_map, frames, normal_frames};
    const auto al = [](const void *q, uintptr_t a) { return ((uintptr_t)q & (a - 1)) == 0; };
    const bool vec = W % 4 == 0 && pix_sV % 4 == 0 && pix_sY % 4 == 0 && al(image, 16) && al(rend_normal, 16) && al(acc_map, 16) &&
                     al(frames, 4) && al(normal_frames, 4);
    L2D_PROF("eval_quantize", s);
    if (vec) L2D_LAUNCH_IN_SCOPE(s, eval_quantize_kernel<4>, dim3((unsigned)((pixels / 4 + 255) / 256)), dim3(256), 0, p);
    else L2D_LAUNCH_IN_SCOPE(s, eval_quantize_kernel<1>, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, p);
    return LARA2DGS_OK;
}

}  // extern "C"
