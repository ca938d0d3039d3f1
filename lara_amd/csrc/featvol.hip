// featvol.hip -- LaRa's image-feature volume (lightning/network.py:352-379 + :448-452): ray features -> ModLN -> projection of the
// R^3 volume grid -> bilinear sample of the modulated map, in the volume layout or straight into the volume transformer's bf16
// operand; the backward as a deterministic gather (no float atomics).  include/lara_featvol.h has the formulas and the contract.
//
// Forward:  act_kernel (per token: bf16 [SiLU(ray features) | 1 | 0...], 64 wide) and wprep_kernel (bf16 [W | bias | 0...]) feed
//           ONE lara_gemm_nt_bf16 whose bf16 result is autocast's Linear output [shift | scale] (the bias rides as the K = 32
//           column, so the sum is rounded once, as the fused addmm does); modln_kernel (wave per token: LayerNorm + modulation,
//           fp32 rows [T, C]); sample_kernel (32 points x all views per block; bilinear taps of every (point, view) in LDS).
// Backward: the same Linear recomputed; index_kernel (per view: texel-keyed (point, tap) lists, counting sort with a stable
//           wave-serial placement); token_bwd_kernel (wave per token: gather dY in list order, LayerNorm backward, bf16 d[shift |
//           scale] rows, per-block gamma/beta partials); lara_gemm_tn_bf16 d[shift | scale]^T . act -> [dW | db]; the
//           view-embedding and gamma/beta partials summed in block order.
#include "common.h"
#include "mfma_gemm.h"
#include "../../include/lara_featvol.h"
#include "../../include/lara_groupattn.h"

namespace {

constexpr int FV_PTS = 32;        // points per sample_kernel block
constexpr int FV_KA = 64;         // width of the Linear's K operand: 32 features, the bias column, zeros
constexpr int FV_TOK_BLOCKS = 1024;   // token_bwd_kernel grid (its gamma / beta partial rows)
constexpr int FV_EMB_BLOCKS = 64;     // view-embedding partial rows

struct FvP {
    int B, V, C, E, h, w, R, S, hw, T, Tp;
    float img_w, img_h, eps;
    long long sx0, sx1, sx2, sx3;
    const float *x, *rays, *w2cs, *ixts, *grid, *ln_w, *ln_b, *mlp_w, *mlp_b, *embed;
};

__device__ __forceinline__ void rsh3(const float x, const float y, const float z, float *o) {
    const float x2 = x * x, y2 = y * y, z2 = z * z, xy = x * y, xz = x * z, yz = y * z;
    o[0] = 0.282094791773878f;
    o[1] = -0.48860251190292f * y;
    o[2] = 0.48860251190292f * z;
    o[3] = -0.48860251190292f * x;
    o[4] = 1.09254843059208f * xy;
    o[5] = -1.09254843059208f * yz;
    o[6] = 0.94617469575756f * z2 - 0.31539156525252f;
    o[7] = -1.09254843059208f * xz;
    o[8] = 0.54627421529604f * x2 - 0.54627421529604f * y2;
    o[9] = -0.590043589926644f * y * (3.0f * x2 - y2);
    o[10] = 2.89061144264055f * xy * z;
    o[11] = 0.304697199642977f * y * (1.5f - 7.5f * z2);
    o[12] = 1.24392110863372f * z * (1.5f * z2 - 0.5f) - 0.497568443453487f * z;
    o[13] = 0.304697199642977f * x * (1.5f - 7.5f * z2);
    o[14] = 1.44530572132028f * z * (x2 - y2);
    o[15] = -0.590043589926644f * x * (x2 - 3.0f * y2);
}

// bf16 [SiLU(f) | 1 | 0 ...] of token t (rows t >= T: zeros)
__global__ void __launch_bounds__(256) act_kernel(const FvP p, unsigned short *__restrict__ act) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= p.Tp) return;
    unsigned *row = (unsigned *)(act + (size_t)t * FV_KA);
    if (t >= p.T) {
        for (int j = 0; j < FV_KA / 2; j++) row[j] = 0u;
        return;
    }
    const float *r = p.rays + (size_t)t * 6;
    const float ox = r[0], oy = r[1], oz = r[2];
    float dx = r[3], dy = r[4], dz = r[5];
    const float den = fmaxf(sqrtf(dx * dx + dy * dy + dz * dz), 1e-12f);
    dx /= den; dy /= den; dz /= den;
    float f[32];
    rsh3(dx, dy, dz, f);
    rsh3(oy * dz - oz * dy, oz * dx - ox * dz, ox * dy - oy * dx, f + 16);
#pragma unroll
    for (int j = 0; j < 32; j += 2) {
        const float a = f[j] / (1.f + expf(-f[j])), b = f[j + 1] / (1.f + expf(-f[j + 1]));
        row[j / 2] = f2bf2(a, b);
    }
    row[16] = f2bf2(1.f, 0.f);
    for (int j = 17; j < FV_KA / 2; j++) row[j] = 0u;
}

// bf16 [W | bias | 0 ...], [2C, 64]
__global__ void __launch_bounds__(256) wprep_kernel(const FvP p, unsigned short *__restrict__ wk) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * p.C * FV_KA) return;
    const int r = i / FV_KA, j = i - r * FV_KA;
    wk[i] = j < 32 ? f2bf(p.mlp_w[(size_t)r * 32 + j]) : j == 32 ? f2bf(p.mlp_b[r]) : (unsigned short)0;
}

// the lane's channels: c = 4 lane + 256 q, q < 4 (valid while c < C)
template <bool CL>
__device__ __forceinline__ void load_x(const FvP &p, const int t, const int lane, float (&x)[4][4]) {
    const int bv = t / p.hw, pix = t - bv * p.hw, yy = pix / p.w, xx = pix - yy * p.w;
    const float *base = p.x + bv * p.sx0 + yy * p.sx2 + xx * p.sx3;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int c = 4 * lane + 256 * q;
        if (c < p.C) {
            if (CL) {
                const float4 v = *(const float4 *)(base + c);
                x[q][0] = v.x; x[q][1] = v.y; x[q][2] = v.z; x[q][3] = v.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++) x[q][i] = base[(long long)(c + i) * p.sx1];
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) x[q][i] = 0.f;
        }
    }
}

// LayerNorm statistics of the lane's row slice (two passes, as torch's reference does over the row)
__device__ __forceinline__ void ln_stats(const FvP &p, const int lane, const float (&x)[4][4], float &mean, float &rstd) {
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int i = 0; i < 4; i++) s += x[q][i];
    mean = wave_sum(s) / (float)p.C;
    float v = 0.f;
#pragma unroll
    for (int q = 0; q < 4; q++)
        if (4 * lane + 256 * q < p.C)
#pragma unroll
            for (int i = 0; i < 4; i++) v += (x[q][i] - mean) * (x[q][i] - mean);
    rstd = 1.f / sqrtf(wave_sum(v) / (float)p.C + p.eps);
}

// shift and bf16(1 + scale) of the lane's channels from the Linear's bf16 rows
__device__ __forceinline__ void load_mod(const FvP &p, const unsigned short *__restrict__ mod, const int t, const int lane,
                                         float (&sh)[4][4], float (&opm)[4][4]) {
    const unsigned short *row = mod + (size_t)t * 2 * p.C;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int c = 4 * lane + 256 * q;
        if (c < p.C) {
            const s16x4 a = *(const s16x4 *)(row + c), b = *(const s16x4 *)(row + p.C + c);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                sh[q][i] = bf2f((unsigned short)a[i]);
                opm[q][i] = bf2f(f2bf(1.f + bf2f((unsigned short)b[i])));
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) sh[q][i] = opm[q][i] = 0.f;
        }
    }
}

// y = LN(x) * bf16(1 + scale) + shift, fp32 rows [T, C]; one wave per token
template <bool CL>
__global__ void __launch_bounds__(256) modln_kernel(const FvP p, const unsigned short *__restrict__ mod, float *__restrict__ y) {
    const int lane = threadIdx.x & 63, t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= p.T) return;
    float x[4][4], sh[4][4], opm[4][4], mean, rstd;
    load_x<CL>(p, t, lane, x);
    ln_stats(p, lane, x, mean, rstd);
    load_mod(p, mod, t, lane, sh, opm);
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int c = 4 * lane + 256 * q;
        if (c >= p.C) continue;
        float o[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const float n = (x[q][i] - mean) * rstd * p.ln_w[c + i] + p.ln_b[c + i];
            o[i] = n * opm[q][i] + sh[q][i];
        }
        *(float4 *)(y + (size_t)t * p.C + c) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// Feature-map position of grid point s in view (b, v), as the reference computes it under bf16 autocast: the two matmuls of
// `projection` (network.py:182-187) on bf16 operands with bf16 results (the translation added in fp32), the division and the
// grid_sample normalisation (:359) on bf16 tensors, then grid_sample's own fp32 unnormalisation ((g + 1) size - 1) / 2.
__device__ __forceinline__ void map_pos(const FvP &p, const int bv, const int s, float &ix, float &iy) {
    const float *g = p.grid + (size_t)s * 3, *m = p.w2cs + (size_t)bv * 16, *k = p.ixts + (size_t)bv * 9;
    const float px = bfr(g[0]), py = bfr(g[1]), pz = bfr(g[2]);
    const float cx = bfr(px * bfr(m[0]) + py * bfr(m[1]) + pz * bfr(m[2])) + m[3];
    const float cy = bfr(px * bfr(m[4]) + py * bfr(m[5]) + pz * bfr(m[6])) + m[7];
    const float cz = bfr(px * bfr(m[8]) + py * bfr(m[9]) + pz * bfr(m[10])) + m[11];
    const float bx = bfr(cx), by = bfr(cy), bz = bfr(cz);
    const float qx = bfr(bx * bfr(k[0]) + by * bfr(k[1]) + bz * bfr(k[2]));
    const float qy = bfr(bx * bfr(k[3]) + by * bfr(k[4]) + bz * bfr(k[5]));
    const float qz = bfr(bx * bfr(k[6]) + by * bfr(k[7]) + bz * bfr(k[8]));
    const float gx = bfr(bfr(bfr(bfr(qx / qz) + 0.5f) / p.img_w) * 2.f) - 1.f, gy = bfr(bfr(bfr(bfr(qy / qz) + 0.5f) / p.img_h) * 2.f) - 1.f;
    ix = ((bfr(gx) + 1.f) * (float)p.w - 1.f) / 2.f;
    iy = ((bfr(gy) + 1.f) * (float)p.h - 1.f) / 2.f;
}

// tap k (0: (x0, y0), 1: (x0 + 1, y0), 2: (x0, y0 + 1), 3: (x0 + 1, y0 + 1)) of a position: texel index or -1 (outside), weight
__device__ __forceinline__ int tap(const FvP &p, const float ix, const float iy, const int k, float &wgt) {
    const float fx = floorf(ix), fy = floorf(iy);
    // (far outside, inf or nan: no tap inside)
    if (!(fx >= -2.f && fx <= (float)p.w + 1.f && fy >= -2.f && fy <= (float)p.h + 1.f)) { wgt = 0.f; return -1; }
    const int xi = (int)fx + (k & 1), yi = (int)fy + (k >> 1);
    const float x1 = fx + 1.f, y1 = fy + 1.f;
    const float wx = (k & 1) ? ix - fx : x1 - ix, wy = (k >> 1) ? iy - fy : y1 - iy;
    wgt = wx * wy;
    return (xi >= 0 && xi < p.w && yi >= 0 && yi < p.h) ? yi * p.w + xi : -1;
}

// One block = FV_PTS points of scene b, every view.  TOKENS: bf16 rows [b S + s][v][C + E], written per point (the lanes along
// the channels: 512-byte runs).  VOLUME: fp32 [b][v][c][s] through an LDS tile [256 channels][FV_PTS points], written per
// channel (the lanes along the points).
template <bool TOKENS>
__global__ void __launch_bounds__(256) sample_kernel(const FvP p, const float *__restrict__ y, void *__restrict__ out) {
    __shared__ int s_idx[8][FV_PTS][4];
    __shared__ float s_wgt[8][FV_PTS][4];
    __shared__ float s_tile[TOKENS ? 1 : 256][FV_PTS + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y, s0 = blockIdx.x * FV_PTS;
    const int npts = min(FV_PTS, p.S - s0), CE = p.C + p.E;
    for (int i = threadIdx.x; i < p.V * FV_PTS; i += 256) {
        const int v = i / FV_PTS, pt = i - v * FV_PTS;
        float ix = 0.f, iy = 0.f;
        if (pt < npts) map_pos(p, b * p.V + v, s0 + pt, ix, iy);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            float wg = 0.f;
            const int id = pt < npts ? tap(p, ix, iy, k, wg) : -1;
            s_idx[v][pt][k] = id;
            s_wgt[v][pt][k] = wg;
        }
    }
    __syncthreads();
    for (int v = 0; v < p.V; v++) {
        const float *yv = y + (size_t)(b * p.V + v) * p.hw * p.C;
        for (int q = 0; 256 * q < p.C; q++) {
            const int c = 4 * lane + 256 * q;
            for (int pt = wave; pt < FV_PTS; pt += 4) {
                if (pt >= npts || c >= p.C) continue;
                float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int id = s_idx[v][pt][k];
                    if (id < 0) continue;
                    const float wg = s_wgt[v][pt][k];
                    const float4 g = *(const float4 *)(yv + (size_t)id * p.C + c);
                    a.x += wg * g.x; a.y += wg * g.y; a.z += wg * g.z; a.w += wg * g.w;
                }
                if (TOKENS) {
                    unsigned short *o = (unsigned short *)out + ((size_t)(b * p.S + s0 + pt) * p.V + v) * CE + c;
                    *(uint2 *)o = make_uint2(f2bf2(a.x, a.y), f2bf2(a.z, a.w));
                } else {
                    const int cl = 4 * lane;
                    s_tile[cl][pt] = a.x; s_tile[cl + 1][pt] = a.y; s_tile[cl + 2][pt] = a.z; s_tile[cl + 3][pt] = a.w;
                }
            }
            if (!TOKENS) {
                __syncthreads();
                const int nc = min(256, p.C - 256 * q);
                float *o = (float *)out + ((size_t)(b * p.V + v) * CE + 256 * q) * p.S + s0;
                for (int r = threadIdx.x / FV_PTS; r < nc; r += 256 / FV_PTS) {
                    const int pt = threadIdx.x % FV_PTS;
                    if (pt < npts) o[(size_t)r * p.S + pt] = s_tile[r][pt];
                }
                __syncthreads();
            }
        }
        // view embedding (network.py:452)
        for (int i = threadIdx.x; i < p.E * FV_PTS; i += 256) {
            if (TOKENS) {
                const int pt = i / p.E, e = i - pt * p.E;
                if (pt < npts)
                    ((unsigned short *)out)[((size_t)(b * p.S + s0 + pt) * p.V + v) * CE + p.C + e] = f2bf(p.embed[v * p.E + e]);
            } else {
                const int e = i / FV_PTS, pt = i - e * FV_PTS;
                if (pt < npts) ((float *)out)[((size_t)(b * p.V + v) * CE + p.C + e) * p.S + s0 + pt] = p.embed[v * p.E + e];
            }
        }
    }
}

// ---- backward ------------------------------------------------------------------------------------------------------------------
// texel (or -1) and weight of entry e = 4 s + k of view bv: ONE out-of-line copy, so that the counting and the placement pass of
// index_kernel agree on every entry bit for bit (two inlined copies could contract their multiply-adds differently)
__device__ __attribute__((noinline)) int entry_key(const FvP &p, const int bv, const int e, float &wg) {
    float ix, iy;
    map_pos(p, bv, e >> 2, ix, iy);
    return tap(p, ix, iy, e & 3, wg);
}

// Per view (block): the 4 S (point, tap) entries grouped by texel, each texel's group in ascending entry order (s, k).
// bins [hw + 1] (exclusive starts), ents [4 S] (entry index, weight).  The placement pass recomputes every entry's texel rather than
// reading what the counting pass's other waves stored: nothing crosses between the waves but the LDS counts.
__global__ void __launch_bounds__(256) index_kernel(const FvP p, int *__restrict__ bins_all, int2 *__restrict__ ents_all) {
    __shared__ int s_cnt[LARA_FEATVOL_MAX_HW + 1];
    const int bv = blockIdx.x, n = 4 * p.S, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int *bins = bins_all + (size_t)bv * (p.hw + 1);
    int2 *ents = ents_all + (size_t)bv * n;
    for (int i = threadIdx.x; i <= p.hw; i += 256) s_cnt[i] = 0;
    __syncthreads();
    for (int e = threadIdx.x; e < n; e += 256) {
        float wg;
        const int id = entry_key(p, bv, e, wg);
        if (id >= 0) atomicAdd(&s_cnt[id], 1);      // (integer counts: the order they land in does not matter)
    }
    __syncthreads();
    if (wave == 0) {   // exclusive scan of the counts, 64-bin chunks in order; the carry passes between lanes by shuffle
        int carry = 0;
        for (int base = 0; base < p.hw; base += 64) {
            const int i = base + lane;
            const int c = i < p.hw ? s_cnt[i] : 0;
            int inc = c;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int u = __shfl_up(inc, o, 64);
                if (lane >= o) inc += u;
            }
            if (i < p.hw) { s_cnt[i] = carry + inc - c; bins[i] = carry + inc - c; }
            carry += __shfl(inc, 63, 64);
        }
        if (lane == 0) bins[p.hw] = carry;
        // stable placement, 64 entries at a time in entry order: a lane's rank among the earlier lanes of its texel.  The cursors
        // are read and advanced by different lanes of this wave: volatile, so that every access is an LDS access in program order.
        volatile int *cur = s_cnt;
        int nbits = 0;
        while ((1 << nbits) < p.hw) nbits++;
        const unsigned long long lt = (1ull << lane) - 1ull;
        for (int base = 0; base < n; base += 64) {
            const int e = base + lane;
            float wg = 0.f;
            int id = -1;
            if (e < n) id = entry_key(p, bv, e, wg);
            unsigned long long same = __ballot(id >= 0);
            for (int bt = 0; bt < nbits; bt++) {
                const unsigned long long on = __ballot(id >= 0 && ((id >> bt) & 1));
                same &= ((id >> bt) & 1) ? on : ~on;
            }
            int pos = 0;
            if (id >= 0) pos = cur[id] + __popcll(same & lt);
            __builtin_amdgcn_wave_barrier();
            if (id >= 0) {
                if (pos < n) ents[pos] = make_int2(e, __float_as_int(wg));
                if ((same >> lane) == 1ull) cur[id] = cur[id] + __popcll(same);   // the group's last lane advances the cursor
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
}

// One wave per token (tokens gw, gw + NW, ...): dY = sum over the texel's entries, in list order, of weight x dL/d(out);
// LayerNorm backward -> dx; bf16 d[shift | scale]; gamma / beta partials per block (waves added in wave order).
template <bool CL>
__global__ void __launch_bounds__(256) token_bwd_kernel(const FvP p, const unsigned short *__restrict__ mod, const int *__restrict__ bins_all,
                                                        const int2 *__restrict__ ents_all, const float *__restrict__ g,
                                                        float *__restrict__ dx, unsigned short *__restrict__ dmod,
                                                        float *__restrict__ part) {
    __shared__ float s_part[2 * LARA_FEATVOL_MAX_C];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nw = gridDim.x * 4, CE = p.C + p.E;
    float pg[4][4], pb[4][4];
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int i = 0; i < 4; i++) pg[q][i] = pb[q][i] = 0.f;
    for (int t = blockIdx.x * 4 + wave; t < p.T; t += nw) {
        const int bv = t / p.hw, pix = t - bv * p.hw, b = bv / p.V, v = bv - b * p.V;
        const int *bins = bins_all + (size_t)bv * (p.hw + 1);
        const int2 *ents = ents_all + (size_t)bv * 4 * p.S;
        float dy[4][4];
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int i = 0; i < 4; i++) dy[q][i] = 0.f;
        const int e1 = min(bins[pix + 1], 4 * p.S);      // (bounds: the lists are built to stay inside [0, 4 S))
        for (int e = max(bins[pix], 0); e < e1; e++) {
            const int2 en = ents[e];
            if ((unsigned)(en.x >> 2) >= (unsigned)p.S) continue;
            const float wg = __int_as_float(en.y);
            const float *gr = g + ((size_t)(b * p.S + (en.x >> 2)) * p.V + v) * CE;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int c = 4 * lane + 256 * q;
                if (c < p.C) {
                    const float4 gv = *(const float4 *)(gr + c);
                    dy[q][0] += wg * gv.x; dy[q][1] += wg * gv.y; dy[q][2] += wg * gv.z; dy[q][3] += wg * gv.w;
                }
            }
        }
        float x[4][4], sh[4][4], opm[4][4], mean, rstd;
        load_x<CL>(p, t, lane, x);
        ln_stats(p, lane, x, mean, rstd);
        load_mod(p, mod, t, lane, sh, opm);
        // y = n * opm + shift:  d shift = bf16(dy), d scale = bf16(dy * n), dn = dy * opm;  n = xh * gamma + beta
        float xh[4][4], dxh[4][4], s1 = 0.f, s2 = 0.f;
        unsigned short *dm = dmod + (size_t)t * 2 * p.C;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int c = 4 * lane + 256 * q;
            if (c >= p.C) {
#pragma unroll
                for (int i = 0; i < 4; i++) xh[q][i] = dxh[q][i] = 0.f;
                continue;
            }
            float dsc[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                xh[q][i] = (x[q][i] - mean) * rstd;
                const float n = xh[q][i] * p.ln_w[c + i] + p.ln_b[c + i];
                const float dn = dy[q][i] * opm[q][i];
                dsc[i] = dy[q][i] * n;
                pg[q][i] += dn * xh[q][i];
                pb[q][i] += dn;
                dxh[q][i] = dn * p.ln_w[c + i];
                s1 += dxh[q][i];
                s2 += dxh[q][i] * xh[q][i];
            }
            *(uint2 *)(dm + c) = make_uint2(f2bf2(dy[q][0], dy[q][1]), f2bf2(dy[q][2], dy[q][3]));
            *(uint2 *)(dm + p.C + c) = make_uint2(f2bf2(dsc[0], dsc[1]), f2bf2(dsc[2], dsc[3]));
        }
        s1 = wave_sum(s1) / (float)p.C;
        s2 = wave_sum(s2) / (float)p.C;
        const int yy = pix / p.w, xx = pix - yy * p.w;
        float *dbase = dx + bv * p.sx0 + yy * p.sx2 + xx * p.sx3;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int c = 4 * lane + 256 * q;
            if (c >= p.C) continue;
            float o[4];
#pragma unroll
            for (int i = 0; i < 4; i++) o[i] = rstd * (dxh[q][i] - s1 - xh[q][i] * s2);
            if (CL) *(float4 *)(dbase + c) = make_float4(o[0], o[1], o[2], o[3]);
            else
#pragma unroll
                for (int i = 0; i < 4; i++) dbase[(long long)(c + i) * p.sx1] = o[i];
        }
    }
    for (int w = 0; w < 4; w++) {   // the block's partial: waves added in order
        if (wave == w) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int c = 4 * lane + 256 * q;
                if (c >= p.C) continue;
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    s_part[c + i] = w ? s_part[c + i] + pg[q][i] : pg[q][i];
                    s_part[p.C + c + i] = w ? s_part[p.C + c + i] + pb[q][i] : pb[q][i];
                }
            }
        }
        __syncthreads();
    }
    for (int i = threadIdx.x; i < 2 * p.C; i += 256) part[(size_t)blockIdx.x * 2 * p.C + i] = s_part[i];
}

// view-embedding partials: block k sums rows [k rows_per, (k + 1) rows_per) of the B S token rows, for every (v, e)
__global__ void __launch_bounds__(256) embed_part_kernel(const FvP p, const float *__restrict__ g, float *__restrict__ part) {
    const int rows = p.B * p.S, per = (rows + gridDim.x - 1) / gridDim.x, r0 = blockIdx.x * per, r1 = min(rows, r0 + per);
    const int CE = p.C + p.E;
    for (int i = threadIdx.x; i < p.V * p.E; i += 256) {
        const int v = i / p.E, e = i - v * p.E;
        float a = 0.f;
        for (int r = r0; r < r1; r++) a += g[((size_t)r * p.V + v) * CE + p.C + e];
        part[(size_t)blockIdx.x * p.V * p.E + i] = a;
    }
}

// out[i] = sum over k < nparts of part[k][i], in k order
__global__ void __launch_bounds__(256) sum_parts_kernel(const float *__restrict__ part, const int nparts, const int width,
                                                        float *__restrict__ out0, float *__restrict__ out1, const int split) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= width) return;
    float a = 0.f;
    for (int k = 0; k < nparts; k++) a += part[(size_t)k * width + i];
    if (i < split) out0[i] = a;
    else out1[i - split] = a;
}

// [2C, 64] fp32 product -> dW [2C, 32] and db [2C] (column 32: the bias column of the operand)
__global__ void __launch_bounds__(256) split_dw_kernel(const float *__restrict__ prod, const int rows, float *__restrict__ dw, float *__restrict__ db) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * 33) return;
    const int r = i / 33, j = i - r * 33;
    if (j < 32) dw[(size_t)r * 32 + j] = prod[(size_t)r * FV_KA + j];
    else db[r] = prod[(size_t)r * FV_KA + 32];
}

// ---- workspace ----
struct FvWs { int64_t act, wk, mod, y, gt, bins, ents, dmod, part, epart, prod, tn, total; };

bool dims_ok(const lara_featvol_dims *d) {
    if (!d) return false;
    if (d->B <= 0 || d->V <= 0 || d->V > 8 || d->C < 64 || d->C > LARA_FEATVOL_MAX_C || (d->C % 64) || d->E < 0 || d->E > 256 || (d->E % 4))
        return false;
    if (d->h <= 0 || d->w <= 0 || (int64_t)d->h * d->w > LARA_FEATVOL_MAX_HW || d->R <= 0 || d->img_w <= 0 || d->img_h <= 0) return false;
    const int64_t S = (int64_t)d->R * d->R * d->R, T = (int64_t)d->B * d->V * d->h * d->w;
    if (S * 4 >= (1ll << 30) || T >= (1ll << 30) || d->B > 65535) return false;
    if ((T + 255) / 256 * 256 * 2 * d->C * 2 >= (1ll << 32)) return false;   // 32-bit operand offsets of the bf16 products
    return true;
}

FvWs ws_layout(const lara_featvol_dims *d) {
    const int64_t S = (int64_t)d->R * d->R * d->R, hw = (int64_t)d->h * d->w, BV = (int64_t)d->B * d->V, T = BV * hw;
    const int64_t Tp = (T + 255) / 256 * 256, C = d->C, CE = d->C + d->E;
    FvWs L{};
    int64_t o = 0;
    L.act = o;  o = align_up(o + Tp * FV_KA * 2, 256);
    L.wk = o;   o = align_up(o + 2 * C * FV_KA * 2, 256);
    L.mod = o;  o = align_up(o + Tp * 2 * C * 2, 256);
    const int64_t shared0 = o;
    L.y = o;    o = align_up(o + T * C * 4, 256);
    const int64_t fwd_end = o;
    o = shared0;
    L.gt = o;   o = align_up(o + (int64_t)d->B * S * d->V * CE * 4, 256);
    L.bins = o; o = align_up(o + BV * (hw + 1) * 4, 256);
    L.ents = o; o = align_up(o + BV * 4 * S * 8, 256);
    L.dmod = o; o = align_up(o + Tp * 2 * C * 2, 256);
    L.part = o; o = align_up(o + (int64_t)FV_TOK_BLOCKS * 2 * C * 4, 256);
    L.epart = o; o = align_up(o + (int64_t)FV_EMB_BLOCKS * d->V * d->E * 4 + 4, 256);
    L.prod = o; o = align_up(o + 2 * C * FV_KA * 4, 256);
    L.tn = o;   o = align_up(o + lara_gemm_tn_workspace_bytes(), 256);
    L.total = o > fwd_end ? o : fwd_end;
    return L;
}

FvP make_params(const lara_featvol_dims *d, const float *x, const float *rays, const float *w2cs, const float *ixts, const float *grid,
                const float *ln_w, const float *ln_b, const float *mlp_w, const float *mlp_b, const float *embed) {
    FvP p{};
    p.B = d->B; p.V = d->V; p.C = d->C; p.E = d->E; p.h = d->h; p.w = d->w; p.R = d->R;
    p.S = d->R * d->R * d->R; p.hw = d->h * d->w; p.T = p.B * p.V * p.hw; p.Tp = (p.T + 255) / 256 * 256;
    p.img_w = (float)d->img_w; p.img_h = (float)d->img_h; p.eps = d->eps;
    p.sx0 = d->x_stride[0]; p.sx1 = d->x_stride[1]; p.sx2 = d->x_stride[2]; p.sx3 = d->x_stride[3];
    p.x = x; p.rays = rays; p.w2cs = w2cs; p.ixts = ixts; p.grid = grid; p.ln_w = ln_w; p.ln_b = ln_b; p.mlp_w = mlp_w; p.mlp_b = mlp_b;
    p.embed = embed;
    return p;
}

// channels-last rows read as float4: unit channel stride, every other stride and the base 16-byte aligned
bool channels_last(const FvP &p, const void *x, const void *dx) {
    return p.sx1 == 1 && p.sx0 % 4 == 0 && p.sx2 % 4 == 0 && p.sx3 % 4 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)dx & 15) == 0;
}

// act, the Linear's operand and its bf16 product [shift | scale]
int linear_fwd(const FvP &p, char *ws, const FvWs &L, hipStream_t s) {
    unsigned short *act = (unsigned short *)(ws + L.act), *wk = (unsigned short *)(ws + L.wk);
    L2D_LAUNCH_IN_SCOPE(s, act_kernel, dim3((p.Tp + 255) / 256), dim3(256), 0, p, act);
    L2D_LAUNCH_IN_SCOPE(s, wprep_kernel, dim3((2 * p.C * FV_KA + 255) / 256), dim3(256), 0, p, wk);
    return lara_gemm_nt_bf16(p.Tp, 2 * p.C, FV_KA, act, wk, ws + L.mod, 0, s);
}

}  // namespace

extern "C" {

int64_t lara_featvol_workspace_bytes(const lara_featvol_dims *d) {
    if (!dims_ok(d)) return LARA2DGS_E_INVALID;
    return ws_layout(d).total;
}

int lara_featvol_forward(const lara_featvol_dims *d, const float *img_feats, const float *rays, const float *w2cs, const float *ixts,
                         const float *grid, const float *ln_w, const float *ln_b, const float *mlp_w, const float *mlp_b,
                         const float *view_embed, int32_t layout, void *out, void *workspace, void *stream) {
    if (!dims_ok(d) || (layout != LARA_FEATVOL_VOLUME && layout != LARA_FEATVOL_TOKENS)) return LARA2DGS_E_INVALID;
    if (!img_feats || !rays || !w2cs || !ixts || !grid || !ln_w || !ln_b || !mlp_w || !mlp_b || !out || !workspace) return LARA2DGS_E_INVALID;
    if (d->E > 0 && !view_embed) return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const FvP p = make_params(d, img_feats, rays, w2cs, ixts, grid, ln_w, ln_b, mlp_w, mlp_b, view_embed);
    const FvWs L = ws_layout(d);
    char *ws = (char *)workspace;
    float *y = (float *)(ws + L.y);
    int rc;
    {
        L2D_PROF("featvol_linear", s);
        if ((rc = linear_fwd(p, ws, L, s)) != LARA2DGS_OK) return rc;
    }
    {
        L2D_PROF("featvol_modln", s);
        const unsigned short *mod = (const unsigned short *)(ws + L.mod);
        if (channels_last(p, img_feats, img_feats)) L2D_LAUNCH_IN_SCOPE(s, modln_kernel<true>, dim3((p.T + 3) / 4), dim3(256), 0, p, mod, y);
        else L2D_LAUNCH_IN_SCOPE(s, modln_kernel<false>, dim3((p.T + 3) / 4), dim3(256), 0, p, mod, y);
    }
    {
        L2D_PROF(layout == LARA_FEATVOL_TOKENS ? "featvol_sample_tokens" : "featvol_sample_volume", s);
        const dim3 grid2((p.S + FV_PTS - 1) / FV_PTS, p.B);
        if (layout == LARA_FEATVOL_TOKENS) L2D_LAUNCH_IN_SCOPE(s, sample_kernel<true>, grid2, dim3(256), 0, p, (const float *)y, out);
        else L2D_LAUNCH_IN_SCOPE(s, sample_kernel<false>, grid2, dim3(256), 0, p, (const float *)y, out);
    }
    return LARA2DGS_OK;
}

int lara_featvol_backward(const lara_featvol_dims *d, const float *img_feats, const float *rays, const float *w2cs, const float *ixts,
                          const float *grid, const float *ln_w, const float *ln_b, const float *mlp_w, const float *mlp_b,
                          const float *grad, int32_t grad_layout, float *dx, float *d_ln_w, float *d_ln_b, float *d_mlp_w,
                          float *d_mlp_b, float *d_view_embed, void *workspace, void *stream) {
    if (!dims_ok(d) || (grad_layout != LARA_FEATVOL_VOLUME && grad_layout != LARA_FEATVOL_TOKENS)) return LARA2DGS_E_INVALID;
    if (!img_feats || !rays || !w2cs || !ixts || !grid || !ln_w || !ln_b || !mlp_w || !mlp_b || !grad || !dx || !d_ln_w || !d_ln_b ||
        !d_mlp_w || !d_mlp_b || !workspace)
        return LARA2DGS_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const FvP p = make_params(d, img_feats, rays, w2cs, ixts, grid, ln_w, ln_b, mlp_w, mlp_b, nullptr);
    const FvWs L = ws_layout(d);
    char *ws = (char *)workspace;
    const int CE = p.C + p.E;
    int rc;
    const float *g = grad;
    if (grad_layout == LARA_FEATVOL_VOLUME) {   // [B][V (C + E)][S] -> the token rows [B][S][V (C + E)]
        L2D_PROF("featvol_grad_transpose", s);
        if ((rc = lara_batched_transpose(p.B, p.V * CE, p.S, grad, ws + L.gt, 0, s)) != LARA2DGS_OK) return rc;
        g = (const float *)(ws + L.gt);
    }
    {
        L2D_PROF("featvol_linear", s);
        if ((rc = linear_fwd(p, ws, L, s)) != LARA2DGS_OK) return rc;
    }
    int *bins = (int *)(ws + L.bins);
    int2 *ents = (int2 *)(ws + L.ents);
    L2D_LAUNCH("featvol_index", s, index_kernel, dim3(p.B * p.V), dim3(256), 0, p, bins, ents);
    unsigned short *dmod = (unsigned short *)(ws + L.dmod);
    float *part = (float *)(ws + L.part);
    const int nblk = min(FV_TOK_BLOCKS, (p.T + 3) / 4);
    {
        L2D_PROF("featvol_token_bwd", s);
        if (p.Tp > p.T) L2D_HIP(hipMemsetAsync(dmod + (size_t)p.T * 2 * p.C, 0, (size_t)(p.Tp - p.T) * 2 * p.C * 2, s));
        const unsigned short *mod = (const unsigned short *)(ws + L.mod);
        if (channels_last(p, img_feats, dx))
            L2D_LAUNCH_IN_SCOPE(s, token_bwd_kernel<true>, dim3(nblk), dim3(256), 0, p, mod, bins, ents, g, dx, dmod, part);
        else L2D_LAUNCH_IN_SCOPE(s, token_bwd_kernel<false>, dim3(nblk), dim3(256), 0, p, mod, bins, ents, g, dx, dmod, part);
    }
    {
        L2D_PROF("featvol_param_grads", s);
        L2D_LAUNCH_IN_SCOPE(s, sum_parts_kernel, dim3((2 * p.C + 255) / 256), dim3(256), 0, (const float *)part, nblk, 2 * p.C, d_ln_w,
                            d_ln_b, p.C);
        if (d_view_embed && p.E > 0) {
            float *ep = (float *)(ws + L.epart);
            L2D_LAUNCH_IN_SCOPE(s, embed_part_kernel, dim3(FV_EMB_BLOCKS), dim3(256), 0, p, g, ep);
            L2D_LAUNCH_IN_SCOPE(s, sum_parts_kernel, dim3((p.V * p.E + 255) / 256), dim3(256), 0, (const float *)ep, FV_EMB_BLOCKS,
                                p.V * p.E, d_view_embed, d_view_embed, p.V * p.E);
        }
        float *prod = (float *)(ws + L.prod);
        L2D_HIP(hipMemsetAsync(prod, 0, (size_t)2 * p.C * FV_KA * 4, s));
        if ((rc = lara_gemm_tn_bf16(p.Tp, 2 * p.C, FV_KA, dmod, (const uint16_t *)(ws + L.act), prod, ws + L.tn, s)) != LARA2DGS_OK)
            return rc;
        L2D_LAUNCH_IN_SCOPE(s, split_dw_kernel, dim3((2 * p.C * 33 + 255) / 256), dim3(256), 0, (const float *)prod, 2 * p.C, d_mlp_w, d_mlp_b);
    }
    return LARA2DGS_OK;
}

}  // extern "C"
