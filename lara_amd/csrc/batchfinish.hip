// batchfinish.hip -- the image half of a loader batch from the stored uint8 arrays: colour over the view's background, mask, rotated
// normals, in ONE streaming kernel.  Interface, layouts and the operation order: lara_batchfinish.h; the per-pixel function, shared
// with the host entry: batchfinish_ops.h.
//
//   bf_kernel<WIDE>                at most 2048 workgroups of 256 threads stride over the quads of the batch: a quad is 4 consecutive
//                                   pixels of the flat index (b, v, h, w), the last one of an odd batch is short.  The kernel is a pure
//                                   stream (7 bytes in, 25 bytes out per pixel), so a lane moves 16 bytes per access where it may:
//                                     colour   one 16-byte load of RGBA, three 16-byte stores of rgb (48 contiguous bytes, lane next to
//                                              lane), one 4-byte word of masks.  H W % 4 == 0: the four pixels share a view and its bg.
//                                     normals  three 4-byte loads (12 contiguous bytes), three 16-byte stores.  W % 4 == 0: the four
//                                              pixels share a row, so their 12 floats are contiguous at out_nrm[b][h][v W + w].
//                                   A half that may not go wide (the shape, or a base address off its alignment: the launcher decides
//                                   once per call) runs the per-pixel function pixel by pixel with byte and word accesses.  Both ways
//                                   call the same function on the same bytes and store the same words.  Pixels are counted in 32 bits
//                                   (the launcher refuses 2^31 and more), byte offsets are formed in 64.
#include "common.h"
#include "batchfinish_ops.h"
#include "../../include/lara_batchfinish.h"

namespace {

constexpr int BF_BLOCK = 256;
constexpr uint32_t BF_QUAD = 4;

// pixel p of the flat index -> (b V + v, b, v, h, w)
struct BfAt { uint32_t bv, b, v, h, w; };
__device__ __forceinline__ BfAt bf_at(const uint32_t p, const uint32_t V, const uint32_t W, const uint32_t HW) {
    BfAt a;
    a.bv = p / HW;
    const uint32_t rem = p - a.bv * HW;
    a.b = a.bv / V;
    a.v = a.bv - a.b * V;
    a.h = rem / W;
    a.w = rem - a.h * W;
    return a;
}

template <int WIDE>                                                      // bit 0: the colour goes wide; bit 1: the normals do
__global__ void __launch_bounds__(BF_BLOCK)
bf_kernel(const uint8_t *__restrict__ rgba, const float *__restrict__ bg, const uint8_t *__restrict__ n_u8, const float *__restrict__ rot,
          const uint32_t N, const uint32_t V, const uint32_t H, const uint32_t W, float *__restrict__ out_rgb,
          uint8_t *__restrict__ out_msk, float *__restrict__ out_nrm) {
    constexpr bool WIDE_RGB = (WIDE & 1) != 0, WIDE_NRM = (WIDE & 2) != 0;
    const uint32_t HW = H * W;
    const uint32_t quads = (N + (BF_QUAD - 1)) / BF_QUAD;
    const uint32_t stride = gridDim.x * BF_BLOCK;
    for (uint32_t q = blockIdx.x * BF_BLOCK + threadIdx.x; q < quads; q += stride) {
        const uint32_t p0 = q * BF_QUAD;
        const uint32_t n = N - p0 < BF_QUAD ? N - p0 : BF_QUAD;          // pixels of this quad
        if (WIDE_RGB) {                                                  // (H W % 4 == 0: n == 4, one view)
            const uint4 word = *(const uint4 *)(rgba + (size_t)p0 * 4);
            const uint32_t w4[4] = {word.x, word.y, word.z, word.w};
            const float *const bgv = bg + 3 * (size_t)(p0 / HW);
            const float back[3] = {bgv[0], bgv[1], bgv[2]};
            float rgb[12];
            uint8_t m[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint8_t px[4] = {(uint8_t)(w4[i] & 255u), (uint8_t)((w4[i] >> 8) & 255u), (uint8_t)((w4[i] >> 16) & 255u),
                                       (uint8_t)(w4[i] >> 24)};
                lara_batchfinish_colour(px, back, rgb + 3 * i, m + i);
            }
            float4 *const o = (float4 *)(out_rgb + (size_t)p0 * 3);
            o[0] = make_float4(rgb[0], rgb[1], rgb[2], rgb[3]);
            o[1] = make_float4(rgb[4], rgb[5], rgb[6], rgb[7]);
            o[2] = make_float4(rgb[8], rgb[9], rgb[10], rgb[11]);
            *(uint32_t *)(out_msk + p0) = (uint32_t)m[0] | ((uint32_t)m[1] << 8) | ((uint32_t)m[2] << 16) | ((uint32_t)m[3] << 24);
        } else {
            for (uint32_t i = 0; i < n; ++i) {
                const uint32_t p = p0 + i;
                lara_batchfinish_colour(rgba + (size_t)p * 4, bg + 3 * (size_t)(p / HW), out_rgb + (size_t)p * 3, out_msk + p);
            }
        }
        if (!n_u8) continue;
        if (WIDE_NRM) {                                                  // (W % 4 == 0: n == 4, one row)
            const uint32_t *const src = (const uint32_t *)(n_u8 + (size_t)p0 * 3);
            const uint32_t w3[3] = {src[0], src[1], src[2]};
            const BfAt a = bf_at(p0, V, W, HW);
            const float *const Rb = rot + 9 * (size_t)a.b;
            float R[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) R[k] = Rb[k];
            float nrm[12];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                uint8_t nb[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) nb[k] = (uint8_t)((w3[(3 * i + k) / 4] >> (8 * ((3 * i + k) % 4))) & 255u);
                lara_batchfinish_normal(nb, R, nrm + 3 * i);
            }
            float4 *const o = (float4 *)(out_nrm + lara_batchfinish_nrm_at(a.b, a.v, a.h, a.w, V, H, W));
            o[0] = make_float4(nrm[0], nrm[1], nrm[2], nrm[3]);
            o[1] = make_float4(nrm[4], nrm[5], nrm[6], nrm[7]);
            o[2] = make_float4(nrm[8], nrm[9], nrm[10], nrm[11]);
        } else {
            for (uint32_t i = 0; i < n; ++i) {
                const uint32_t p = p0 + i;
                const BfAt a = bf_at(p, V, W, HW);
                lara_batchfinish_normal(n_u8 + (size_t)p * 3, rot + 9 * (size_t)a.b, out_nrm + lara_batchfinish_nrm_at(a.b, a.v, a.h, a.w, V, H, W));
            }
        }
    }
}

// 0: an empty batch; 1: work to do; < 0: refused
int bf_args(const uint8_t *rgba, const float *bg, const uint8_t *n_u8, const float *rot, const int64_t B, const int64_t V, const int64_t H,
            const int64_t W, const float *out_rgb, const uint8_t *out_msk, const float *out_nrm, int64_t *pixels) {
    const int64_t LIMIT = (int64_t)1 << 31;
    if (B < 0 || V < 0 || H < 0 || W < 0) return LARA2DGS_E_INVALID;
    *pixels = 0;
    if (B == 0 || V == 0 || H == 0 || W == 0) return 0;
    if (B >= LIMIT || V >= LIMIT || H >= LIMIT || W >= LIMIT) return LARA2DGS_E_INVALID;
    int64_t n = B * V;                                                   // (each factor < 2^31: no product overflows 2^63 before it is checked)
    if (n >= LIMIT) return LARA2DGS_E_INVALID;
    n *= H;
    if (n >= LIMIT) return LARA2DGS_E_INVALID;
    n *= W;
    if (n >= LIMIT) return LARA2DGS_E_INVALID;
    if (!rgba || !bg || !out_rgb || !out_msk) return LARA2DGS_E_INVALID;
    const int have = (n_u8 != nullptr) + (rot != nullptr) + (out_nrm != nullptr);
    if (have != 0 && have != 3) return LARA2DGS_E_INVALID;
    *pixels = n;
    return 1;
}

bool bf_aligned(const void *p, const uintptr_t to) { return ((uintptr_t)p & (to - 1)) == 0; }

}  // namespace

extern "C" {

int lara_batch_finish(const uint8_t *rgba, const float *bg, const uint8_t *nrm_u8, const float *rot, int64_t B, int64_t V, int64_t H,
                      int64_t W, float *out_rgb, uint8_t *out_msk, float *out_nrm, void *stream) {
    int64_t N = 0;
    const int go = bf_args(rgba, bg, nrm_u8, rot, B, V, H, W, out_rgb, out_msk, out_nrm, &N);
    if (go <= 0) return go;
    const bool wide_rgb = (H * W) % 4 == 0 && bf_aligned(rgba, 16) && bf_aligned(out_rgb, 16) && bf_aligned(out_msk, 4);
    const bool wide_nrm = nrm_u8 && W % 4 == 0 && bf_aligned(nrm_u8, 4) && bf_aligned(out_nrm, 16);
    const int64_t quads = (N + 3) / 4;
    const int64_t want = (quads + BF_BLOCK - 1) / BF_BLOCK;
    const unsigned groups = (unsigned)(want < LARA_BATCHFINISH_MAX_GROUPS ? want : LARA_BATCHFINISH_MAX_GROUPS);
#define BF_GO(WIDE)                                                                                                                 \
    L2D_LAUNCH_IN_SCOPE((hipStream_t)stream, bf_kernel<WIDE>, dim3(groups), dim3(BF_BLOCK), 0, rgba, bg, nrm_u8, rot, (uint32_t)N,  \
                        (uint32_t)V, (uint32_t)H, (uint32_t)W, out_rgb, out_msk, out_nrm)
    switch ((wide_rgb ? 1 : 0) | (wide_nrm ? 2 : 0)) {
    case 0: BF_GO(0); break;
    case 1: BF_GO(1); break;
    case 2: BF_GO(2); break;
    default: BF_GO(3); break;
    }
#undef BF_GO
    return LARA2DGS_OK;
}

int lara_batch_finish_host(const uint8_t *rgba, const float *bg, const uint8_t *nrm_u8, const float *rot, int64_t B, int64_t V, int64_t H,
                           int64_t W, float *out_rgb, uint8_t *out_msk, float *out_nrm) {
    int64_t N = 0;
    const int go = bf_args(rgba, bg, nrm_u8, rot, B, V, H, W, out_rgb, out_msk, out_nrm, &N);
    if (go <= 0) return go;
    lara_batchfinish_host_pixels(rgba, bg, nrm_u8, rot, B, V, H, W, out_rgb, out_msk, out_nrm);
    return LARA2DGS_OK;
}

}  // extern "C"
