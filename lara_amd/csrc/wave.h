// wave.h -- device primitives shared by the translation units: MFMA operand vectors, bf16 conversion, the 64-lane butterfly
// sum, minimum and maximum, and the DPP move the wave-level reductions are built from.
#pragma once
#include <hip/hip_runtime.h>

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) unsigned short u16x8;

// fp32 -> bf16, round to nearest even, on gfx950's v_cvt_pk_bf16_f32 (two values per instruction; the integer form
// u += 0x7fff + ((u >> 16) & 1) >> 16 is three half-rate instructions per value, and a kernel that rounds hundreds of values per lane
// -- the fused attention step: 512 -- spent 40 % of its vector instructions on it).  Same result for every finite input and inf.
// (through the compiler's own conversion, not inline asm: an asm statement that reads an MFMA accumulator is invisible to the
// hazard recognizer -- the first version did exactly that behind the attention's P.V product and produced NaNs)
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned f2bf2(float lo, float hi) {   // bf16(lo) | bf16(hi) << 16
    const f32x2_t v = {lo, hi};
    const bf16x2_t r = __builtin_convertvector(v, bf16x2_t);
    unsigned u;
    __builtin_memcpy(&u, &r, 4);
    return u;
}
__device__ __forceinline__ unsigned short f2bf(float f) { return (unsigned short)f2bf2(f, f); }
__device__ __forceinline__ float bf2f(unsigned short h) { return __uint_as_float((unsigned)h << 16); }
__device__ __forceinline__ float bfr(const float v) { return bf2f(f2bf(v)); }   // round to bf16 and back

// wave-wide sum by the xor butterfly: the same value in every lane
template <class T>
__device__ __forceinline__ T wave_sum_xor(T v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ float wave_sum(float v) { return wave_sum_xor(v); }
__device__ __forceinline__ double wave_sum(double v) { return wave_sum_xor(v); }
__device__ __forceinline__ int wave_sum(int v) { return wave_sum_xor(v); }

// wave-wide minimum / maximum by the same butterfly (fminf / fmaxf skip a NaN)
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = fminf(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
    return v;
}

// wave-wide inclusive prefix sum over the lanes (Hillis-Steele on __shfl_up); lane = the caller's lane id, 0..63
template <class T>
__device__ __forceinline__ T wave_inclusive_scan(T v, const int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T u = __shfl_up(v, d, 64);
        if (lane >= d) v += u;
    }
    return v;
}

// x moved across lanes by one DPP control (lanes the control or the row mask leaves out read 0): the step of the DPP reductions
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_move(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, ROW_MASK, 0xf, false));
}

}  // namespace
