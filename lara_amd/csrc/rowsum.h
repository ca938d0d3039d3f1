// rowsum.h -- the fixed-order sum of per-item terms to one row, in two launches (meshmetrics.hip, depthsurface.hip, meshalign.hip):
// every workgroup of 256 leaves part[block][NQ] doubles and cnt[block][NC] integers, one workgroup adds the partials up.  The order
// of the additions is the contract: the xor butterfly inside a wave, the four waves as ((w0 + w1) + w2) + w3, the partials strided
// by 256 per thread, then the 256-wide tree.  Where a total lands in the row is the calling kernel's.  Everything sits in an unnamed
// namespace and is __forceinline__.  Include it from units built with -ffp-contract=off only.
#pragma once
#include "common.h"
#include "wave.h"

namespace {

// the wave's sum of v -> the wave's slot of red
template <class T>
__device__ __forceinline__ void rowsum_wave(T (&red)[4], const T v) {
    const T s = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
}

// after every rowsum_wave: the four slots of each quantity -> part[block][NQ], cnt[block][NC]
template <int NQ, int NC>
__device__ __forceinline__ void rowsum_block_partial(const double (&red)[NQ][4], const int (&redc)[NC][4], double *__restrict__ part,
                                                     unsigned *__restrict__ cnt) {
    __syncthreads();
    if (threadIdx.x < NQ) {
        const int k = threadIdx.x;
        part[(size_t)blockIdx.x * NQ + k] = ((red[k][0] + red[k][1]) + red[k][2]) + red[k][3];
    }
    if (threadIdx.x >= 64 && threadIdx.x < 64 + NC) {
        const int k = threadIdx.x - 64;
        cnt[(size_t)blockIdx.x * NC + k] = (unsigned)(((redc[k][0] + redc[k][1]) + redc[k][2]) + redc[k][3]);
    }
}

// both steps for a thread that holds its NQ terms and NC flags
template <int NQ, int NC>
__device__ __forceinline__ void rowsum_block(const double (&s)[NQ], const int (&c)[NC], double *__restrict__ part,
                                             unsigned *__restrict__ cnt) {
    __shared__ double red[NQ][4];
    __shared__ int redc[NC][4];
#pragma unroll
    for (int k = 0; k < NQ; k++) rowsum_wave(red[k], s[k]);
#pragma unroll
    for (int k = 0; k < NC; k++) rowsum_wave(redc[k], c[k]);
    rowsum_block_partial(red, redc, part, cnt);
}

// one workgroup of 256: put_sum(q, total of part[.][q]) and put_count(q, total of cnt[.][q]) from thread 0
template <int NQ, int NC, class PutSum, class PutCount>
__device__ __forceinline__ void rowsum_finish(const int blocks, const double *__restrict__ part, const unsigned *__restrict__ cnt,
                                              PutSum put_sum, PutCount put_count) {
    __shared__ double red[256];
    __shared__ unsigned long long redc[256];
    const int tid = threadIdx.x;
    for (int q = 0; q < NQ; q++) {
        double s = 0.0;
        for (int k = tid; k < blocks; k += 256) s += part[(size_t)k * NQ + q];
        red[tid] = s;
        __syncthreads();
        for (int d = 128; d > 0; d >>= 1) {
            if (tid < d) red[tid] += red[tid + d];
            __syncthreads();
        }
        if (tid == 0) put_sum(q, red[0]);
        __syncthreads();
    }
    for (int q = 0; q < NC; q++) {
        unsigned long long s = 0;
        for (int k = tid; k < blocks; k += 256) s += cnt[(size_t)k * NC + q];
        redc[tid] = s;
        __syncthreads();
        for (int d = 128; d > 0; d >>= 1) {
            if (tid < d) redc[tid] += redc[tid + d];
            __syncthreads();
        }
        if (tid == 0) put_count(q, (double)redc[0]);
        __syncthreads();
    }
}

}  // namespace
