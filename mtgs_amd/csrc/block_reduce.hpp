// block_reduce.hpp -- the fixed-order block reductions of the loss, metric and output-head kernels.
//
// Every sum here is part of a contract: the summation order is fixed (per-thread strided partial sums, then a fixed
// tree over the block), there are no float atomics, so results are bitwise reproducible, and nothing is read back or
// allocated, so the callers can be captured in a HIP graph.  The float and the fp64 finishes round differently on
// purpose (the fp64 ones restate reductions the reference runs in double); they are not interchangeable.
#pragma once
#include "common.hpp"

namespace {

// Sum over a block of exactly 256 threads (4 waves); every thread gets the total.  `lds` holds 4 floats and may be
// reused by the next call (the leading barrier protects the previous call's reads).
__device__ __forceinline__ float block_sum4(float v, float *lds) {
    v = wave_sum_to_lane63(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 63) lds[wave] = v;
    __syncthreads();
    return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

// Fixed-order sum over a block of BLOCK threads (a halving tree in `lds`, BLOCK elements); returns the total.  `lds` may be reused
// once every thread has passed a barrier behind the call.  Callers name the precision: block_tree_sum_f64 / _f32.
template <int BLOCK, class T>
__device__ __forceinline__ T block_tree_sum(T a, T *lds) {
    const int tid = threadIdx.x;
    lds[tid] = a;
    __syncthreads();
    for (int o = BLOCK / 2; o > 0; o >>= 1) {
        if (tid < o) lds[tid] += lds[tid + o];
        __syncthreads();
    }
    return lds[0];
}
template <int BLOCK>
__device__ __forceinline__ double block_tree_sum_f64(double a, double *lds) { return block_tree_sum<BLOCK>(a, lds); }
template <int BLOCK>
__device__ __forceinline__ float block_tree_sum_f32(float a, float *lds) { return block_tree_sum<BLOCK>(a, lds); }

// Fixed-order fp64 sum of K interleaved float partials over nblocks blocks, by one block of BLOCK threads; thread 0 ends
// with the totals.  (One tree for all K columns: one barrier per level, not K.)
template <int K, int BLOCK>
__device__ __forceinline__ void finish_sums(int64_t nblocks, const float *__restrict__ partials, double *s) {
    __shared__ double lds[K][BLOCK];
    double acc[K];
#pragma unroll
    for (int j = 0; j < K; ++j) acc[j] = 0.0;
    for (int64_t i = threadIdx.x; i < nblocks; i += BLOCK) {
#pragma unroll
        for (int j = 0; j < K; ++j) acc[j] += (double)partials[i * K + j];
    }
#pragma unroll
    for (int j = 0; j < K; ++j) lds[j][threadIdx.x] = acc[j];
    __syncthreads();
    for (int w = BLOCK / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
#pragma unroll
            for (int j = 0; j < K; ++j) lds[j][threadIdx.x] += lds[j][threadIdx.x + w];
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < K; ++j) s[j] = lds[j][0];
}

}  // namespace
