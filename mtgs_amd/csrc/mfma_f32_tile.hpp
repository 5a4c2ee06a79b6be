// mfma_f32_tile.hpp -- the one exact-f32 MFMA tile (v_mfma_f32_32x32x2_f32) of the LPIPS convolutions (lpips.hip) and the DINOv2
// GEMM and attention (dino.hip).  A new consumer includes this; it does not restate it.
//
// Operand layout of one MFMA: lane l = (i = l & 31, h = l >> 5) supplies A(i, 2s + h) and B(2s + h, i) to k-step s; register v of
// the 32 x 32 result is row acc_row(v, h) = (v & 3) + 8 (v >> 2) + 4h, column i.
//
// The tile: a workgroup of TB = 256 threads = 4 waves computes 128 (M) x 32 NH (N) of A[M, K] B[K][N], K in steps of BK = 32 through
// LDS; wave w owns rows 32w .. 32w + 31 and NH 32-column halves (independent accumulators).  A is staged as sA[m][k] with stride 33
// (the 32 rows a k-step reads fall into 32 banks), B as sB[k][n] in float4 rows.  The next K-step's operands are fetched into
// registers before the current one is multiplied, and staged behind a barrier after it.  K is never split over lanes, waves or
// workgroups: every output is one k-ordered fma chain, the last K-step zero-filled beyond K, so a result is a function of the shape
// only.  With SEG > 0 the chain is restarted every SEG k's and the finished partial sums are added to a running total in k order.
#pragma once
#include "common.hpp"

namespace {

constexpr int TB = 256;
constexpr int BM = 128, BN = 64, BK = 32, SA = BK + 1;
constexpr int KQ = BK / 4;                 // 16-byte pieces of one row of the A tile
constexpr int RA = BM * KQ / TB;           // rows of the A tile per thread
static_assert(BM * KQ % TB == 0 && BM == 32 * (TB / 64) && BN == 64, "tile shape and loaders");

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ int acc_row(int v, int h) { return (v & 3) + 8 * (v >> 2) + 4 * h; }

// The A loader's share of the tile: this thread fetches k = k0 + 4 tile_a_kq() .. + 3 of the tile's rows tile_a_row(r), r < RA.
__device__ __forceinline__ int tile_a_kq() { return threadIdx.x % KQ; }
__device__ __forceinline__ int tile_a_row(int r) { return threadIdx.x / KQ + (TB / KQ) * r; }

// STEPS k-steps of a wave: acc += A[32, 2 STEPS] B[2 STEPS][32 NH].  `arow` is row i of A in LDS (k contiguous), `b` is B in LDS with
// the row stride LDB.  Each accumulator element stays one fma chain in k order.
template <int NH, int LDB, int STEPS>
__device__ __forceinline__ void mfma_f32_ksteps(const float *arow, const float *b, f32x16 &acc0, f32x16 &acc1) {
    const int l = threadIdx.x & 63, i = l & 31, hh = l >> 5;
    const float *pa = arow + hh, *pb = b + hh * LDB + i;
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
        const float a = pa[2 * s];
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, pb[2 * s * LDB], acc0, 0, 0, 0);
        if (NH == 2) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, pb[2 * s * LDB + 32], acc1, 0, 0, 0);
    }
}

// The tile body of workgroup (blockIdx.x, blockIdx.y): rows blockIdx.x BM .., columns blockIdx.y 32 NH .. of A[M, K] wt[K][N].
//   NH       32-column halves per workgroup (2: 128 x 64, 1: 128 x 32)
//   SEG      k's per fma chain (a multiple of BK); 0: one chain over all of K, and no totals exist
//   GUARD    N is a multiple of 32 only, so the last 64-wide tile may be half empty (the four columns of a float4 stand or fall
//            together); without it N is a multiple of 32 NH
//   fetch_a(k0, ra)   fills ra[r] with A(tile_a_row(r), k0 + 4 tile_a_kq() .. + 3), zero beyond M and K
//   epilogue(n)       called once per column of this lane; returns column(m, x), called for every row m < M with the finished sum x
template <int NH, int SEG, bool GUARD, class FetchA, class Epilogue>
__device__ __forceinline__ void mfma_f32_tile(const float *wt, int M, int N, int K, FetchA fetch_a, Epilogue epilogue) {
    static_assert((NH == 1 || NH == 2) && SEG % BK == 0, "tile shape");
    constexpr int SB = 32 * NH, BQ = SB / 4, BR = TB / BQ, RB = BK / BR;      // B tile: row stride, float4 per row, rows per pass, passes
    __shared__ float sA[BM * SA];
    __shared__ __attribute__((aligned(16))) float sB[BK * SB];
    const int t = threadIdx.x, wv = t >> 6, l = t & 63, i = l & 31, hh = l >> 5;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * SB;

    const int kb = t / BQ, nq = t % BQ;            // B: rows kb + BR r of the K-step, columns n0 + 4 nq .. + 3
    const bool colok = !GUARD || n0 + 4 * nq < N;
    float4 ra[RA], rb[RB];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const int k = k0 + kb + BR * r;
            rb[r] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (colok && k < K) rb[r] = *reinterpret_cast<const float4 *>(wt + (size_t)k * N + n0 + 4 * nq);
        }
        fetch_a(k0, ra);
    };
    auto stage = [&]() {
#pragma unroll
        for (int r = 0; r < RA; ++r) {
            float *d = sA + tile_a_row(r) * SA + 4 * tile_a_kq();
            d[0] = ra[r].x; d[1] = ra[r].y; d[2] = ra[r].z; d[3] = ra[r].w;
        }
#pragma unroll
        for (int r = 0; r < RB; ++r) *reinterpret_cast<float4 *>(sB + (kb + BR * r) * SB + 4 * nq) = rb[r];
    };

    f32x16 acc0, acc1, tot0, tot1;             // the running chain and, with SEG, the total of the finished ones
#pragma unroll
    for (int v = 0; v < 16; ++v) { acc0[v] = 0.f; acc1[v] = 0.f; tot0[v] = 0.f; tot1[v] = 0.f; }

    fetch(0);
    stage();
    __syncthreads();
    for (int k0 = 0; k0 < K; k0 += BK) {
        const bool more = k0 + BK < K;
        if (more) fetch(k0 + BK);
        if constexpr (SEG > 0) {
            if (k0 != 0 && k0 % SEG == 0) {
#pragma unroll
                for (int v = 0; v < 16; ++v) { tot0[v] += acc0[v]; tot1[v] += acc1[v]; acc0[v] = 0.f; acc1[v] = 0.f; }
            }
        }
        mfma_f32_ksteps<NH, SB, BK / 2>(sA + (wv * 32 + i) * SA, sB, acc0, acc1);
        __syncthreads();
        if (more) {
            stage();
            __syncthreads();
        }
    }
    if constexpr (SEG > 0) {
#pragma unroll
        for (int v = 0; v < 16; ++v) { acc0[v] += tot0[v]; acc1[v] += tot1[v]; }      // + 0 for K <= SEG: the single chain's bits
    }

    // lane i holds column i of every half: 128-byte rows of stores
#pragma unroll
    for (int half = 0; half < NH; ++half) {
        const int n = n0 + 32 * half + i;
        if (GUARD && n >= N) continue;
        auto column = epilogue(n);
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int m = m0 + wv * 32 + acc_row(v, hh);
            if (m >= M) continue;
            column(m, half ? acc1[v] : acc0[v]);
        }
    }
}

}  // namespace
