// wild.hip -- WildGaussians appearance colours (config/WildGaussians.py, use_wild_gaussians=True): the appearance MLP of
// mtgs_scene_graph.py:308-318 / :623-632, forward and backward, on exact-f32 MFMA (v_mfma_f32_32x32x2_f32).
//
//   rgb    = clamp(features_dc * C0 + 0.5, 0, 1)                      [3]
//   x      = [rgb | features_rest.view(N, -1)[:, :24] | e]             [27 + 32]
//   y      = 0.01 * L3(relu(L2(relu(L1(x)))))                          59 -> 128 -> 128 -> 6
//   colour = rgb * (1 + y[3:6]) + y[0:3]
//
// The embedding is the same for every row, so it is folded into the first bias (b1' = b1 + W1[:, 27:59] e, computed by every
// workgroup in the same order) and layer 1 is 27 -> 128.
//
// Layout.  A workgroup (4 waves) keeps the weights in LDS for its whole life (W2 alone is 64 KB; 113 KB forward, 148 KB backward:
// one workgroup per CU, one wave per SIMD -- the 32x32x2 f32 MFMA issues every 64 cycles with a dependent-accumulator latency of
// 64, so one accumulator chain per wave is the full rate) and walks tiles of 32 rows, grid-strided, at most WILD_GRID workgroups.
// Activations are kept TRANSPOSED in the accumulators: hidden unit on the MFMA row (registers), row of the tile on the lane, so
// that the 32 columns of a tile never mix -- each row's colour is a function of that row alone, whichever tile, position or
// launch form (dense, visible rows, flagged rows) it is computed in.  Wave w owns hidden units [32 w, 32 w + 32) of each layer;
// the layers meet in LDS ([row][hidden], 129-float rows: the lane-strided MFMA operand reads are bank-conflict free).
// Layer 3 (6 outputs) runs on the VALU: per-lane partial sums over the 16 hidden units a lane holds, then a fixed-order sum
// over the 8 (wave, lane half) partials.
//
// Backward: h1 and h2 are RECOMPUTED from the inputs (storing them is 1 KB per row written and read
// again).  The weight gradients are sums over rows; each workgroup accumulates its own in registers (dW2, dW1[:, :27]: MFMA
// with the tile's rows as the contraction index) and VGPR sums (dW3, db3, db2, sum dh1), writes ONE partial per workgroup,
// and mtgs_wild_reduce adds the partials in workgroup order.  No float atomics: the weight gradients are bitwise identical
// from run to run.  Nothing reads a count on the host: the row count of the visible form is the device word `totals`.
#include "common.hpp"

namespace {

constexpr int WT = 32;           // rows per tile (the MFMA's 32 columns)
constexpr int WB = 256;          // threads per workgroup: 4 waves
constexpr int NH = 128, NF = 27, NE = 32, NO = 6, NIN = NF + NE;
constexpr int P1 = 33;           // LDS row stride of W1[:, :27] (columns 27..32 zero) and of the input tile
constexpr int P2 = 129;          // LDS row stride of W2 and of the [row][hidden] activation tiles
constexpr int WILD_GRID = 256;   // workgroups at most (one per CU); fixed, so the partial-sum order does not depend on the device
constexpr float C0 = 0.28209479177387814f;
// partial sums of one workgroup (floats): dW1[:, :27] | sum dh1 | dW2 | db2 | dW3 | db3
constexpr int OFF_W1 = 0, OFF_S1 = OFF_W1 + NH * NF, OFF_W2 = OFF_S1 + NH, OFF_B2 = OFF_W2 + NH * NH, OFF_W3 = OFF_B2 + NH,
              OFF_B3 = OFF_W3 + NO * NH, PART = OFF_B3 + 8;

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ int acc_row(int v, int h) { return (v & 3) + 8 * (v >> 2) + 4 * h; }   // row of register v (C/D map)

// acc += A[32 x 2K] . B[2K x 32], both in LDS: A(i, k) = A[i * ai + k * ak], B(k, j) = B[k * bk + j * bj].
// Lane l supplies A(l & 31, 2s + (l >> 5)) and B(2s + (l >> 5), l & 31) to k-step s.
template <int KSTEPS>
__device__ __forceinline__ f32x16 mfma_lds(f32x16 acc, const float *A, int ai, int ak, const float *B, int bk, int bj) {
    const int l = threadIdx.x & 63, i = l & 31, h = l >> 5;
#pragma unroll 8
    for (int s = 0; s < KSTEPS; ++s) {
        const int k = 2 * s + h;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(A[i * ai + k * ak], B[k * bk + i * bj], acc, 0, 0, 0);
    }
    return acc;
}
__device__ __forceinline__ f32x16 zero16() {
    f32x16 z;
#pragma unroll
    for (int v = 0; v < 16; ++v) z[v] = 0.f;
    return z;
}
__device__ __forceinline__ float rgb_pre(float dc) {     // dc * C0 + 0.5, rounded twice as PyTorch does
#pragma clang fp contract(off)
    return dc * C0 + 0.5f;
}

struct Weights {
    const float *emb, *w1, *b1, *w2, *b2, *w3, *b3;
};
struct Rows {      // the row set: dense (vis_ids null: row r is Gaussian r, n = cap) or visible rows (n = min(totals >> 32, cap))
    const int32_t *vis_ids;
    const int64_t *totals;
    int64_t cap;
    __device__ int64_t count() const {
        if (!vis_ids) return cap;
        const int64_t n = *totals >> 32;
        return n < cap ? n : cap;
    }
    __device__ int64_t gauss(int64_t r) const { return vis_ids ? (int64_t)vis_ids[r] : r; }
};

// LDS weight image: W1[:, :27] [128][33], W2 [128][129], W3 [6][128], b1' (embedding folded), b2, b3
struct WeightLds {
    float w1[NH * P1], w2[NH * P2], w3[NO * NH], b1[NH], b2[NH], b3[8];
};
__device__ void load_weights(WeightLds &s, const Weights &W) {
    const int t = threadIdx.x;
    for (int e = t; e < NH * P1; e += WB) {
        const int o = e / P1, c = e - o * P1;
        s.w1[e] = c < NF ? W.w1[o * NIN + c] : 0.f;
    }
    for (int e = t; e < NH * NH; e += WB) s.w2[(e >> 7) * P2 + (e & 127)] = W.w2[e];
    for (int e = t; e < NO * NH; e += WB) s.w3[e] = W.w3[e];
    if (t < NH) {
        float b = W.b1[t];
        if (W.emb) {
            const float *we = W.w1 + t * NIN + NF;
            for (int c = 0; c < NE; ++c) b = fmaf(we[c], W.emb[c], b);
        }
        s.b1[t] = b;
        s.b2[t] = W.b2[t];
    }
    if (t < NO) s.b3[t] = W.b3[t];
}

// Input tile [32][33]: rgb (clamped) | features_rest[:24] | zeros.  mask (nullable): the clamp's pass-through bits, 1.f / 0.f
// (torch.clamp passes the gradient where min <= x <= max).  Rows past the count (or not flagged) are zero.
__device__ void load_inputs(float *sx, float *mask, const Rows &R, int64_t n, const uint8_t *flags, int64_t r0, const float *dc,
                            int64_t dc_stride, const float *rest, int64_t rest_stride) {
    for (int e = threadIdx.x; e < WT * WT; e += WB) {
        const int row = e >> 5, c = e & 31;
        const int64_t r = r0 + row;
        float v = 0.f;
        if (c < NF && r < n && (!flags || flags[r])) {
            const int64_t g = R.gauss(r);
            if (c < 3) {
                const float x = rgb_pre(dc[g * dc_stride + c]);
                v = x < 0.f ? 0.f : (x > 1.f ? 1.f : x);
                if (mask) mask[row * 4 + c] = (x >= 0.f && x <= 1.f) ? 1.f : 0.f;
            } else {
                v = rest[g * rest_stride + (c - 3)];
            }
        } else if (c < 3 && mask) {
            mask[row * 4 + c] = 0.f;
        }
        sx[row * P1 + c] = v;
    }
}

// Layers 1 and 2 of the tile.  Leaves relu(h1) in s_h1 [row][hidden] and returns this wave's block of relu(h2)^T
// (hidden w * 32 + acc_row(v, lane >> 5), row lane & 31).
__device__ f32x16 layers12(const WeightLds &s, const float *sx, float *s_h1) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63, j = l & 31, h = l >> 5;
    f32x16 a = mfma_lds<14>(zero16(), s.w1 + w * 32 * P1, P1, 1, sx, 1, P1);
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int o = w * 32 + acc_row(v, h);
        const float x = a[v] + s.b1[o];
        s_h1[j * P2 + o] = x > 0.f ? x : 0.f;
    }
    __syncthreads();
    a = mfma_lds<64>(zero16(), s.w2 + w * 32 * P2, P2, 1, s_h1, 1, P2);
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const float x = a[v] + s.b2[w * 32 + acc_row(v, h)];
        a[v] = x > 0.f ? x : 0.f;
    }
    return a;
}
// Layer 3, first half: this lane's partial sums over its 16 hidden units -> s_p[(wave * 2 + half) * 32 + row][6]
__device__ void layer3_partial(const WeightLds &s, const f32x16 &h2, float *s_p) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63, j = l & 31, h = l >> 5;
    float p[NO];
#pragma unroll
    for (int k = 0; k < NO; ++k) p[k] = 0.f;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int o = w * 32 + acc_row(v, h);
#pragma unroll
        for (int k = 0; k < NO; ++k) p[k] = fmaf(s.w3[k * NH + o], h2[v], p[k]);
    }
#pragma unroll
    for (int k = 0; k < NO; ++k) s_p[((w * 2 + h) * 32 + j) * NO + k] = p[k];
}
// ... second half (one thread per row): y = 0.01 * (b3 + the 8 partials in a fixed order)
__device__ void layer3_sum(const WeightLds &s, const float *s_p, int row, float y[NO]) {
#pragma unroll
    for (int k = 0; k < NO; ++k) {
        float z = 0.f;
        for (int q = 0; q < 8; ++q) z += s_p[(q * 32 + row) * NO + k];
        y[k] = 0.01f * (z + s.b3[k]);
    }
}

__global__ __launch_bounds__(WB) void wild_fwd_kernel(Rows R, const uint8_t *__restrict__ flags, const float *__restrict__ dc,
                                                      int64_t dc_stride, const float *__restrict__ rest, int64_t rest_stride,
                                                      Weights W, float *__restrict__ out, int64_t out_stride) {
    __shared__ WeightLds s;
    __shared__ float sx[WT * P1], s_h1[WT * P2], s_p[8 * WT * NO];
    const int64_t n = R.count(), tiles = ceil_div64(n, WT);
    if ((int64_t)blockIdx.x >= tiles) return;
    load_weights(s, W);
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t r0 = t * WT;
        load_inputs(sx, nullptr, R, n, flags, r0, dc, dc_stride, rest, rest_stride);
        __syncthreads();
        const f32x16 h2 = layers12(s, sx, s_h1);
        layer3_partial(s, h2, s_p);
        __syncthreads();
        if (threadIdx.x < WT) {
            const int row = threadIdx.x;
            const int64_t r = r0 + row;
            if (r < n) {
                float y[NO];
                layer3_sum(s, s_p, row, y);
                float *o = out + r * out_stride;
                if (!flags || flags[r]) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) o[c] = sx[row * P1 + c] * (1.f + y[3 + c]) + y[c];
                } else {      // a row the frame composites nothing from: a finite constant, nothing of it is read
                    o[0] = 0.f; o[1] = 0.f; o[2] = 0.f;
                }
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(WB) void wild_bwd_kernel(Rows R, const float *__restrict__ grad, int64_t grad_stride,
                                                      const float *__restrict__ dc, int64_t dc_stride, const float *__restrict__ rest,
                                                      int64_t rest_stride, Weights W, float *__restrict__ d_dc, float *__restrict__ d_rest,
                                                      int64_t d_rest_width, float *__restrict__ partials) {
    __shared__ WeightLds s;
    __shared__ float sx[WT * P1], s_h1[WT * P2], s_h2[WT * P2], s_dh2[WT * P2], s_p[8 * WT * NO], s_dz[WT * 8], s_dr[WT * 4],
        s_mask[WT * 4];
    float *const s_dh1 = s_h2;     // (h2 is dead once dW3 has read it)
    float *const s_dx = s_dh2;     // (dh2 is dead once dW2 and dh1 have read it): [wave][c][row] partials of W1^T dh1
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63, j = l & 31, h = l >> 5, t_ = threadIdx.x;
    const int64_t n = R.count(), tiles = ceil_div64(n, WT);
    load_weights(s, W);
    f32x16 g_w2[4], g_w1 = zero16();       // this wave's rows [32 w, 32 w + 32) of dW2 (four 32-column blocks) and of dW1[:, :27]
#pragma unroll
    for (int b = 0; b < 4; ++b) g_w2[b] = zero16();
    float g_w3[3] = {0.f, 0.f, 0.f}, g_b = 0.f, g_b3 = 0.f;   // dW3 elements t, t + 256, t + 512; db2 (t < 128) / sum dh1 (t >= 128); db3
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t r0 = t * WT;
        load_inputs(sx, s_mask, R, n, nullptr, r0, dc, dc_stride, rest, rest_stride);
        if (t_ < WT * 3) {
            const int row = t_ / 3, c = t_ - row * 3;
            const int64_t r = r0 + row;
            s_dr[row * 4 + c] = r < n ? grad[r * grad_stride + c] : 0.f;      // (the cotangent until the row's thread below)
        }
        __syncthreads();
        f32x16 h2 = layers12(s, sx, s_h1);
#pragma unroll
        for (int v = 0; v < 16; ++v) s_h2[j * P2 + w * 32 + acc_row(v, h)] = h2[v];
        layer3_partial(s, h2, s_p);
        __syncthreads();
        if (t_ < WT) {       // d colour -> dz = 0.01 [g | g rgb], and the direct part of d rgb: g (1 + mul)
            const int row = t_;
            float y[NO];
            layer3_sum(s, s_p, row, y);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float g = s_dr[row * 4 + c], rgb = sx[row * P1 + c];
                s_dz[row * 8 + c] = 0.01f * g;
                s_dz[row * 8 + 3 + c] = 0.01f * (g * rgb);
                s_dr[row * 4 + c] = g * (1.f + y[3 + c]);
            }
        }
        __syncthreads();
        // dh2 = (W3^T dz) * (h2 > 0), this wave's block
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int o = w * 32 + acc_row(v, h);
            float d = 0.f;
#pragma unroll
            for (int k = 0; k < NO; ++k) d = fmaf(s.w3[k * NH + o], s_dz[j * 8 + k], d);
            s_dh2[j * P2 + o] = h2[v] > 0.f ? d : 0.f;
        }
        // dW3 += dz^T h2, db3 += sum dz (rows in order)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int e = t_ + q * WB, k = e >> 7, o = e & 127;
            float a = 0.f;
            for (int row = 0; row < WT; ++row) a = fmaf(s_dz[row * 8 + k], s_h2[row * P2 + o], a);
            g_w3[q] += a;      // (the tile's sum first: shorter accumulation chains)
        }
        if (t_ < NO) {
            float a = 0.f;
            for (int row = 0; row < WT; ++row) a += s_dz[row * 8 + t_];
            g_b3 += a;
        }
        __syncthreads();
        // dW2 += dh2^T h1 (the tile's rows are the contraction index), db2 += sum dh2
#pragma unroll
        for (int b = 0; b < 4; ++b) g_w2[b] = mfma_lds<16>(g_w2[b], s_dh2 + w * 32, 1, P2, s_h1 + b * 32, P2, 1);
        if (t_ < NH) {
            float a = 0.f;
            for (int row = 0; row < WT; ++row) a += s_dh2[row * P2 + t_];
            g_b += a;
        }
        // dh1 = (W2^T dh2) * (h1 > 0), this wave's block
        {
            const f32x16 a = mfma_lds<64>(zero16(), s.w2 + w * 32, 1, P2, s_dh2, 1, P2);
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int o = w * 32 + acc_row(v, h);
                s_dh1[j * P2 + o] = s_h1[j * P2 + o] > 0.f ? a[v] : 0.f;
            }
        }
        __syncthreads();
        // dW1[:, :27] += dh1^T x, sum dh1; dx = W1[:, :27]^T dh1 as four partials (one per wave's 32 hidden units)
        g_w1 = mfma_lds<16>(g_w1, s_dh1 + w * 32, 1, P2, sx, P1, 1);
        if (t_ >= NH) {
            float a = 0.f;
            for (int row = 0; row < WT; ++row) a += s_dh1[row * P2 + (t_ - NH)];
            g_b += a;
        }
        {
            const f32x16 a = mfma_lds<16>(zero16(), s.w1 + w * 32 * P1, 1, P1, s_dh1 + w * 32, 1, P2);
#pragma unroll
            for (int v = 0; v < 16; ++v) s_dx[(w * 32 + acc_row(v, h)) * 32 + j] = a[v];
        }
        __syncthreads();
        // d features_dc (through the clamp) and d features_rest[:24] (zeros behind them) of the tile's rows
        const int64_t wrow = 3 + d_rest_width;
        for (int e = t_; e < WT * wrow; e += WB) {
            const int row = (int)(e / wrow), c = (int)(e - row * wrow);
            const int64_t r = r0 + row;
            if (r >= n) continue;
            const int64_t g = R.gauss(r);
            float dx = 0.f;
            if (c < NF) {
                dx = s_dx[(0 * 32 + c) * 32 + row];
                dx += s_dx[(1 * 32 + c) * 32 + row];
                dx += s_dx[(2 * 32 + c) * 32 + row];
                dx += s_dx[(3 * 32 + c) * 32 + row];
            }
            if (c < 3)
                d_dc[g * 3 + c] = s_mask[row * 4 + c] != 0.f ? (s_dr[row * 4 + c] + dx) * C0 : 0.f;
            else
                d_rest[g * d_rest_width + (c - 3)] = dx;    // (c - 3 >= 24: dx = 0)
        }
        __syncthreads();
    }
    // this workgroup's partial sums
    float *p = partials + (int64_t)blockIdx.x * PART;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int o = w * 32 + acc_row(v, h);
#pragma unroll
        for (int b = 0; b < 4; ++b) p[OFF_W2 + o * NH + b * 32 + j] = g_w2[b][v];
        if (j < NF) p[OFF_W1 + o * NF + j] = g_w1[v];
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) p[OFF_W3 + t_ + q * WB] = g_w3[q];
    p[(t_ < NH ? OFF_B2 + t_ : OFF_S1 + t_ - NH)] = g_b;
    if (t_ < NO) p[OFF_B3 + t_] = g_b3;
}

// Fixed-order sum of the workgroups' partials (accumulated in double: up to 256 terms, and d e is a 128-term dot product of
// such sums with cancellation), scattered into the final layouts.  The LAST workgroup also forms the embedding
// parts: dW1[:, 27:59] = (sum dh1) e^T, d e = W1[:, 27:59]^T sum dh1.
constexpr int RB = 256;
__global__ __launch_bounds__(RB) void wild_reduce_kernel(int nb, const float *__restrict__ partials, const float *__restrict__ emb,
                                                         const float *__restrict__ w1, float *__restrict__ d_w1, float *__restrict__ d_b1,
                                                         float *__restrict__ d_w2, float *__restrict__ d_b2, float *__restrict__ d_w3,
                                                         float *__restrict__ d_b3, float *__restrict__ d_emb) {
    auto total = [&](int e) {
        double a = 0.0;
        for (int b = 0; b < nb; ++b) a += (double)partials[(int64_t)b * PART + e];
        return a;
    };
    if ((int)blockIdx.x == (int)gridDim.x - 1) {
        __shared__ double s1[NH];
        if (threadIdx.x < NH) s1[threadIdx.x] = total(OFF_S1 + threadIdx.x);
        __syncthreads();
        for (int e = threadIdx.x; e < NH * NE; e += RB) {
            const int o = e / NE, c = e - o * NE;
            d_w1[o * NIN + NF + c] = emb ? (float)(s1[o] * (double)emb[c]) : 0.f;
        }
        if (d_emb && threadIdx.x < NE) {
            double a = 0.0;
            for (int o = 0; o < NH; ++o) a += (double)w1[o * NIN + NF + threadIdx.x] * s1[o];
            d_emb[threadIdx.x] = (float)a;
        }
        return;
    }
    const int e = blockIdx.x * RB + threadIdx.x;
    if (e >= OFF_B3 + NO) return;
    const float a = (float)total(e);
    if (e < OFF_S1) d_w1[(e / NF) * NIN + e % NF] = a;
    else if (e < OFF_W2) d_b1[e - OFF_S1] = a;
    else if (e < OFF_B2) d_w2[e - OFF_W2] = a;
    else if (e < OFF_W3) d_b2[e - OFF_B2] = a;
    else if (e < OFF_B3) d_w3[e - OFF_W3] = a;
    else d_b3[e - OFF_B3] = a;
}

int grid_of(int64_t cap) { return (int)(cap < (int64_t)WILD_GRID * WT ? ceil_div64(cap, WT) : WILD_GRID); }

int check_widths(const char *fn, int n_feat, int n_embed, int n_hidden, int n_out) {
    MTGS_REQUIRE(n_feat == NF && n_embed == NE && n_hidden == NH && n_out == NO, MTGS_EUNSUPPORTED,
                 "%s: MLP widths %d+%d -> %d -> %d -> %d: only 27+32 -> 128 -> 128 -> 6 (WildGaussians.py's appearance MLP)", fn,
                 n_feat, n_embed, n_hidden, n_hidden, n_out);
    return MTGS_OK;
}

}  // namespace

#define WILD_WEIGHTS_NONNULL(fn) \
    MTGS_NONNULL(fn, w1); MTGS_NONNULL(fn, b1); MTGS_NONNULL(fn, w2); MTGS_NONNULL(fn, b2); MTGS_NONNULL(fn, w3); MTGS_NONNULL(fn, b3)

extern "C" int mtgs_wild_workspace_bytes(int64_t cap_rows, size_t *bytes) {
    MTGS_REQUIRE(cap_rows >= 0 && bytes, MTGS_EINVAL, "mtgs_wild_workspace_bytes: cap_rows < 0 or null pointer: bytes");
    *bytes = (size_t)grid_of(cap_rows) * PART * sizeof(float);
    return MTGS_OK;
}

extern "C" int mtgs_wild_fwd(int64_t cap_rows, const int32_t *vis_ids, const int64_t *totals, const uint8_t *row_flags,
                             const float *features_dc, int64_t dc_stride, const float *features_rest, int64_t rest_stride,
                             const float *embedding, const float *w1, const float *b1, const float *w2, const float *b2,
                             const float *w3, const float *b3, int n_feat, int n_embed, int n_hidden, int n_out, float *out,
                             int64_t out_stride, void *stream) {
    const char *fn = "mtgs_wild_fwd";
    if (int rc = check_widths(fn, n_feat, n_embed, n_hidden, n_out)) return rc;
    MTGS_REQUIRE(cap_rows >= 0 && dc_stride >= 3 && rest_stride >= 24 && out_stride >= 3, MTGS_EINVAL,
                 "mtgs_wild_fwd: bad sizes (cap_rows >= 0, dc_stride >= 3, rest_stride >= 24, out_stride >= 3)");
    MTGS_REQUIRE(!row_flags || vis_ids, MTGS_EINVAL, "mtgs_wild_fwd: row_flags need vis_ids");
    if (cap_rows == 0) return MTGS_OK;
    MTGS_NONNULL(fn, features_dc); MTGS_NONNULL(fn, features_rest); WILD_WEIGHTS_NONNULL(fn); MTGS_NONNULL(fn, out);
    MTGS_REQUIRE(!vis_ids || totals, MTGS_EINVAL, "mtgs_wild_fwd: null pointer: totals (vis_ids given)");
    const Weights W{embedding, w1, b1, w2, b2, w3, b3};
    wild_fwd_kernel<<<grid_of(cap_rows), WB, 0, (hipStream_t)stream>>>(Rows{vis_ids, totals, cap_rows}, row_flags, features_dc,
                                                                         dc_stride, features_rest, rest_stride, W, out, out_stride);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}

extern "C" int mtgs_wild_bwd(int64_t cap_rows, const int32_t *vis_ids, const int64_t *totals, const float *grad, int64_t grad_stride,
                             const float *features_dc, int64_t dc_stride, const float *features_rest, int64_t rest_stride,
                             const float *embedding, const float *w1, const float *b1, const float *w2, const float *b2,
                             const float *w3, const float *b3, int n_feat, int n_embed, int n_hidden, int n_out, float *d_dc,
                             float *d_rest, int64_t d_rest_width, float *partials, size_t ws_bytes, void *stream) {
    const char *fn = "mtgs_wild_bwd";
    if (int rc = check_widths(fn, n_feat, n_embed, n_hidden, n_out)) return rc;
    MTGS_REQUIRE(cap_rows >= 0 && grad_stride >= 3 && dc_stride >= 3 && rest_stride >= 24 && d_rest_width >= 24, MTGS_EINVAL,
                 "mtgs_wild_bwd: bad sizes (cap_rows >= 0, grad_stride >= 3, dc_stride >= 3, rest_stride >= 24, d_rest_width >= 24)");
    if (cap_rows == 0) return MTGS_OK;
    MTGS_NONNULL(fn, grad); MTGS_NONNULL(fn, features_dc); MTGS_NONNULL(fn, features_rest); WILD_WEIGHTS_NONNULL(fn);
    MTGS_NONNULL(fn, d_dc); MTGS_NONNULL(fn, d_rest); MTGS_NONNULL(fn, partials);
    MTGS_REQUIRE(!vis_ids || totals, MTGS_EINVAL, "mtgs_wild_bwd: null pointer: totals (vis_ids given)");
    const int grid = grid_of(cap_rows);
    MTGS_REQUIRE(ws_bytes >= (size_t)grid * PART * sizeof(float), MTGS_EWORKSPACE, "mtgs_wild_bwd: workspace %zu < %zu bytes", ws_bytes,
                 (size_t)grid * PART * sizeof(float));
    const Weights W{embedding, w1, b1, w2, b2, w3, b3};
    wild_bwd_kernel<<<grid, WB, 0, (hipStream_t)stream>>>(Rows{vis_ids, totals, cap_rows}, grad, grad_stride, features_dc, dc_stride,
                                                          features_rest, rest_stride, W, d_dc, d_rest, d_rest_width, partials);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}

extern "C" int mtgs_wild_reduce(int64_t cap_rows, const float *partials, const float *embedding, const float *w1, int n_feat,
                                int n_embed, int n_hidden, int n_out, float *d_w1, float *d_b1, float *d_w2, float *d_b2, float *d_w3,
                                float *d_b3, float *d_embed, void *stream) {
    const char *fn = "mtgs_wild_reduce";
    if (int rc = check_widths(fn, n_feat, n_embed, n_hidden, n_out)) return rc;
    MTGS_REQUIRE(cap_rows >= 0, MTGS_EINVAL, "mtgs_wild_reduce: cap_rows < 0");
    if (cap_rows == 0) return MTGS_OK;
    MTGS_NONNULL(fn, partials); MTGS_NONNULL(fn, w1); MTGS_NONNULL(fn, d_w1); MTGS_NONNULL(fn, d_b1); MTGS_NONNULL(fn, d_w2);
    MTGS_NONNULL(fn, d_b2); MTGS_NONNULL(fn, d_w3); MTGS_NONNULL(fn, d_b3);
    MTGS_REQUIRE(!d_embed || embedding, MTGS_EINVAL, "mtgs_wild_reduce: null pointer: embedding (d_embed given)");
    wild_reduce_kernel<<<(unsigned)ceil_div64(OFF_B3 + NO, RB) + 1, RB, 0, (hipStream_t)stream>>>(
        grid_of(cap_rows), partials, embedding, w1, d_w1, d_b1, d_w2, d_b2, d_w3, d_b3, d_embed);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}
