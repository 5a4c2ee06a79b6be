// dino.hip -- the DINOv2 similarity metric (include/mtgs_dino.h): Pillow's two-pass integer BILINEAR resample and centre crop of
// both images, the mask's NEAREST resize as patch weights, a ViT forward (patch embedding, `depth` blocks, final layer norm) and the
// weighted cosine tail.  No library kernels, no atomics, no host read, one stream.
//
//   dino_preprocess     one thread per pixel of the cropped S x S window of either image: for every vertical tap the horizontal
//                       pass of that source row (integer coefficients, 2^21 start, >> 22, clip) and then the vertical pass over
//                       those 8-bit values, as Pillow orders them; recomputing the horizontal pass per vertical tap keeps the
//                       launch free of an intermediate image (about 5 x 5 taps at 1080 -> 518).  Writes the normalised value into
//                       the patch matrix [2 G^2, 588] in the (c, ky, kx) order.
//   dino_patch_weights  one workgroup of 16 waves, the NEAREST tables in LDS: per patch the count of non-zero mask pixels behind its 196
//                       window pixels, four patches per wave in flight; counts are integers, so the weights and their sum do not
//                       depend on an order.
//   dino_gemm           the tile of mfma_f32_tile.hpp, 128 (M) x 64 (N) per workgroup (128 x 32 where that tile would make fewer than
//                       512 workgroups: N = 768 at 2740 rows is 264 of them on 256 CUs).  One lane's fma chain is RESTARTED every
//                       128 k's (K <= 128 is one chain): a single chain over K = 3072 measured 7.5e-6 on 768-wide features against
//                       2.5e-6 of the fp32 CPU restatement, outside the bound of tests/test_gpu_dino.py.  The last step is
//                       zero-filled beyond K (K = 588).  Epilogues: bias | bias, GELU | bias, gamma, + residual in place |
//                       bias + pos_embed with the row-to-token remap (and the two class rows).
//   dino_layernorm      one wave per row held in registers; the mean, then the variance about the mean, by wave_reduce_x4.
//   dino_attention      one workgroup per (image, head, 128 query rows), a wave per 32 of them; K and V blocks of 32 keys through
//                       LDS (shared by the four waves, the next block prefetched into registers); S = (q / 8) k^T by 32 MFMAs, through a
//                       per-wave LDS tile into "one lane per (row, half of the keys)" for the running maximum and the exponentials,
//                       P back through the same tile as the A operand of P V (the tile's k-steps, 32 MFMAs into two accumulators).
//   dino_cosine         one wave per patch: both rows in registers, two norms, the sum of the normalised products, x the weight.
//   dino_finish         one workgroup: the per-patch terms in a fixed tree, / the weight sum, or 0 when that is <= 1e-6.
#include <math.h>

#include "block_reduce.hpp"
#include "common.hpp"
#include "mfma_f32_tile.hpp"
#include "wave_reduce.hpp"

namespace {

constexpr int WIDE_GRID = 512;             // workgroups of 128 x 64 from which on that tile is used (two per CU); below: 128 x 32
constexpr int SEG = 128;                   // k's per fma chain of the GEMM
constexpr int PATCH = MTGS_DINO_PATCH, PP = PATCH * PATCH, PK = 3 * PP;       // 14, 196, 588
constexpr int HD = MTGS_DINO_HEAD_DIM;
constexpr int LN_Q = MTGS_DINO_MAX_DIM / 64;      // elements of a row per lane
constexpr int AQ = 32 * (TB / 64), AKB = 32;      // query rows per workgroup, keys per block
constexpr int SKS = HD + 1, SSS = AKB + 1;        // LDS row strides of the K tile and of the score tile
constexpr int PW_TB = 1024, PW_U = 4;
constexpr int MAX_S = 4096;                    // the largest network input side
constexpr int64_t LIMIT = (int64_t)1 << 31;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// every lane receives the sum over the wave, in one fixed order
__device__ __forceinline__ float wave_total(float s) {
    float in[4] = {s, s, s, s}, out[1];
    wave_reduce_x4<1>(in, out);
    return out[0];
}

// ---- preprocessing ---------------------------------------------------------------------------------------------------------
struct Tables {
    const int32_t *hb, *hc, *vb, *vc, *mx, *my;
};

__host__ __device__ inline Tables split_tables(const int32_t *t, int S, int hk, int vk) {
    Tables r;
    r.hb = t;
    r.hc = r.hb + 2 * (size_t)S;
    r.vb = r.hc + (size_t)S * hk;
    r.vc = r.vb + 2 * (size_t)S;
    r.mx = r.vc + (size_t)S * vk;
    r.my = r.mx + S;
    return r;
}

__global__ __launch_bounds__(TB) void dino_preprocess_kernel(int H, int W, int S, const float *__restrict__ img0, const float *__restrict__ img1,
                                                             const int32_t *__restrict__ tables, int hk, int vk, uint8_t *__restrict__ bytes,
                                                             float *__restrict__ patches) {
    const int e = blockIdx.x * TB + threadIdx.x;
    if (e >= 2 * S * S) return;
    const int x = e % S, y = (e / S) % S, im = e / (S * S);
    const Tables t = split_tables(tables, S, hk, vk);
    const float *img = im ? img1 : img0;
    const int xmin = t.hb[2 * x], xn = clampi(t.hb[2 * x + 1], 0, hk);
    const int ymin = t.vb[2 * y], yn = clampi(t.vb[2 * y + 1], 0, vk);
    int acc[3] = {1 << 21, 1 << 21, 1 << 21};
    for (int ty = 0; ty < yn; ++ty) {
        const int row = clampi(ymin + ty, 0, H - 1);
        int h[3] = {1 << 21, 1 << 21, 1 << 21};
        for (int tx = 0; tx < xn; ++tx) {
            const int col = clampi(xmin + tx, 0, W - 1);
            const int k = t.hc[(size_t)x * hk + tx];
            const float *p = img + ((size_t)row * W + col) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) h[c] += (int)(fminf(fmaxf(p[c], 0.f), 1.f) * 255.f) * k;
        }
        const int k = t.vc[(size_t)y * vk + ty];
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += clampi(h[c] >> 22, 0, 255) * k;
    }
    const int G = S / PATCH;
    const size_t prow = (size_t)im * G * G + (size_t)(y / PATCH) * G + x / PATCH;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int b = clampi(acc[c] >> 22, 0, 255);
        if (bytes != nullptr) bytes[(size_t)e * 3 + c] = (uint8_t)b;
        patches[prow * PK + c * PP + (y % PATCH) * PATCH + x % PATCH] = ((float)b / 255.f - 0.5f) / 0.5f;
    }
}

__global__ __launch_bounds__(PW_TB) void dino_patch_weights_kernel(int H, int W, int S, const uint8_t *__restrict__ mask,
                                                                   const int32_t *__restrict__ tables, int hk, int vk, float *__restrict__ weights) {
    __shared__ int s_total[PW_TB / 64];
    __shared__ int s_mx[MAX_S], s_my[MAX_S];               // the source column / row of every window column / row, clamped into the mask
    const int wv = threadIdx.x >> 6, l = threadIdx.x & 63;
    const Tables t = split_tables(tables, S, hk, vk);
    const int G = S / PATCH, G2 = G * G;
    for (int k = threadIdx.x; k < S; k += PW_TB) {
        s_mx[k] = clampi(t.mx[k], 0, W - 1);
        s_my[k] = clampi(t.my[k], 0, H - 1);
    }
    __syncthreads();
    int total = 0;
    for (int p0 = wv; p0 < G2; p0 += PW_U * (PW_TB / 64)) {          // PW_U patches per wave and turn: their loads are in flight together
        int cnt[PW_U];
#pragma unroll
        for (int u = 0; u < PW_U; ++u) {
            const int p = p0 + u * (PW_TB / 64);                      // the same for the whole wave
            const int pc = p < G2 ? p : G2 - 1, py = pc / G, px = pc - py * G;
            cnt[u] = 0;
#pragma unroll
            for (int j = 0; j < (PP + 63) / 64; ++j) {
                const int k = l + 64 * j, kc = k < PP ? k : PP - 1, ky = kc / PATCH, kx = kc - ky * PATCH;
                const int on = mask == nullptr ? 1 : (int)(mask[(size_t)s_my[py * PATCH + ky] * W + s_mx[px * PATCH + kx]] != 0);
                cnt[u] += (k < PP && p < G2) ? on : 0;
            }
        }
#pragma unroll
        for (int u = 0; u < PW_U; ++u) {
            const int c = wave_sum_all(cnt[u]);
            const int p = p0 + u * (PW_TB / 64);
            if (l == 0 && p < G2) weights[p] = (float)c / (float)PP;
            total += c;
        }
    }
    if (l == 0) s_total[wv] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        int sum = 0;
        for (int k = 0; k < PW_TB / 64; ++k) sum += s_total[k];
        weights[G2] = (float)sum / (float)PP;
    }
}

// ---- the GEMM --------------------------------------------------------------------------------------------------------------
struct Gemm {
    const float *a;         // [M, K]
    const float *w;         // [K][N]
    const float *bias;      // [N]
    const float *gamma;     // SCALE_RESIDUAL: [N]
    const float *pos;       // PATCH_EMBED: [tokens][N]
    const float *cls;       // PATCH_EMBED: [N]
    float *out;
    int M, N, K, epi, tokens;
};

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752440f)); }

// NH: 32-column halves of the output tile per workgroup (2: 128 x 64, 1: 128 x 32 for grids that would leave CUs idle)
template <bool VEC, int NH>
__global__ __launch_bounds__(TB, 4) void dino_gemm_kernel(Gemm c) {      // four workgroups per CU: at most 128 registers
    auto fetch_a = [&](int k0, float4 (&ra)[RA]) {
        const int k = k0 + 4 * tile_a_kq();        // K is a multiple of 4: the four elements stand or fall together
#pragma unroll
        for (int r = 0; r < RA; ++r) {
            const int m = blockIdx.x * BM + tile_a_row(r);
            ra[r] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (m < c.M && k < c.K) {
                const float *p = c.a + (size_t)m * c.K + k;
                if (VEC) ra[r] = *reinterpret_cast<const float4 *>(p);
                else ra[r] = make_float4(p[0], p[1], p[2], p[3]);
            }
        }
    };
    const int G2 = c.tokens - 1;                   // the column's bias and gamma are read once, then the epilogue of every row
    mfma_f32_tile<NH, SEG, false>(c.w, c.M, c.N, c.K, fetch_a, [&](int n) {
        const float b = c.bias[n];
        const float g = c.epi == MTGS_DINO_EPI_SCALE_RESIDUAL ? c.gamma[n] : 0.f;
        return [&c, G2, n, b, g](int m, float sum) {
            const float x = sum + b;
            if (c.epi == MTGS_DINO_EPI_BIAS) {
                c.out[(size_t)m * c.N + n] = x;
            } else if (c.epi == MTGS_DINO_EPI_BIAS_GELU) {
                c.out[(size_t)m * c.N + n] = gelu_erf(x);
            } else if (c.epi == MTGS_DINO_EPI_SCALE_RESIDUAL) {
                float *o = c.out + (size_t)m * c.N + n;
                *o = *o + g * x;
            } else {
                const int im = m / G2, p = m - im * G2;
                c.out[((size_t)im * c.tokens + 1 + p) * c.N + n] = x + c.pos[(size_t)(1 + p) * c.N + n];
            }
        };
    });
    const int t = threadIdx.x;
    if (c.epi == MTGS_DINO_EPI_PATCH_EMBED && blockIdx.x == 0 && t < 32 * NH) {   // the two class rows, this block's columns
        const int n = blockIdx.y * 32 * NH + t;
        const float v = c.cls[n] + c.pos[n];
        c.out[n] = v;
        c.out[(size_t)c.tokens * c.N + n] = v;
    }
}

// ---- layer norm -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TB) void dino_layernorm_kernel(int M, int D, float eps, const float *__restrict__ in, const float *__restrict__ w,
                                                            const float *__restrict__ b, float *__restrict__ out) {
    const int row = blockIdx.x * (TB / 64) + (threadIdx.x >> 6), l = threadIdx.x & 63;
    if (row >= M) return;                          // the whole wave; no barrier below
    const float *x = in + (size_t)row * D;
    float v[LN_Q], s = 0.f;
#pragma unroll
    for (int q = 0; q < LN_Q; ++q) {
        v[q] = l + 64 * q < D ? x[l + 64 * q] : 0.f;
        s += v[q];
    }
    const float mean = wave_total(s) / (float)D;
    float s2 = 0.f;
#pragma unroll
    for (int q = 0; q < LN_Q; ++q) {
        v[q] = l + 64 * q < D ? v[q] - mean : 0.f;
        s2 += v[q] * v[q];
    }
    const float r = 1.f / sqrtf(wave_total(s2) / (float)D + eps);
#pragma unroll
    for (int q = 0; q < LN_Q; ++q)
        if (l + 64 * q < D) out[(size_t)row * D + l + 64 * q] = v[q] * r * w[l + 64 * q] + b[l + 64 * q];
}

// ---- attention --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TB) void dino_attention_kernel(int T, int heads, const float *__restrict__ qkv, float *__restrict__ out) {
    __shared__ float sK[AKB * SKS];
    __shared__ __attribute__((aligned(16))) float sV[AKB * HD];
    __shared__ float sS[TB / 64][32 * SSS];
    __shared__ float sAl[TB / 64][32];
    const int t = threadIdx.x, wv = t >> 6, l = t & 63, i = l & 31, hh = l >> 5;
    const int D = heads * HD, ld = 3 * D;
    const int head = blockIdx.y, im = blockIdx.z, q0 = blockIdx.x * AQ + wv * 32;
    const float *base = qkv + (size_t)im * T * ld + head * HD;
    float *S = sS[wv], *Al = sAl[wv];

    float qr[HD / 2];                              // A operand of q k^T: q(i, 2s + hh) / 8 (64^-0.5, exact)
    {
        const bool ok = q0 + i < T;
        const float *q = base + (size_t)(ok ? q0 + i : 0) * ld;
#pragma unroll
        for (int s = 0; s < HD / 2; ++s) qr[s] = ok ? q[2 * s + hh] * 0.125f : 0.f;
    }

    // K / V loader: 32 keys x 16 float4 each, two per thread
    float4 rk[2], rv[2];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int idx = t + TB * r, key = idx >> 4, c4 = idx & 15;
            rk[r] = rv[r] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (k0 + key < T) {
                const float *p = base + (size_t)(k0 + key) * ld + 4 * c4;
                rk[r] = *reinterpret_cast<const float4 *>(p + D);
                rv[r] = *reinterpret_cast<const float4 *>(p + 2 * D);
            }
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int idx = t + TB * r, key = idx >> 4, c4 = idx & 15;
            float *d = sK + key * SKS + 4 * c4;
            d[0] = rk[r].x; d[1] = rk[r].y; d[2] = rk[r].z; d[3] = rk[r].w;
            *reinterpret_cast<float4 *>(sV + key * HD + 4 * c4) = rv[r];
        }
    };

    f32x16 o0, o1;
#pragma unroll
    for (int v = 0; v < 16; ++v) { o0[v] = 0.f; o1[v] = 0.f; }
    float m_run = -INFINITY, l_run = 0.f;          // of query row i, over the keys so far (both halves hold the same)

    fetch(0);
    stage();
    __syncthreads();
    for (int k0 = 0; k0 < T; k0 += AKB) {
        const bool more = k0 + AKB < T;
        if (more) fetch(k0 + AKB);
        // scores of this wave's 32 rows against the 32 keys; lane i holds key k0 + i
        f32x16 sc;
#pragma unroll
        for (int v = 0; v < 16; ++v) sc[v] = 0.f;
        const float *pk = sK + i * SKS + hh;
#pragma unroll
        for (int s = 0; s < HD / 2; ++s) sc = __builtin_amdgcn_mfma_f32_32x32x2f32(qr[s], pk[2 * s], sc, 0, 0, 0);
        const bool live = k0 + i < T;
#pragma unroll
        for (int v = 0; v < 16; ++v) S[acc_row(v, hh) * SSS + i] = live ? sc[v] : -INFINITY;
        __syncthreads();
        // lane (i, hh): row i, keys 16 hh .. 16 hh + 15
        float *ps = S + i * SSS + 16 * hh;
        float mx = ps[0];
#pragma unroll
        for (int j = 1; j < 16; ++j) mx = fmaxf(mx, ps[j]);
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);      // finite: key k0 is live in every block
        const float alpha = expf(m_run - m_new);
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float p = expf(ps[j] - m_new);
            ps[j] = p;
            sum += p;
        }
        sum += __shfl_xor(sum, 32, 64);
        l_run = l_run * alpha + sum;
        m_run = m_new;
        if (hh == 0) Al[i] = alpha;
        __syncthreads();
        // O = alpha O + P V
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const float al = Al[acc_row(v, hh)];
            o0[v] *= al;
            o1[v] *= al;
        }
        mfma_f32_ksteps<2, HD, AKB / 2>(S + i * SSS, sV, o0, o1);
        __syncthreads();
        if (more) {
            stage();
            __syncthreads();
        }
    }
    if (hh == 0) Al[i] = l_run;
    __syncthreads();
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int r = acc_row(v, hh), row = q0 + r;
        if (row >= T) continue;
        const float d = Al[r];
        float *o = out + ((size_t)im * T + row) * D + head * HD + i;
        o[0] = o0[v] / d;
        o[32] = o1[v] / d;
    }
}

// ---- the tail ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TB) void dino_cosine_kernel(int G2, int D, const float *__restrict__ fa, const float *__restrict__ fb,
                                                         const float *__restrict__ weights, float *__restrict__ terms) {
    const int p = blockIdx.x * (TB / 64) + (threadIdx.x >> 6), l = threadIdx.x & 63;
    if (p >= G2) return;                           // the whole wave; no barrier below
    const float *a = fa + (size_t)p * D, *b = fb + (size_t)p * D;
    float va[LN_Q], vb[LN_Q], sa = 0.f, sb = 0.f;
#pragma unroll
    for (int q = 0; q < LN_Q; ++q) {
        const bool ok = l + 64 * q < D;
        va[q] = ok ? a[l + 64 * q] : 0.f;
        vb[q] = ok ? b[l + 64 * q] : 0.f;
        sa += va[q] * va[q];
        sb += vb[q] * vb[q];
    }
    const float na = fmaxf(sqrtf(wave_total(sa)), 1e-8f), nb = fmaxf(sqrtf(wave_total(sb)), 1e-8f);
    float d = 0.f;
#pragma unroll
    for (int q = 0; q < LN_Q; ++q) d += (va[q] / na) * (vb[q] / nb);
    d = wave_total(d);
    if (l == 0) terms[p] = d * weights[p];
}

__global__ __launch_bounds__(TB) void dino_finish_kernel(int G2, const float *__restrict__ terms, const float *__restrict__ weights,
                                                         float *__restrict__ out) {
    __shared__ float s[TB];
    const int t = threadIdx.x;
    float v = 0.f;
    for (int p = t; p < G2; p += TB) v += terms[p];
    const float sum = block_tree_sum_f32<TB>(v, s);
    if (t == 0) {
        const float total = weights[G2];
        out[0] = total > 1e-6f ? sum / total : 0.f;
    }
}

__global__ __launch_bounds__(TB) void dino_gather_kernel(int G2, int T, int D4, const float4 *__restrict__ tokens, float4 *__restrict__ features, int n) {
    const int e = blockIdx.x * TB + threadIdx.x;
    if (e >= n) return;
    const int c = e % D4, r = e / D4, im = r / G2, p = r - im * G2;
    features[e] = tokens[((size_t)im * T + 1 + p) * D4 + c];
}

// ---- host -------------------------------------------------------------------------------------------------------------------
size_t round4(size_t n) { return (n + 3) & ~(size_t)3; }

struct Net {
    int dim, heads, depth, S, G, G2, T, hidden;
    float eps;
    size_t block_floats, total_floats;
    // workspace, in floats
    size_t patches, x, y, big, pw, terms, ws_floats;
};

int make_net(const char *fn, const mtgs_dino_config *cfg, Net &n) {
    MTGS_REQUIRE(cfg != nullptr, MTGS_EINVAL, "%s: null pointer: cfg", fn);
    MTGS_REQUIRE(cfg->dim > 0 && cfg->heads > 0 && cfg->depth > 0 && cfg->image > 0, MTGS_EINVAL,
                 "%s: dim %d, heads %d, depth %d and image %d must be positive", fn, cfg->dim, cfg->heads, cfg->depth, cfg->image);
    MTGS_REQUIRE(cfg->patch == PATCH, MTGS_EUNSUPPORTED, "%s: patch = %d: only %d is implemented", fn, cfg->patch, PATCH);
    MTGS_REQUIRE(cfg->mlp_ratio == 4, MTGS_EUNSUPPORTED, "%s: mlp_ratio = %d: only 4 is implemented", fn, cfg->mlp_ratio);
    MTGS_REQUIRE(cfg->dim == cfg->heads * HD, MTGS_EUNSUPPORTED, "%s: dim / heads = %d / %d: the head dimension must be %d", fn, cfg->dim,
                 cfg->heads, HD);
    MTGS_REQUIRE(cfg->dim <= MTGS_DINO_MAX_DIM, MTGS_EUNSUPPORTED, "%s: dim = %d exceeds %d", fn, cfg->dim, MTGS_DINO_MAX_DIM);
    MTGS_REQUIRE(cfg->image % PATCH == 0 && cfg->image <= MAX_S, MTGS_EINVAL, "%s: image = %d must be a multiple of the patch, at most 4096", fn, cfg->image);
    MTGS_REQUIRE(cfg->ln_eps > 0.f, MTGS_EINVAL, "%s: ln_eps must be positive", fn);
    n.dim = cfg->dim; n.heads = cfg->heads; n.depth = cfg->depth; n.S = cfg->image; n.eps = cfg->ln_eps;
    n.G = n.S / PATCH; n.G2 = n.G * n.G; n.T = n.G2 + 1; n.hidden = 4 * n.dim;
    const size_t d = (size_t)n.dim;
    n.block_floats = 2 * d + d * 3 * d + 3 * d + d * d + d + d + 2 * d + d * 4 * d + 4 * d + 4 * d * d + d + d;
    n.total_floats = (size_t)PK * d + d + d + (size_t)n.T * d + (size_t)n.depth * n.block_floats + 2 * d;
    MTGS_REQUIRE((int64_t)2 * n.T * n.hidden < LIMIT && (int64_t)2 * n.G2 * PK < LIMIT, MTGS_EUNSUPPORTED, "%s: an activation of 2^31 elements or more", fn);
    size_t o = 0;
    n.patches = o; o += round4((size_t)2 * n.G2 * PK);
    n.x = o; o += round4((size_t)2 * n.T * d);
    n.y = o; o += round4((size_t)2 * n.T * d);
    n.big = o; o += round4((size_t)2 * n.T * n.hidden);
    n.pw = o; o += round4((size_t)n.G2 + 1);
    n.terms = o; o += round4((size_t)n.G2);
    n.ws_floats = o;
    return MTGS_OK;
}

int launch_preprocess(const char *fn, int H, int W, int S, const float *pred, const float *gt, const int32_t *tables, int hk, int vk,
                      uint8_t *bytes, float *patches, hipStream_t st) {
    MTGS_REQUIRE(H > 0 && W > 0 && (int64_t)H * W * 3 < LIMIT, MTGS_EINVAL, "%s: a %d x %d image", fn, H, W);
    MTGS_REQUIRE(S > 0 && S % PATCH == 0 && S <= MAX_S, MTGS_EINVAL, "%s: S = %d must be a positive multiple of %d, at most 4096", fn, S, PATCH);
    MTGS_REQUIRE(hk > 0 && vk > 0, MTGS_EINVAL, "%s: tap counts hk = %d and vk = %d must be positive", fn, hk, vk);
    MTGS_REQUIRE(pred && gt && tables && patches, MTGS_EINVAL, "%s: null pointer: pred, gt, tables or patches", fn);
    dino_preprocess_kernel<<<(unsigned)ceil_div64((int64_t)2 * S * S, TB), TB, 0, st>>>(H, W, S, pred, gt, tables, hk, vk, bytes, patches);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}

int launch_patch_weights(const char *fn, int H, int W, int S, const uint8_t *mask, const int32_t *tables, int hk, int vk, float *weights,
                         hipStream_t st) {
    MTGS_REQUIRE(H > 0 && W > 0 && (int64_t)H * W < LIMIT, MTGS_EINVAL, "%s: a %d x %d mask", fn, H, W);
    MTGS_REQUIRE(S > 0 && S % PATCH == 0 && S <= MAX_S, MTGS_EINVAL, "%s: S = %d must be a positive multiple of %d, at most 4096", fn, S, PATCH);
    MTGS_REQUIRE(hk > 0 && vk > 0, MTGS_EINVAL, "%s: tap counts hk = %d and vk = %d must be positive", fn, hk, vk);
    MTGS_REQUIRE(tables && weights, MTGS_EINVAL, "%s: null pointer: tables or weights", fn);
    dino_patch_weights_kernel<<<1, PW_TB, 0, st>>>(H, W, S, mask, tables, hk, vk, weights);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}

int launch_gemm(const char *fn, Gemm c, hipStream_t st) {
    MTGS_REQUIRE(c.M > 0 && c.N > 0 && c.K > 0, MTGS_EINVAL, "%s: M = %d, K = %d and N = %d must be positive", fn, c.M, c.K, c.N);
    MTGS_REQUIRE(c.N % BN == 0, MTGS_EUNSUPPORTED, "%s: N = %d is not a multiple of %d", fn, c.N, BN);
    MTGS_REQUIRE(c.K % 4 == 0, MTGS_EUNSUPPORTED, "%s: K = %d is not a multiple of 4", fn, c.K);
    MTGS_REQUIRE(c.a && c.w && c.bias && c.out, MTGS_EINVAL, "%s: null pointer: a, w, bias or out", fn);
    MTGS_REQUIRE(c.epi >= MTGS_DINO_EPI_BIAS && c.epi <= MTGS_DINO_EPI_PATCH_EMBED, MTGS_EINVAL, "%s: unknown epilogue %d", fn, c.epi);
    MTGS_REQUIRE(c.epi != MTGS_DINO_EPI_SCALE_RESIDUAL || c.gamma, MTGS_EINVAL, "%s: null pointer: gamma", fn);
    int64_t rows = c.M;
    if (c.epi == MTGS_DINO_EPI_PATCH_EMBED) {
        MTGS_REQUIRE(c.pos && c.cls, MTGS_EINVAL, "%s: null pointer: pos or cls", fn);
        MTGS_REQUIRE(c.tokens > 1 && c.M == 2 * (c.tokens - 1), MTGS_EINVAL, "%s: the patch embedding takes M = 2 (tokens - 1) rows, got M = %d, tokens = %d",
                     fn, c.M, c.tokens);
        rows = 2 * (int64_t)c.tokens;
    } else {
        c.tokens = 2;                              // G2 = 1: never read, never a divisor of 0
    }
    MTGS_REQUIRE((((uintptr_t)c.w | (uintptr_t)c.out) & 15) == 0, MTGS_EINVAL, "%s: w and out must be 16-byte aligned", fn);
    MTGS_REQUIRE(rows * c.N < LIMIT && (int64_t)c.M * c.K < LIMIT && (int64_t)c.K * c.N < LIMIT, MTGS_EUNSUPPORTED, "%s: an array of 2^31 elements or more", fn);
    const bool vec = ((uintptr_t)c.a & 15) == 0;
    const int64_t row_tiles = ceil_div64(c.M, BM);
    if (row_tiles * (c.N / BN) >= WIDE_GRID) {
        const dim3 grid((unsigned)row_tiles, (unsigned)(c.N / BN));
        if (vec) dino_gemm_kernel<true, 2><<<grid, TB, 0, st>>>(c);
        else dino_gemm_kernel<false, 2><<<grid, TB, 0, st>>>(c);
    } else {
        const dim3 grid((unsigned)row_tiles, (unsigned)(c.N / 32));
        if (vec) dino_gemm_kernel<true, 1><<<grid, TB, 0, st>>>(c);
        else dino_gemm_kernel<false, 1><<<grid, TB, 0, st>>>(c);
    }
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}

int launch_layernorm(const char *fn, int M, int D, float eps, const float *in, const float *w, const float *b, float *out, hipStream_t st) {
    MTGS_REQUIRE(M > 0 && D > 0, MTGS_EINVAL, "%s: M = %d and D = %d must be positive", fn, M, D);
    MTGS_REQUIRE(D % 64 == 0 && D <= MTGS_DINO_MAX_DIM, MTGS_EUNSUPPORTED, "%s: D = %d must be a multiple of 64, at most %d", fn, D, MTGS_DINO_MAX_DIM);
    MTGS_REQUIRE(eps > 0.f, MTGS_EINVAL, "%s: eps must be positive", fn);
    MTGS_REQUIRE(in && w && b && out, MTGS_EINVAL, "%s: null pointer: in, w, b or out", fn);
    MTGS_REQUIRE((int64_t)M * D < LIMIT, MTGS_EUNSUPPORTED, "%s: an array of 2^31 elements or more", fn);
    dino_layernorm_kernel<<<(unsigned)ceil_div64(M, TB / 64), TB, 0, st>>>(M, D, eps, in, w, b, out);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}

int launch_attention(const char *fn, int n, int T, int heads, const float *qkv, float *out, hipStream_t st) {
    MTGS_REQUIRE(n > 0 && T > 0 && heads > 0, MTGS_EINVAL, "%s: n = %d, T = %d and heads = %d must be positive", fn, n, T, heads);
    MTGS_REQUIRE(n <= 65535 && heads <= 65535, MTGS_EUNSUPPORTED, "%s: n = %d or heads = %d exceeds 65535", fn, n, heads);
    MTGS_REQUIRE(qkv && out, MTGS_EINVAL, "%s: null pointer: qkv or out", fn);
    MTGS_REQUIRE(((uintptr_t)qkv & 15) == 0, MTGS_EINVAL, "%s: qkv must be 16-byte aligned", fn);
    MTGS_REQUIRE((int64_t)n * T * heads * HD * 3 < LIMIT, MTGS_EUNSUPPORTED, "%s: an array of 2^31 elements or more", fn);
    const dim3 grid((unsigned)ceil_div64(T, AQ), (unsigned)heads, (unsigned)n);
    dino_attention_kernel<<<grid, TB, 0, st>>>(T, heads, qkv, out);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}

int launch_tail(const char *fn, int G2, int D, const float *a, const float *b, const float *weights, float *scratch, float *out, hipStream_t st) {
    MTGS_REQUIRE(G2 > 0 && D > 0, MTGS_EINVAL, "%s: G2 = %d and D = %d must be positive", fn, G2, D);
    MTGS_REQUIRE(D <= MTGS_DINO_MAX_DIM, MTGS_EUNSUPPORTED, "%s: D = %d exceeds %d", fn, D, MTGS_DINO_MAX_DIM);
    MTGS_REQUIRE(a && b && weights && scratch && out, MTGS_EINVAL, "%s: null pointer: a, b, weights, scratch or out", fn);
    dino_cosine_kernel<<<(unsigned)ceil_div64(G2, TB / 64), TB, 0, st>>>(G2, D, a, b, weights, scratch);
    MTGS_CHECK_LAUNCH(fn);
    dino_finish_kernel<<<1, TB, 0, st>>>(G2, scratch, weights, out);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}

// steps 1 and 3: the final layer norm's output, all 2 T rows, is left at ws + n.y
int run_network(const char *fn, const Net &n, int H, int W, const float *pred, const float *gt, const int32_t *tables, int hk, int vk,
                const float *weights, float *ws, hipStream_t st) {
    const size_t d = (size_t)n.dim;
    const int M = 2 * n.T;
    float *patches = ws + n.patches, *x = ws + n.x, *y = ws + n.y, *big = ws + n.big;
    if (int rc = launch_preprocess(fn, H, W, n.S, pred, gt, tables, hk, vk, nullptr, patches, st)) return rc;
    const float *p = weights;
    auto take = [&](size_t count) { const float *r = p; p += count; return r; };
    {
        Gemm c{};
        c.a = patches; c.w = take((size_t)PK * d); c.bias = take(d); c.cls = take(d); c.pos = take((size_t)n.T * d); c.out = x;
        c.M = 2 * n.G2; c.N = n.dim; c.K = PK; c.epi = MTGS_DINO_EPI_PATCH_EMBED; c.tokens = n.T;
        if (int rc = launch_gemm(fn, c, st)) return rc;
    }
    auto linear = [&](const float *a, int K, int N, int epi, const float *gamma, float *out) {
        Gemm c{};
        c.a = a; c.w = take((size_t)K * N); c.bias = take((size_t)N); c.gamma = gamma; c.out = out;
        c.M = M; c.N = N; c.K = K; c.epi = epi;
        return launch_gemm(fn, c, st);
    };
    for (int blk = 0; blk < n.depth; ++blk) {
        const float *w1 = take(d), *b1 = take(d);
        if (int rc = launch_layernorm(fn, M, n.dim, n.eps, x, w1, b1, y, st)) return rc;
        if (int rc = linear(y, n.dim, 3 * n.dim, MTGS_DINO_EPI_BIAS, nullptr, big)) return rc;
        if (int rc = launch_attention(fn, 2, n.T, n.heads, big, y, st)) return rc;
        const float *ls1 = p + d * d + d;            // behind proj and its bias
        if (int rc = linear(y, n.dim, n.dim, MTGS_DINO_EPI_SCALE_RESIDUAL, ls1, x)) return rc;
        take(d);
        const float *w2 = take(d), *b2 = take(d);
        if (int rc = launch_layernorm(fn, M, n.dim, n.eps, x, w2, b2, y, st)) return rc;
        if (int rc = linear(y, n.dim, n.hidden, MTGS_DINO_EPI_BIAS_GELU, nullptr, big)) return rc;
        const float *ls2 = p + (size_t)n.hidden * d + d;
        if (int rc = linear(big, n.hidden, n.dim, MTGS_DINO_EPI_SCALE_RESIDUAL, ls2, x)) return rc;
        take(d);
    }
    const float *wn = take(d), *bn = take(d);
    return launch_layernorm(fn, M, n.dim, n.eps, x, wn, bn, y, st);
}

int check_run(const char *fn, const Net &n, const void *weights, const void *ws, size_t ws_bytes) {
    MTGS_REQUIRE(weights && ws, MTGS_EINVAL, "%s: null pointer: weights or ws", fn);
    MTGS_REQUIRE((((uintptr_t)ws | (uintptr_t)weights) & 15) == 0, MTGS_EINVAL, "%s: ws and weights must be 16-byte aligned", fn);
    MTGS_REQUIRE(ws_bytes >= n.ws_floats * sizeof(float), MTGS_EWORKSPACE, "%s: workspace %zu < %zu bytes", fn, ws_bytes, n.ws_floats * sizeof(float));
    return MTGS_OK;
}

}  // namespace

extern "C" int mtgs_dino_weight_floats(const mtgs_dino_config *cfg, size_t *floats) {
    const char *fn = "mtgs_dino_weight_floats";
    MTGS_REQUIRE(floats != nullptr, MTGS_EINVAL, "%s: null pointer: floats", fn);
    Net n;
    if (int rc = make_net(fn, cfg, n)) return rc;
    *floats = n.total_floats;
    return MTGS_OK;
}

extern "C" int mtgs_dino_workspace_bytes(const mtgs_dino_config *cfg, size_t *bytes) {
    const char *fn = "mtgs_dino_workspace_bytes";
    MTGS_REQUIRE(bytes != nullptr, MTGS_EINVAL, "%s: null pointer: bytes", fn);
    Net n;
    if (int rc = make_net(fn, cfg, n)) return rc;
    *bytes = n.ws_floats * sizeof(float);
    return MTGS_OK;
}

extern "C" int mtgs_dino_preprocess(int H, int W, int S, const float *pred, const float *gt, const int32_t *tables, int hk, int vk,
                                    uint8_t *bytes, float *patches, void *stream) {
    return launch_preprocess("mtgs_dino_preprocess", H, W, S, pred, gt, tables, hk, vk, bytes, patches, (hipStream_t)stream);
}

extern "C" int mtgs_dino_patch_weights(int H, int W, int S, const uint8_t *mask, const int32_t *tables, int hk, int vk, float *weights,
                                       void *stream) {
    return launch_patch_weights("mtgs_dino_patch_weights", H, W, S, mask, tables, hk, vk, weights, (hipStream_t)stream);
}

extern "C" int mtgs_dino_linear(int M, int K, int N, const float *a, const float *w, const float *bias, int epilogue, const float *gamma,
                                const float *pos, const float *cls, int tokens, float *out, void *stream) {
    Gemm c{};
    c.a = a; c.w = w; c.bias = bias; c.gamma = gamma; c.pos = pos; c.cls = cls; c.out = out;
    c.M = M; c.N = N; c.K = K; c.epi = epilogue; c.tokens = tokens;
    return launch_gemm("mtgs_dino_linear", c, (hipStream_t)stream);
}

extern "C" int mtgs_dino_layernorm(int M, int D, float eps, const float *in, const float *w, const float *b, float *out, void *stream) {
    return launch_layernorm("mtgs_dino_layernorm", M, D, eps, in, w, b, out, (hipStream_t)stream);
}

extern "C" int mtgs_dino_attention(int n, int T, int heads, const float *qkv, float *out, void *stream) {
    return launch_attention("mtgs_dino_attention", n, T, heads, qkv, out, (hipStream_t)stream);
}

extern "C" int mtgs_dino_tail(int G2, int D, const float *a, const float *b, const float *weights, float *scratch, float *out, void *stream) {
    return launch_tail("mtgs_dino_tail", G2, D, a, b, weights, scratch, out, (hipStream_t)stream);
}

extern "C" int mtgs_dino_features(const mtgs_dino_config *cfg, int H, int W, const float *pred, const float *gt, const int32_t *tables, int hk,
                                  int vk, const float *weights, float *features, void *ws, size_t ws_bytes, void *stream) {
    const char *fn = "mtgs_dino_features";
    Net n;
    if (int rc = make_net(fn, cfg, n)) return rc;
    if (int rc = check_run(fn, n, weights, ws, ws_bytes)) return rc;
    MTGS_REQUIRE(features != nullptr && ((uintptr_t)features & 15) == 0, MTGS_EINVAL, "%s: features must be a 16-byte aligned pointer", fn);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = run_network(fn, n, H, W, pred, gt, tables, hk, vk, weights, (float *)ws, st)) return rc;
    const int count = 2 * n.G2 * (n.dim / 4);
    dino_gather_kernel<<<(unsigned)ceil_div64(count, TB), TB, 0, st>>>(n.G2, n.T, n.dim / 4, (const float4 *)((float *)ws + n.y), (float4 *)features, count);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}

extern "C" int mtgs_dino_similarity(const mtgs_dino_config *cfg, int H, int W, const float *pred, const float *gt, const uint8_t *mask,
                                    const int32_t *tables, int hk, int vk, const float *weights, float *out, void *ws, size_t ws_bytes,
                                    void *stream) {
    const char *fn = "mtgs_dino_similarity";
    Net n;
    if (int rc = make_net(fn, cfg, n)) return rc;
    if (int rc = check_run(fn, n, weights, ws, ws_bytes)) return rc;
    MTGS_REQUIRE(out != nullptr, MTGS_EINVAL, "%s: null pointer: out", fn);
    hipStream_t st = (hipStream_t)stream;
    float *f = (float *)ws;
    if (int rc = launch_patch_weights(fn, H, W, n.S, mask, tables, hk, vk, f + n.pw, st)) return rc;
    if (int rc = run_network(fn, n, H, W, pred, gt, tables, hk, vk, weights, f, st)) return rc;
    const float *y = f + n.y;
    return launch_tail(fn, n.G2, n.dim, y + n.dim, y + ((size_t)n.T + 1) * n.dim, f + n.pw, f + n.terms, out, st);
}
