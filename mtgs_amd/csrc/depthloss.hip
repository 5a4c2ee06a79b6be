// depthloss.hip -- the "pseudo" depth branch of get_loss_dict (mtgs_scene_graph.py:844-873): the rendered depth against the
// dense monocular depth image, by one of the losses of mtgs/utils/geometric_loss.py:16-256 ("scalar" implementation), with
// e = pred - gt over the n pixels of m = (gt > lo) & (gt < hi) & mask:
//     mse             mean(e^2)
//     L1              mean(|e|)
//     InverseL1       mean(|1 / (pred + 1e-6) - 1 / (gt + 1e-6)|)        (1e-6: not the 1e-5 of the lidar branch)
//     LogL1           mean(log(1 + |e|))
//     HuberL1         d = thresh max|e|;  mean(|e| < d ? (e^2 + d^2) / (2 d) : |e|)     (its own gt != 0 mask is applied too)
//     EdgeAwareLogL1  sum_x / n_x + sum_y / n_y,  Lx[v,u] = exp(-mean_c |rgb[v,u,c] - rgb[v,u+1,c]|) log(1 + |e[v,u]|) over the
//                     selected pixels with u < W - 1, Ly the same downwards over those with v < H - 1.  Only the mask of the
//                     pixel itself is consulted and only its depth is read, as in the reference.
// PyTorch: pred[m] / gt[m] (nonzero + gather: a host read of the count every step) and `if m.sum() == 0` (another one).  Here
// the selection is evaluated inside the kernels and the empty case (value 0, zero gradient) is decided on the device.
//
// Forward: a grid-stride pass writes per-block partials, a single-workgroup finish adds them in a fixed order in fp64 and
// writes the record out[MTGS_DEPTH_LOSS_RECORD_FLOATS] = {loss, n, n_x, n_y, d, dL/dd, ties, max|e|}.  HuberL1 needs the
// maximum before the sum: a max / count pass and its finish come first, the sum pass reads d and the maximum from the record.
// Backward: one element-wise kernel that writes EVERY pixel (zero outside the selection) from the record and the device
// cotangent.  d is differentiable: dL/dd = (1/n) sum_{|e| < d} (1/2 - e^2 / (2 d^2)) reaches, through thresh * max|e|, the
// selected pixels that attain the maximum, shared evenly among ties (torch.max() over a whole tensor).
//
// Compiled with -ffp-contract=off (build.py) so every expression rounds as the reference's per-operation kernels do.  No float
// atomics: every reduction is in a fixed order, so results are bitwise reproducible; nothing is read back to the host and
// nothing is allocated here, so every entry point can be captured in a HIP graph.
#include "common.hpp"
#include "block_reduce.hpp"

namespace {
constexpr int DL_BLOCK = 256;
constexpr int DL_MAX_BLOCKS = 1024;      // forward launch cap (4 workgroups for each of the 256 CUs); the passes stride over the rest
constexpr int DL_PARTS = 5;              // partials per block (the widest pass: sum_x, sum_y, n_x, n_y, n)
static_assert(MTGS_DEPTH_LOSS_RECORD_FLOATS == 8, "the record's layout is part of the ABI");
enum { R_LOSS = 0, R_N = 1, R_NX = 2, R_NY = 3, R_D = 4, R_DLDD = 5, R_TIES = 6, R_MAX = 7 };

// (gt > lo) & (gt < hi) & mask, strict and in fp32; HuberL1 also applies its own gt != 0
template <int KIND>
__device__ __forceinline__ bool selected(float g, int64_t p, const uint8_t *__restrict__ mask, float lo, float hi) {
    if (KIND == MTGS_DEPTH_LOSS_HUBER_L1 && g == 0.f) return false;
    return g > lo && g < hi && (mask == nullptr || mask[p] != 0);
}

// exp(-mean_c |rgb[p, c] - rgb[q, c]|)
__device__ __forceinline__ float edge_weight(const float *__restrict__ rgb, int64_t p, int64_t q) {
    const float s = (fabsf(rgb[p * 3] - rgb[q * 3]) + fabsf(rgb[p * 3 + 1] - rgb[q * 3 + 1])) + fabsf(rgb[p * 3 + 2] - rgb[q * 3 + 2]);
    return expf(-(s / 3.f));
}

// the per-pixel term of the kinds that are a plain mean
template <int KIND>
__device__ __forceinline__ float pixel_term(float q, float g) {
    if (KIND == MTGS_DEPTH_LOSS_MSE) { const float e = q - g; return e * e; }
    if (KIND == MTGS_DEPTH_LOSS_L1) return fabsf(q - g);
    if (KIND == MTGS_DEPTH_LOSS_INVERSE_L1) return fabsf(1.f / (q + 1e-6f) - 1.f / (g + 1e-6f));
    return logf(1.f + fabsf(q - g));      // LogL1
}

__device__ __forceinline__ void write_parts(float *__restrict__ partials, const float (&v)[DL_PARTS]) {
    if (threadIdx.x == 0) {
        float *o = partials + (int64_t)blockIdx.x * DL_PARTS;
#pragma unroll
        for (int j = 0; j < DL_PARTS; ++j) o[j] = v[j];
    }
}

// mse, L1, InverseL1, LogL1: partials {sum, 0, 0, 0, n}
template <int KIND>
__global__ __launch_bounds__(DL_BLOCK) void depth_mean_fwd_kernel(int64_t P, const float *__restrict__ pred, const float *__restrict__ gt,
                                                                  const uint8_t *__restrict__ mask, float lo, float hi,
                                                                  float *__restrict__ partials) {
    __shared__ float s_red[4];
    float sum = 0.f, cnt = 0.f;
    for (int64_t p = (int64_t)blockIdx.x * DL_BLOCK + threadIdx.x; p < P; p += (int64_t)gridDim.x * DL_BLOCK) {
        const float g = gt[p];
        if (selected<KIND>(g, p, mask, lo, hi)) {
            sum += pixel_term<KIND>(pred[p], g);
            cnt += 1.f;
        }
    }
    const float v[DL_PARTS] = {block_sum4(sum, s_red), 0.f, 0.f, 0.f, block_sum4(cnt, s_red)};
    write_parts(partials, v);
}

// EdgeAwareLogL1: partials {sum_x, sum_y, n_x, n_y, n}
__global__ __launch_bounds__(DL_BLOCK) void depth_edge_fwd_kernel(int W, int H, const float *__restrict__ pred, const float *__restrict__ gt,
                                                                  const uint8_t *__restrict__ mask, const float *__restrict__ rgb,
                                                                  float lo, float hi, float *__restrict__ partials) {
    __shared__ float s_red[4];
    const int64_t P = (int64_t)W * H;
    float sx = 0.f, sy = 0.f, nx = 0.f, ny = 0.f, cnt = 0.f;
    for (int64_t p = (int64_t)blockIdx.x * DL_BLOCK + threadIdx.x; p < P; p += (int64_t)gridDim.x * DL_BLOCK) {
        const float g = gt[p];
        if (!selected<MTGS_DEPTH_LOSS_EDGE_AWARE_LOG_L1>(g, p, mask, lo, hi)) continue;
        const int u = (int)(p % W), v = (int)(p / W);
        const float l = logf(1.f + fabsf(pred[p] - g));
        cnt += 1.f;
        if (u + 1 < W) { sx += edge_weight(rgb, p, p + 1) * l; nx += 1.f; }
        if (v + 1 < H) { sy += edge_weight(rgb, p, p + W) * l; ny += 1.f; }
    }
    const float v[DL_PARTS] = {block_sum4(sx, s_red), block_sum4(sy, s_red), block_sum4(nx, s_red), block_sum4(ny, s_red),
                               block_sum4(cnt, s_red)};
    write_parts(partials, v);
}

// |e| >= 0, so the order of the bit patterns is the order of the values, and a NaN (above +inf) wins as it does in torch.max
__device__ __forceinline__ int abs_bits(float e) { return __builtin_bit_cast(int, fabsf(e)); }

// HuberL1, pass 1: partials {max|e| (its bits), 0, 0, 0, n}
__global__ __launch_bounds__(DL_BLOCK) void depth_huber_max_kernel(int64_t P, const float *__restrict__ pred, const float *__restrict__ gt,
                                                                   const uint8_t *__restrict__ mask, float lo, float hi,
                                                                   float *__restrict__ partials) {
    __shared__ float s_red[4];
    __shared__ int s_max[4];
    int mx = 0;
    float cnt = 0.f;
    for (int64_t p = (int64_t)blockIdx.x * DL_BLOCK + threadIdx.x; p < P; p += (int64_t)gridDim.x * DL_BLOCK) {
        const float g = gt[p];
        if (selected<MTGS_DEPTH_LOSS_HUBER_L1>(g, p, mask, lo, hi)) {
            mx = max(mx, abs_bits(pred[p] - g));
            cnt += 1.f;
        }
    }
    mx = wave_max_i32(mx);
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = mx;
    cnt = block_sum4(cnt, s_red);        // (its barriers also publish s_max)
    if (threadIdx.x == 0) {
        float *o = partials + (int64_t)blockIdx.x * DL_PARTS;
        o[0] = __builtin_bit_cast(float, max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3])));
        o[1] = 0.f; o[2] = 0.f; o[3] = 0.f;
        o[4] = cnt;
    }
}

// HuberL1, finish of pass 1: the record's n, max|e| and d = thresh * max|e| (fp32, as thresh * torch.max(l1))
__global__ __launch_bounds__(DL_BLOCK) void depth_huber_max_finish_kernel(int64_t nblocks, float thresh, const float *__restrict__ partials,
                                                                          float *__restrict__ out) {
    __shared__ int s_max[DL_BLOCK];
    __shared__ double s_cnt[DL_BLOCK];
    int mx = 0;
    double cnt = 0.0;
    for (int64_t i = threadIdx.x; i < nblocks; i += DL_BLOCK) {
        mx = max(mx, __builtin_bit_cast(int, partials[i * DL_PARTS]));
        cnt += (double)partials[i * DL_PARTS + 4];
    }
    s_max[threadIdx.x] = mx;
    cnt = block_tree_sum_f64<DL_BLOCK>(cnt, s_cnt);      // (s_max is published by its first barrier)
    for (int o = DL_BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s_max[threadIdx.x] = max(s_max[threadIdx.x], s_max[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const float m = __builtin_bit_cast(float, s_max[0]);
    out[R_N] = (float)cnt;
    out[R_MAX] = m;
    out[R_D] = thresh * m;
}

// HuberL1, pass 2: partials {sum, sum of (1/2 - e^2 / (2 d^2)) over the quadratic branch, pixels at the maximum, 0, n}
__global__ __launch_bounds__(DL_BLOCK) void depth_huber_sum_kernel(int64_t P, const float *__restrict__ pred, const float *__restrict__ gt,
                                                                   const uint8_t *__restrict__ mask, float lo, float hi,
                                                                   const float *__restrict__ rec, float *__restrict__ partials) {
    __shared__ float s_red[4];
    const float d = rec[R_D], m = rec[R_MAX];
    float sum = 0.f, dd = 0.f, ties = 0.f, cnt = 0.f;
    for (int64_t p = (int64_t)blockIdx.x * DL_BLOCK + threadIdx.x; p < P; p += (int64_t)gridDim.x * DL_BLOCK) {
        const float g = gt[p];
        if (!selected<MTGS_DEPTH_LOSS_HUBER_L1>(g, p, mask, lo, hi)) continue;
        const float e = pred[p] - g, a = fabsf(e);
        cnt += 1.f;
        if (a < d) {          // (never with d = 0: no 0 / 0)
            sum += (e * e + d * d) / (2.f * d);
            dd += 0.5f - (e * e) / ((2.f * d) * d);
        } else {
            sum += a;
        }
        if (a == m) ties += 1.f;
    }
    const float v[DL_PARTS] = {block_sum4(sum, s_red), block_sum4(dd, s_red), block_sum4(ties, s_red), 0.f, block_sum4(cnt, s_red)};
    write_parts(partials, v);
}

// The record.  n = 0: the loss is 0 (the reference's `if depth_loss_mask.sum() == 0`); n > 0 with n_x = 0 or n_y = 0: that
// term is 0 / 0 = NaN, as torch's mean of an empty tensor.
__global__ __launch_bounds__(DL_BLOCK) void depth_loss_finish_kernel(int kind, int64_t nblocks, const float *__restrict__ partials,
                                                                     float *__restrict__ out) {
    double s[DL_PARTS];
    finish_sums<DL_PARTS, DL_BLOCK>(nblocks, partials, s);
    if (threadIdx.x != 0) return;
    const double n = s[4];
    out[R_N] = (float)n;
    if (kind == MTGS_DEPTH_LOSS_EDGE_AWARE_LOG_L1) {
        const float nan = __builtin_nanf("");
        const float a = s[2] > 0.0 ? (float)(s[0] / s[2]) : nan, b = s[3] > 0.0 ? (float)(s[1] / s[3]) : nan;
        out[R_LOSS] = n > 0.0 ? a + b : 0.f;
        out[R_NX] = (float)s[2];
        out[R_NY] = (float)s[3];
        out[R_D] = 0.f; out[R_DLDD] = 0.f; out[R_TIES] = 0.f; out[R_MAX] = 0.f;
        return;
    }
    out[R_LOSS] = n > 0.0 ? (float)(s[0] / n) : 0.f;
    out[R_NX] = 0.f;
    out[R_NY] = 0.f;
    if (kind == MTGS_DEPTH_LOSS_HUBER_L1) {      // (d and max|e| are pass 1's)
        out[R_DLDD] = n > 0.0 ? (float)(s[1] / n) : 0.f;
        out[R_TIES] = (float)s[2];
    } else {
        out[R_D] = 0.f; out[R_DLDD] = 0.f; out[R_TIES] = 0.f; out[R_MAX] = 0.f;
    }
}

__global__ __launch_bounds__(DL_BLOCK) void depth_loss_bwd_kernel(int kind, int W, int H, const float *__restrict__ pred,
                                                                  const float *__restrict__ gt, const uint8_t *__restrict__ mask,
                                                                  const float *__restrict__ rgb, float lo, float hi, float thresh,
                                                                  const float *__restrict__ v_out, const float *__restrict__ rec,
                                                                  float *__restrict__ v_pred) {
    const int64_t p = (int64_t)blockIdx.x * DL_BLOCK + threadIdx.x;
    if (p >= (int64_t)W * H) return;
    const float v = v_out[0], n = rec[R_N];
    const float g = gt[p];
    const bool sel = kind == MTGS_DEPTH_LOSS_HUBER_L1 ? selected<MTGS_DEPTH_LOSS_HUBER_L1>(g, p, mask, lo, hi)
                                                      : selected<MTGS_DEPTH_LOSS_MSE>(g, p, mask, lo, hi);
    // zero cotangent (the term was dropped) and the empty selection: exact zeros, also next to NaN pixels
    if (v == 0.f || !(n > 0.f) || !sel) {
        v_pred[p] = 0.f;
        return;
    }
    const float q = pred[p], e = q - g, a = fabsf(e);
    const float w = v / n;                   // mean's backward: v / numel of the selection
    float r;
    if (kind == MTGS_DEPTH_LOSS_MSE) {
        r = w * (2.f * e);
    } else if (kind == MTGS_DEPTH_LOSS_L1) {
        r = w * sgn0(e);
    } else if (kind == MTGS_DEPTH_LOSS_INVERSE_L1) {
        const float iq = 1.f / (q + 1e-6f), ig = 1.f / (g + 1e-6f);
        r = -(w * sgn0(iq - ig)) * (iq * iq);
    } else if (kind == MTGS_DEPTH_LOSS_LOG_L1) {
        r = w / (1.f + a) * sgn0(e);
    } else if (kind == MTGS_DEPTH_LOSS_HUBER_L1) {
        const float d = rec[R_D];
        r = a < d ? w * (e / d) : w * sgn0(e);
        if (a == rec[R_MAX]) r += (v * rec[R_DLDD]) * thresh / rec[R_TIES] * sgn0(e);
    } else {                                 // EdgeAwareLogL1: each half has its own count; an empty half sends nothing
        const int u = (int)(p % W), row = (int)(p / W);
        float c = 0.f;
        if (u + 1 < W) c += v / rec[R_NX] * edge_weight(rgb, p, p + 1);
        if (row + 1 < H) c += v / rec[R_NY] * edge_weight(rgb, p, p + W);
        r = c / (1.f + a) * sgn0(e);
    }
    v_pred[p] = r;
}

inline int64_t fwd_blocks(int64_t P) {
    const int64_t nb = ceil_div64(P, DL_BLOCK);
    return nb < DL_MAX_BLOCKS ? nb : DL_MAX_BLOCKS;
}

int check_args(const char *fn, int kind, int width, int height, const float *pred, const float *gt, const float *rgb, float lo, float hi,
               float thresh) {
    MTGS_REQUIRE(kind >= MTGS_DEPTH_LOSS_MSE && kind <= MTGS_DEPTH_LOSS_EDGE_AWARE_LOG_L1, MTGS_EINVAL,
                 "%s: kind must be one of MTGS_DEPTH_LOSS_* (got %d)", fn, kind);
    MTGS_REQUIRE(width > 0, MTGS_EINVAL, "%s: width must be >= 1 (got %d)", fn, width);
    MTGS_REQUIRE(height > 0, MTGS_EINVAL, "%s: height must be >= 1 (got %d)", fn, height);
    MTGS_REQUIRE(pred, MTGS_EINVAL, "%s: pred is NULL", fn);
    MTGS_REQUIRE(gt, MTGS_EINVAL, "%s: gt is NULL", fn);
    MTGS_REQUIRE(kind != MTGS_DEPTH_LOSS_EDGE_AWARE_LOG_L1 || rgb, MTGS_EINVAL, "%s: rgb is NULL (EdgeAwareLogL1 reads it)", fn);
    MTGS_REQUIRE(lo == lo && hi == hi, MTGS_EINVAL, "%s: lo and hi must not be NaN", fn);
    MTGS_REQUIRE(kind != MTGS_DEPTH_LOSS_HUBER_L1 || (__builtin_isfinite(thresh) && thresh > 0.f), MTGS_EINVAL,
                 "%s: huber_thresh must be finite and > 0", fn);
    return MTGS_OK;
}
}  // namespace

extern "C" int mtgs_depth_loss_workspace_floats(int width, int height, size_t *n) {
    MTGS_REQUIRE(width > 0 && height > 0, MTGS_EINVAL, "mtgs_depth_loss_workspace_floats: width and height must be >= 1");
    MTGS_REQUIRE(n, MTGS_EINVAL, "mtgs_depth_loss_workspace_floats: n is NULL");
    *n = (size_t)fwd_blocks((int64_t)width * height) * DL_PARTS;
    return MTGS_OK;
}

extern "C" int mtgs_depth_loss_fwd(int kind, int width, int height, const float *pred, const float *gt, const uint8_t *mask,
                                   const float *rgb, float lo, float hi, float huber_thresh, float *partials, float *out,
                                   void *stream) {
    const int rc = check_args("mtgs_depth_loss_fwd", kind, width, height, pred, gt, rgb, lo, hi, huber_thresh);
    if (rc != MTGS_OK) return rc;
    MTGS_REQUIRE(partials, MTGS_EINVAL, "mtgs_depth_loss_fwd: partials is NULL");
    MTGS_REQUIRE(out, MTGS_EINVAL, "mtgs_depth_loss_fwd: out is NULL");
    const int64_t P = (int64_t)width * height;
    const int64_t nb = fwd_blocks(P);
    const unsigned grid = (unsigned)nb;
    hipStream_t st = (hipStream_t)stream;
    switch (kind) {
    case MTGS_DEPTH_LOSS_MSE:
        depth_mean_fwd_kernel<MTGS_DEPTH_LOSS_MSE><<<grid, DL_BLOCK, 0, st>>>(P, pred, gt, mask, lo, hi, partials);
        break;
    case MTGS_DEPTH_LOSS_L1:
        depth_mean_fwd_kernel<MTGS_DEPTH_LOSS_L1><<<grid, DL_BLOCK, 0, st>>>(P, pred, gt, mask, lo, hi, partials);
        break;
    case MTGS_DEPTH_LOSS_INVERSE_L1:
        depth_mean_fwd_kernel<MTGS_DEPTH_LOSS_INVERSE_L1><<<grid, DL_BLOCK, 0, st>>>(P, pred, gt, mask, lo, hi, partials);
        break;
    case MTGS_DEPTH_LOSS_LOG_L1:
        depth_mean_fwd_kernel<MTGS_DEPTH_LOSS_LOG_L1><<<grid, DL_BLOCK, 0, st>>>(P, pred, gt, mask, lo, hi, partials);
        break;
    case MTGS_DEPTH_LOSS_HUBER_L1:
        depth_huber_max_kernel<<<grid, DL_BLOCK, 0, st>>>(P, pred, gt, mask, lo, hi, partials);
        depth_huber_max_finish_kernel<<<1, DL_BLOCK, 0, st>>>(nb, huber_thresh, partials, out);
        depth_huber_sum_kernel<<<grid, DL_BLOCK, 0, st>>>(P, pred, gt, mask, lo, hi, out, partials);
        break;
    default:
        depth_edge_fwd_kernel<<<grid, DL_BLOCK, 0, st>>>(width, height, pred, gt, mask, rgb, lo, hi, partials);
        break;
    }
    depth_loss_finish_kernel<<<1, DL_BLOCK, 0, st>>>(kind, nb, partials, out);
    MTGS_CHECK_LAUNCH("mtgs_depth_loss_fwd");
    return MTGS_OK;
}

extern "C" int mtgs_depth_loss_bwd(int kind, int width, int height, const float *pred, const float *gt, const uint8_t *mask,
                                   const float *rgb, float lo, float hi, float huber_thresh, const float *v_out, const float *out,
                                   float *v_pred, void *stream) {
    const int rc = check_args("mtgs_depth_loss_bwd", kind, width, height, pred, gt, rgb, lo, hi, huber_thresh);
    if (rc != MTGS_OK) return rc;
    MTGS_REQUIRE(v_out, MTGS_EINVAL, "mtgs_depth_loss_bwd: v_out is NULL");
    MTGS_REQUIRE(out, MTGS_EINVAL, "mtgs_depth_loss_bwd: out is NULL");
    MTGS_REQUIRE(v_pred, MTGS_EINVAL, "mtgs_depth_loss_bwd: v_pred is NULL");
    const int64_t nb = ceil_div64((int64_t)width * height, DL_BLOCK);
    depth_loss_bwd_kernel<<<(unsigned)nb, DL_BLOCK, 0, (hipStream_t)stream>>>(kind, width, height, pred, gt, mask, rgb, lo, hi,
                                                                              huber_thresh, v_out, out, v_pred);
    MTGS_CHECK_LAUNCH("mtgs_depth_loss_bwd");
    return MTGS_OK;
}
