// geomloss.hip -- the geometric terms of get_loss_dict that the shipped configs switch on (config/MTGS.py:111-118:
// use_normal_loss, normal_supervision = 'depth', use_normal_tv_loss, two_d_gaussians, sharp_shape_reg_lambda = 1.0).
//
// 1. The target normal image of the depth-supervised normal loss (mtgs_scene_graph.py:905-935; eval image :1103-1121):
//        P(v,u)  = ((u + 0.5 - cx) d / fx, (v + 0.5 - cy) d / fy, d) @ inv(eye(3))     get_means3d_backproj, c2w = eye(4)
//        n       = normalize(cross(P[v,u+1] - P[v,u-1], P[v-1,u] - P[v+1,u]))         pcd_to_normal, one-pixel zero border
//        target  = (1 + n @ diag(1,-1,-1)) / 2                                        (geometric_loss.py:350-388)
//    PyTorch: six .item() host reads of the camera, a matrix inverse and ~25 small kernels.  Here the intrinsics are read from
//    the device K [3,3] by the kernel, and the loss kernels recompute the target per pixel from the depth neighbourhood (four
//    depth reads that neighbouring threads share through the caches) instead of storing it.
// 2. The loss |target - pred|[m].mean() + TVLoss(pred), m = (depth > lo) & (depth < hi) & mask: one pass forward (four
//    per-block partial sums, then a fixed-order fp64 finish), one pass backward.
// 3. The scale regularisers on the collected scales [N,3] (:937-940, :969-981): min(s).mean() and
//    mean(max(s_a / s_b, r) - r), (s_a, s_b) = (two largest) with two_d_gaussians, (max, min) without: one pass each way.
//
// The matrix products with the identity / diag(1,-1,-1) are restated with their zero terms: x*1 + y*0 + z*0 is NaN when y or
// z is not finite, so a non-finite component spreads to the others as it does in the reference.  Compiled with
// -ffp-contract=off (build.py) so every expression rounds as the reference's per-operation kernels do.
// No float atomics: every reduction is in a fixed order, so results are bitwise reproducible; nothing is read back to the
// host and nothing is allocated here, so every entry point can be captured in a HIP graph.
#include "common.hpp"
#include "block_reduce.hpp"

namespace {
constexpr int GL_BLOCK = 256;
constexpr int NL_PARTS = 4;      // normal loss partials per block: L1 sum, count, TV (left/right) sum, TV (up/down) sum
constexpr int SR_PARTS = 2;      // scale regulariser partials per block: 2D sum, sharp sum

struct Intr { float fx, fy, cx, cy; };

__device__ __forceinline__ Intr load_intr(const float *__restrict__ K) { return {K[0], K[4], K[2], K[5]}; }

// get_means3d_backproj for one pixel, then `@ inv(eye(3)) + 0` (the zero products carry a non-finite component's NaN over)
__device__ __forceinline__ float3 backproject(int u, int v, float d, const Intr &k) {
    const float x = ((float)u + 0.5f - k.cx) * d / k.fx;
    const float y = ((float)v + 0.5f - k.cy) * d / k.fy;
    const float z = d;
    const float zx = x * 0.f, zy = y * 0.f, zz = z * 0.f;
    return make_float3(x + zy + zz, zx + y + zz, zx + zy + z);
}

// The target normal of pixel (u, v), after the flip and (1 + n) / 2.  Border pixels: 0.5.
__device__ __forceinline__ float3 target_normal(int W, int H, int u, int v, const float *__restrict__ depth, const Intr &k) {
    if (u == 0 || v == 0 || u == W - 1 || v == H - 1) return make_float3(0.5f, 0.5f, 0.5f);
    const int64_t p = (int64_t)v * W + u;
    const float3 l = backproject(u - 1, v, depth[p - 1], k), r = backproject(u + 1, v, depth[p + 1], k);
    const float3 t = backproject(u, v - 1, depth[p - W], k), b = backproject(u, v + 1, depth[p + W], k);
    const float a0 = r.x - l.x, a1 = r.y - l.y, a2 = r.z - l.z;          // left_to_right
    const float c0 = t.x - b.x, c1 = t.y - b.y, c2 = t.z - b.z;          // bottom_to_top
    float n0 = a1 * c2 - a2 * c1, n1 = a2 * c0 - a0 * c2, n2 = a0 * c1 - a1 * c0;
    const float nrm = fmaxf(sqrtf(n0 * n0 + n1 * n1 + n2 * n2), 1e-12f);   // F.normalize: clamp_min(eps) (a NaN norm stays NaN)
    n0 = n0 / nrm; n1 = n1 / nrm; n2 = n2 / nrm;
    const float z0 = n0 * 0.f, z1 = n1 * 0.f, z2 = n2 * 0.f;               // @ diag(1, -1, -1)
    const float f0 = n0 + z1 + z2, f1 = z0 - n1 + z2, f2 = z0 + z1 - n2;
    return make_float3((1.f + f0) / 2.f, (1.f + f1) / 2.f, (1.f + f2) / 2.f);
}

__device__ __forceinline__ bool selected(float d, int64_t p, const uint8_t *__restrict__ mask, float lo, float hi) {
    return d > lo && d < hi && (mask == nullptr || mask[p] != 0);
}

__global__ __launch_bounds__(GL_BLOCK) void depth_normals_kernel(int W, int H, const float *__restrict__ depth,
                                                                 const float *__restrict__ K, float *__restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * GL_BLOCK + threadIdx.x;
    if (p >= (int64_t)W * H) return;
    const Intr k = load_intr(K);
    const float3 n = target_normal(W, H, (int)(p % W), (int)(p / W), depth, k);
    out[p * 3] = n.x; out[p * 3 + 1] = n.y; out[p * 3 + 2] = n.z;
}

__global__ __launch_bounds__(GL_BLOCK) void normal_loss_fwd_kernel(int W, int H, const float *__restrict__ pred,
                                                                   const float *__restrict__ depth, const float *__restrict__ K,
                                                                   const uint8_t *__restrict__ mask, float lo, float hi, int tv,
                                                                   float *__restrict__ partials) {
    __shared__ float s_red[4];
    const int64_t p = (int64_t)blockIdx.x * GL_BLOCK + threadIdx.x;
    float l1 = 0.f, cnt = 0.f, ta = 0.f, tb = 0.f;
    if (p < (int64_t)W * H) {
        const int u = (int)(p % W), v = (int)(p / W);
        const float q0 = pred[p * 3], q1 = pred[p * 3 + 1], q2 = pred[p * 3 + 2];
        if (selected(depth[p], p, mask, lo, hi)) {
            const float3 g = target_normal(W, H, u, v, depth, load_intr(K));
            l1 = (fabsf(g.x - q0) + fabsf(g.y - q1)) + fabsf(g.z - q2);
            cnt = 1.f;
        }
        if (tv) {
            if (u + 1 < W) ta = (fabsf(q0 - pred[p * 3 + 3]) + fabsf(q1 - pred[p * 3 + 4])) + fabsf(q2 - pred[p * 3 + 5]);
            if (v + 1 < H) {
                const int64_t e = (p + W) * 3;
                tb = (fabsf(q0 - pred[e]) + fabsf(q1 - pred[e + 1])) + fabsf(q2 - pred[e + 2]);
            }
        }
    }
    l1 = block_sum4(l1, s_red);
    cnt = block_sum4(cnt, s_red);
    ta = block_sum4(ta, s_red);
    tb = block_sum4(tb, s_red);
    if (threadIdx.x == 0) {
        float *o = partials + (int64_t)blockIdx.x * NL_PARTS;
        o[0] = l1; o[1] = cnt; o[2] = ta; o[3] = tb;
    }
}

// out = {loss, count, L1 part, TV part}.  mean over an empty selection is NaN, as in torch.
__global__ __launch_bounds__(GL_BLOCK) void normal_loss_finish_kernel(int64_t nblocks, double na, double nb, int tv,
                                                                      const float *__restrict__ partials, float *__restrict__ out) {
    double s[NL_PARTS];
    finish_sums<NL_PARTS, GL_BLOCK>(nblocks, partials, s);
    if (threadIdx.x != 0) return;
    const float l1 = s[1] > 0.0 ? (float)(s[0] / (3.0 * s[1])) : __builtin_nanf("");
    float t = 0.f;
    if (tv) {
        const float a = na > 0.0 ? (float)(s[2] / na) : __builtin_nanf("");
        const float b = nb > 0.0 ? (float)(s[3] / nb) : __builtin_nanf("");
        t = a + b;
    }
    out[0] = l1 + t;
    out[1] = (float)s[1];
    out[2] = l1;
    out[3] = t;
}

__global__ __launch_bounds__(GL_BLOCK) void normal_loss_bwd_kernel(int W, int H, const float *__restrict__ pred,
                                                                   const float *__restrict__ depth, const float *__restrict__ K,
                                                                   const uint8_t *__restrict__ mask, float lo, float hi, int tv,
                                                                   float inv_a, float inv_b, const float *__restrict__ v_out,
                                                                   const float *__restrict__ out, float *__restrict__ v_pred) {
    const int64_t p = (int64_t)blockIdx.x * GL_BLOCK + threadIdx.x;
    if (p >= (int64_t)W * H) return;
    const float v = v_out[0];
    if (v == 0.f) {      // zero cotangent (the term was dropped): exact zeros, also next to NaN pixels
        v_pred[p * 3] = 0.f; v_pred[p * 3 + 1] = 0.f; v_pred[p * 3 + 2] = 0.f;
        return;
    }
    const int u = (int)(p % W), r = (int)(p / W);
    const float q[3] = {pred[p * 3], pred[p * 3 + 1], pred[p * 3 + 2]};
    float g[3] = {0.f, 0.f, 0.f};
    if (selected(depth[p], p, mask, lo, hi)) {
        const float3 t = target_normal(W, H, u, r, depth, load_intr(K));
        const float w = v / (3.f * out[1]);          // mean's backward: v / numel of the selection
        g[0] = w * sgn0(q[0] - t.x); g[1] = w * sgn0(q[1] - t.y); g[2] = w * sgn0(q[2] - t.z);
    }
    if (tv) {
        const float va = v * inv_a, vb = v * inv_b;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float ga = 0.f, gb = 0.f;
            if (u + 1 < W) ga += sgn0(q[c] - pred[p * 3 + 3 + c]);
            if (u > 0) ga -= sgn0(pred[p * 3 - 3 + c] - q[c]);
            if (r + 1 < H) gb += sgn0(q[c] - pred[(p + W) * 3 + c]);
            if (r > 0) gb -= sgn0(pred[(p - W) * 3 + c] - q[c]);
            if (W > 1) g[c] += va * ga;              // (an empty difference image: no gradient, as torch's empty mean)
            if (H > 1) g[c] += vb * gb;
        }
    }
    v_pred[p * 3] = g[0]; v_pred[p * 3 + 1] = g[1]; v_pred[p * 3 + 2] = g[2];
}

// ---- scale regularisers ----
struct RowPick {
    int imin;          // torch.min(dim=1): lowest index on ties
    int ia, ib;        // the numerator / denominator of the sharp ratio (see mtgs_rast.h for the tie rules)
    float ratio;
    bool nan;          // a NaN in the row: both terms are NaN (min, sort, amax and amin all propagate it)
};

__device__ __forceinline__ RowPick pick(const float s[3], int two_d) {
    RowPick r;
    r.nan = s[0] != s[0] || s[1] != s[1] || s[2] != s[2];
    int lo = 0, hi = 0;
    for (int i = 1; i < 3; ++i) {
        if (s[i] < s[lo]) lo = i;
        if (s[i] > s[hi]) hi = i;
    }
    r.imin = lo;
    if (two_d) {
        int b = hi == 0 ? 1 : 0;                     // the largest of the other two, lowest index on ties
        for (int i = b + 1; i < 3; ++i)
            if (i != hi && s[i] > s[b]) b = i;
        r.ia = hi; r.ib = b;
    } else {
        r.ia = hi; r.ib = lo;
    }
    r.ratio = s[r.ia] / s[r.ib];
    return r;
}

__global__ __launch_bounds__(GL_BLOCK) void scale_reg_fwd_kernel(int64_t n, const float *__restrict__ scales, int two_d, float max_ratio,
                                                                 float *__restrict__ partials) {
    __shared__ float s_red[4];
    const int64_t i = (int64_t)blockIdx.x * GL_BLOCK + threadIdx.x;
    float a = 0.f, b = 0.f;
    if (i < n) {
        const float s[3] = {scales[i * 3], scales[i * 3 + 1], scales[i * 3 + 2]};
        const RowPick r = pick(s, two_d);
        if (r.nan) {
            a = b = __builtin_nanf("");
        } else {
            a = s[r.imin];
            b = (r.ratio > max_ratio ? r.ratio : max_ratio) - max_ratio;
        }
    }
    a = block_sum4(a, s_red);
    b = block_sum4(b, s_red);
    if (threadIdx.x == 0) { partials[(int64_t)blockIdx.x * SR_PARTS] = a; partials[(int64_t)blockIdx.x * SR_PARTS + 1] = b; }
}

__global__ __launch_bounds__(GL_BLOCK) void scale_reg_finish_kernel(int64_t nblocks, int64_t n, const float *__restrict__ partials,
                                                                    float *__restrict__ out) {
    double s[SR_PARTS];
    finish_sums<SR_PARTS, GL_BLOCK>(nblocks, partials, s);
    if (threadIdx.x != 0) return;
    out[0] = n > 0 ? (float)(s[0] / (double)n) : __builtin_nanf("");
    out[1] = n > 0 ? (float)(s[1] / (double)n) : __builtin_nanf("");
}

__global__ __launch_bounds__(GL_BLOCK) void scale_reg_bwd_kernel(int64_t n, const float *__restrict__ scales, int two_d, float max_ratio,
                                                                 const float *__restrict__ v_out, float *__restrict__ v_scales) {
    const int64_t i = (int64_t)blockIdx.x * GL_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float v0 = v_out[0], v1 = v_out[1];
    const float s[3] = {scales[i * 3], scales[i * 3 + 1], scales[i * 3 + 2]};
    float g[3] = {0.f, 0.f, 0.f};
    const RowPick r = pick(s, two_d);
    if (v0 != 0.f) g[r.imin] += v0 / (float)n;
    if (v1 != 0.f) {
        // torch.maximum: the whole gradient above max_ratio, half of it at equality, none below (NaN: the whole gradient)
        const float f = r.ratio < max_ratio ? 0.f : (r.ratio == max_ratio ? 0.5f : 1.f);
        const float gr = (v1 / (float)n) * f;
        const float sa = s[r.ia], sb = s[r.ib];
        const float da = gr / sb, db = -gr * sa / (sb * sb);      // div's backward: grad / b, -grad * a / (b * b)
        if (two_d) {
            g[r.ia] += da;
            g[r.ib] += db;
        } else {       // amax / amin: split evenly among the tied entries
            int cmax = 0, cmin = 0;
            for (int j = 0; j < 3; ++j) { cmax += s[j] == sa; cmin += s[j] == sb; }
            for (int j = 0; j < 3; ++j) {
                if (s[j] == sa) g[j] += da / (float)cmax;
                if (s[j] == sb) g[j] += db / (float)cmin;
            }
        }
    }
    v_scales[i * 3] = g[0]; v_scales[i * 3 + 1] = g[1]; v_scales[i * 3 + 2] = g[2];
}

inline int64_t nblocks_of(int64_t n) { return ceil_div64(n, GL_BLOCK); }

// TV element counts of an [H, W, 3] image: H (W - 1) 3 and (H - 1) W 3
inline void tv_counts(int W, int H, double &na, double &nb) {
    na = (double)H * (W - 1) * 3;
    nb = (double)(H - 1) * W * 3;
}
}  // namespace

extern "C" int mtgs_depth_normals(int width, int height, const float *depth, const float *K, float *out, void *stream) {
    MTGS_REQUIRE(width > 0, MTGS_EINVAL, "mtgs_depth_normals: width must be >= 1 (got %d)", width);
    MTGS_REQUIRE(height > 0, MTGS_EINVAL, "mtgs_depth_normals: height must be >= 1 (got %d)", height);
    MTGS_REQUIRE(depth, MTGS_EINVAL, "mtgs_depth_normals: depth is NULL");
    MTGS_REQUIRE(K, MTGS_EINVAL, "mtgs_depth_normals: K is NULL");
    MTGS_REQUIRE(out, MTGS_EINVAL, "mtgs_depth_normals: out is NULL");
    const int64_t P = (int64_t)width * height;
    depth_normals_kernel<<<(unsigned)nblocks_of(P), GL_BLOCK, 0, (hipStream_t)stream>>>(width, height, depth, K, out);
    MTGS_CHECK_LAUNCH("mtgs_depth_normals");
    return MTGS_OK;
}

extern "C" int mtgs_depth_normal_loss_workspace_floats(int width, int height, size_t *n) {
    MTGS_REQUIRE(width > 0 && height > 0, MTGS_EINVAL, "mtgs_depth_normal_loss_workspace_floats: width and height must be >= 1");
    MTGS_REQUIRE(n, MTGS_EINVAL, "mtgs_depth_normal_loss_workspace_floats: n is NULL");
    *n = (size_t)nblocks_of((int64_t)width * height) * NL_PARTS;
    return MTGS_OK;
}

static int check_normal_loss_args(const char *fn, int width, int height, const float *pred, const float *depth, const float *K) {
    MTGS_REQUIRE(width > 0, MTGS_EINVAL, "%s: width must be >= 1 (got %d)", fn, width);
    MTGS_REQUIRE(height > 0, MTGS_EINVAL, "%s: height must be >= 1 (got %d)", fn, height);
    MTGS_REQUIRE(pred, MTGS_EINVAL, "%s: pred is NULL", fn);
    MTGS_REQUIRE(depth, MTGS_EINVAL, "%s: depth is NULL", fn);
    MTGS_REQUIRE(K, MTGS_EINVAL, "%s: K is NULL", fn);
    return MTGS_OK;
}

extern "C" int mtgs_depth_normal_loss_fwd(int width, int height, const float *pred, const float *depth, const float *K,
                                          const uint8_t *mask, float lo, float hi, int tv, float *partials, float *out, void *stream) {
    const int rc = check_normal_loss_args("mtgs_depth_normal_loss_fwd", width, height, pred, depth, K);
    if (rc != MTGS_OK) return rc;
    MTGS_REQUIRE(partials, MTGS_EINVAL, "mtgs_depth_normal_loss_fwd: partials is NULL");
    MTGS_REQUIRE(out, MTGS_EINVAL, "mtgs_depth_normal_loss_fwd: out is NULL");
    const int64_t nb = nblocks_of((int64_t)width * height);
    double na_, nb_;
    tv_counts(width, height, na_, nb_);
    hipStream_t st = (hipStream_t)stream;
    normal_loss_fwd_kernel<<<(unsigned)nb, GL_BLOCK, 0, st>>>(width, height, pred, depth, K, mask, lo, hi, tv != 0, partials);
    normal_loss_finish_kernel<<<1, GL_BLOCK, 0, st>>>(nb, na_, nb_, tv != 0, partials, out);
    MTGS_CHECK_LAUNCH("mtgs_depth_normal_loss_fwd");
    return MTGS_OK;
}

extern "C" int mtgs_depth_normal_loss_bwd(int width, int height, const float *pred, const float *depth, const float *K,
                                          const uint8_t *mask, float lo, float hi, int tv, const float *v_out, const float *out,
                                          float *v_pred, void *stream) {
    const int rc = check_normal_loss_args("mtgs_depth_normal_loss_bwd", width, height, pred, depth, K);
    if (rc != MTGS_OK) return rc;
    MTGS_REQUIRE(v_out, MTGS_EINVAL, "mtgs_depth_normal_loss_bwd: v_out is NULL");
    MTGS_REQUIRE(out, MTGS_EINVAL, "mtgs_depth_normal_loss_bwd: out is NULL");
    MTGS_REQUIRE(v_pred, MTGS_EINVAL, "mtgs_depth_normal_loss_bwd: v_pred is NULL");
    double na_, nb_;
    tv_counts(width, height, na_, nb_);
    const float inv_a = na_ > 0 ? (float)(1.0 / na_) : 0.f, inv_b = nb_ > 0 ? (float)(1.0 / nb_) : 0.f;
    normal_loss_bwd_kernel<<<(unsigned)nblocks_of((int64_t)width * height), GL_BLOCK, 0, (hipStream_t)stream>>>(
        width, height, pred, depth, K, mask, lo, hi, tv != 0, inv_a, inv_b, v_out, out, v_pred);
    MTGS_CHECK_LAUNCH("mtgs_depth_normal_loss_bwd");
    return MTGS_OK;
}

extern "C" int mtgs_scale_reg_workspace_floats(int64_t n, size_t *nf) {
    MTGS_REQUIRE(n >= 0, MTGS_EINVAL, "mtgs_scale_reg_workspace_floats: n must be >= 0");
    MTGS_REQUIRE(nf, MTGS_EINVAL, "mtgs_scale_reg_workspace_floats: nf is NULL");
    *nf = (size_t)(nblocks_of(n) > 0 ? nblocks_of(n) : 1) * SR_PARTS;
    return MTGS_OK;
}

extern "C" int mtgs_scale_reg_fwd(int64_t n, const float *scales, int two_d, float max_ratio, float *partials, float *out,
                                  void *stream) {
    MTGS_REQUIRE(n >= 0, MTGS_EINVAL, "mtgs_scale_reg_fwd: n must be >= 0");
    MTGS_REQUIRE(n == 0 || scales, MTGS_EINVAL, "mtgs_scale_reg_fwd: scales is NULL");
    MTGS_REQUIRE(__builtin_isfinite(max_ratio), MTGS_EINVAL, "mtgs_scale_reg_fwd: max_ratio must be finite");
    MTGS_REQUIRE(partials, MTGS_EINVAL, "mtgs_scale_reg_fwd: partials is NULL");
    MTGS_REQUIRE(out, MTGS_EINVAL, "mtgs_scale_reg_fwd: out is NULL");
    const int64_t nb = nblocks_of(n);
    hipStream_t st = (hipStream_t)stream;
    if (nb > 0) scale_reg_fwd_kernel<<<(unsigned)nb, GL_BLOCK, 0, st>>>(n, scales, two_d != 0, max_ratio, partials);
    scale_reg_finish_kernel<<<1, GL_BLOCK, 0, st>>>(nb, n, partials, out);
    MTGS_CHECK_LAUNCH("mtgs_scale_reg_fwd");
    return MTGS_OK;
}

extern "C" int mtgs_scale_reg_bwd(int64_t n, const float *scales, int two_d, float max_ratio, const float *v_out, float *v_scales,
                                  void *stream) {
    MTGS_REQUIRE(n >= 0, MTGS_EINVAL, "mtgs_scale_reg_bwd: n must be >= 0");
    MTGS_REQUIRE(__builtin_isfinite(max_ratio), MTGS_EINVAL, "mtgs_scale_reg_bwd: max_ratio must be finite");
    if (n == 0) return MTGS_OK;
    MTGS_REQUIRE(scales, MTGS_EINVAL, "mtgs_scale_reg_bwd: scales is NULL");
    MTGS_REQUIRE(v_out, MTGS_EINVAL, "mtgs_scale_reg_bwd: v_out is NULL");
    MTGS_REQUIRE(v_scales, MTGS_EINVAL, "mtgs_scale_reg_bwd: v_scales is NULL");
    scale_reg_bwd_kernel<<<(unsigned)nblocks_of(n), GL_BLOCK, 0, (hipStream_t)stream>>>(n, scales, two_d != 0, max_ratio, v_out,
                                                                                         v_scales);
    MTGS_CHECK_LAUNCH("mtgs_scale_reg_bwd");
    return MTGS_OK;
}
