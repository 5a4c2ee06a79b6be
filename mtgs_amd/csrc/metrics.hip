// metrics.hip -- MTGS's per-step image metrics on the device: colour-corrected PSNR, PSNR and the lidar depth errors
// (mtgs/scene_model/mtgs_scene_graph.py get_metrics_dict, mtgs/utils/pnsr.py color_correct / MaskedPSNR).
//
// color_correct fits, per channel, a quadratic colour warp a(x) . w_c -> ref_c by least squares over the rows that are unclipped
// in the input, in the current estimate and in ref, num_iters times, and applies x <- clip(a(x) W, 0, 1) after every fit.
// One call is
//     for k < num_iters:  cc_accum (x_k = the input warped by W_0..W_{k-1}; per-workgroup fp64 Gram [A b]^T diag(m_c) [A b])
//                         metrics_reduce (fixed-order sum of the partials)    cc_solve (fp64 Cholesky of the 3 systems -> W_k)
//     cc_final (x_n; writes it and/or accumulates the PSNR and depth sums)     metrics_reduce + metrics_finish (image_metrics)
// x_k is recomputed from the input in every pass (k warps of 30 fp64 FMAs per pixel) instead of being stored: a pass reads the
// image, ref and mask (25 B per pixel) and writes nothing per pixel but the final output.  No float atomics and no host reads:
// the result is bitwise reproducible and the call can be captured in a graph.  DESIGN.md section 9.
#include "common.hpp"
#include "block_reduce.hpp"

namespace {

constexpr int NF = 10;                  // features a = [x0^2, x0x1, x0x2, x1^2, x1x2, x2^2, x0, x1, x2, 1]
constexpr int NG = NF * (NF + 1) / 2;   // upper triangle of A^T diag(m) A
constexpr int NE = NG + NF;             // + A^T diag(m) b: entries per channel
constexpr int NCE = 3 * NE;             // entries per workgroup partial of a fit
constexpr int NS = 7;                   // sums of the final pass
constexpr int AB = 192;                 // accumulation workgroup: 3 waves, wave c accumulates channel c
constexpr int MAX_GRID = 1024;
constexpr int RB = 256;                 // reduction workgroup
// A fit fails when a Cholesky pivot is not above PIVOT_TOL times its diagonal entry (column j of the masked A lies within
// 1e-6 rad of the span of columns 0..j-1, or is empty), or when the Gram or the solution is not finite.
constexpr double PIVOT_TOL = 1e-12;

// position of Gram entry (i, j), i <= j, in the row-major upper triangle that cc_accum_kernel writes
__host__ __device__ constexpr int gram_index(int i, int j) { return i * NF - i * (i - 1) / 2 + (j - i); }

__host__ __device__ inline int grid_of(int64_t P) {
    const int64_t g = ceil_div64(P, 2 * AB);
    return (int)(g < 1 ? 1 : (g > MAX_GRID ? MAX_GRID : g));
}

struct Thr {
    float lo, hi;                       // unclipped(z) = z >= lo && z <= hi (eps and 1 - eps rounded to f32, as torch compares)
};

__device__ inline bool unclipped(float z, Thr t) { return z >= t.lo && z <= t.hi; }

__device__ inline void features(const float x[3], double f[NF]) {
    const double a = x[0], b = x[1], c = x[2];
    f[0] = a * a; f[1] = a * b; f[2] = a * c; f[3] = b * b; f[4] = b * c; f[5] = c * c;
    f[6] = a; f[7] = b; f[8] = c; f[9] = 1.0;
}

// x <- clip(a(x) W_k, 0, 1) for k < n (W: [n][3][NF] doubles)
__device__ inline void warp_chain(float x[3], const double *__restrict__ W, int n) {
    for (int k = 0; k < n; ++k) {
        double f[NF];
        features(x, f);
        const double *w = W + k * 3 * NF;
        for (int c = 0; c < 3; ++c) {
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < NF; ++i) s = fma(f[i], w[c * NF + i], s);
            x[c] = fminf(fmaxf((float)s, 0.f), 1.f);
        }
    }
}

// img * mask and ref * mask of pixel p (a float product as in the reference's masked call; mask NULL = all ones)
__device__ inline void load_pixel(int64_t p, const float *__restrict__ img, const float *__restrict__ ref, const uint8_t *__restrict__ mask,
                                  float x[3], float r[3], float &mf) {
    mf = (!mask || mask[p]) ? 1.f : 0.f;
    for (int c = 0; c < 3; ++c) {
        x[c] = img[p * 3 + c] * mf;
        r[c] = ref ? ref[p * 3 + c] * mf : 0.f;
    }
}

__device__ inline double wave_sum(double v) {
    for (int o = MTGS_WAVE / 2; o > 0; o >>= 1) v += __shfl_down(v, o, MTGS_WAVE);
    return v;
}

// Pass k < num_iters: the Gram of the rows of channel c that pass mask0 & unclipped(x_k) & unclipped(ref), per workgroup.
// part layout [entry][workgroup] (entry = c * NE + e), so that the reduction reads each entry's partials contiguously.
__global__ __launch_bounds__(AB) void cc_accum_kernel(int64_t P, const float *__restrict__ img, const float *__restrict__ ref,
                                                      const uint8_t *__restrict__ mask, const double *__restrict__ W, int k, Thr t,
                                                      double *__restrict__ part) {
    __shared__ float sx[3][AB];
    __shared__ float sr[3][AB];
    __shared__ uint32_t sm[AB];
    const int tid = threadIdx.x, c = tid / MTGS_WAVE, lane = tid % MTGS_WAVE;
    double acc[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) acc[e] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * AB;
    for (int64_t base = (int64_t)blockIdx.x * AB; base < P; base += stride) {
        const int64_t p = base + tid;
        float x[3] = {0.f, 0.f, 0.f}, r[3] = {0.f, 0.f, 0.f};
        uint32_t bits = 0;
        if (p < P) {
            float mf;
            load_pixel(p, img, ref, mask, x, r, mf);
            uint32_t m0 = 0;
            for (int j = 0; j < 3; ++j) m0 |= (unclipped(x[j], t) ? 1u : 0u) << j;
            warp_chain(x, W, k);
            for (int j = 0; j < 3; ++j) bits |= ((m0 >> j) & (unclipped(x[j], t) && unclipped(r[j], t) ? 1u : 0u)) << j;
        }
        __syncthreads();                 // the previous round's readers are done
        for (int j = 0; j < 3; ++j) { sx[j][tid] = x[j]; sr[j][tid] = r[j]; }
        sm[tid] = bits;
        __syncthreads();
        for (int q = lane; q < AB; q += MTGS_WAVE) {
            const float xq[3] = {sx[0][q], sx[1][q], sx[2][q]};
            const double m = (double)((sm[q] >> c) & 1u);
            const double b = (double)sr[c][q];
            double f[NF];
            features(xq, f);
            int e = 0;
#pragma unroll
            for (int i = 0; i < NF; ++i) {
                const double fm = f[i] * m;
#pragma unroll
                for (int j = i; j < NF; ++j) {
                    acc[e] = fma(fm, f[j], acc[e]);
                    ++e;
                }
            }
#pragma unroll
            for (int i = 0; i < NF; ++i) acc[NG + i] = fma(f[i] * m, b, acc[NG + i]);
        }
    }
    // Lane sums of 16 entries at a time through LDS (a shuffle tree per entry costs 6 dependent cross-lane moves for each of the
    // 65 entries): lane l adds entry l % 16 over lanes 16 (l / 16) .. 16 (l / 16) + 15, then the four quarters are added.
    __shared__ double red[3][16][MTGS_WAVE + 1];
#pragma unroll
    for (int e0 = 0; e0 < NE; e0 += 16) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (e0 + i < NE) red[c][i][lane] = acc[e0 + i];
        __syncthreads();
        const int i = lane % 16, q = lane / 16;
        double v = 0.0;
#pragma unroll
        for (int j = 0; j < 16; ++j) v += red[c][i][q * 16 + j];
        v += __shfl_down(v, 32, MTGS_WAVE);
        v += __shfl_down(v, 16, MTGS_WAVE);
        if (q == 0 && e0 + i < NE) part[(int64_t)(c * NE + e0 + i) * gridDim.x + blockIdx.x] = v;
    }
}

// total[e] = sum over workgroups b = 0..nb-1 of part[e * nb + b], in a fixed order (strided per thread, then a fixed tree).
__global__ __launch_bounds__(RB) void metrics_reduce_kernel(int nb, const double *__restrict__ part, double *__restrict__ total) {
    __shared__ double s[RB];
    const int e = blockIdx.x, tid = threadIdx.x;
    double a = 0.0;
    for (int b = tid; b < nb; b += RB) a += part[(int64_t)e * nb + b];
    const double t = block_tree_sum_f64<RB>(a, s);
    if (tid == 0) total[e] = t;
}

// Thread c < 3 solves (A^T M A) w = A^T M b of channel c by an fp64 Cholesky factorisation, writes W_k[c] and ORs a failure
// into *flag (k = 0 writes it).
__global__ __launch_bounds__(MTGS_WAVE) void cc_solve_kernel(const double *__restrict__ total, int k, double *__restrict__ W,
                                                            int *__restrict__ flag) {
    __shared__ int fails[3];
    const int c = threadIdx.x;
    if (c < 3) {
        const double *g = total + c * NE;
        double L[NF][NF], y[NF];
        bool bad = false;
#pragma unroll
        for (int j = 0; j < NF; ++j) {
            const double gjj = g[gram_index(j, j)];
            double d = gjj;
#pragma unroll
            for (int q = 0; q < j; ++q) d -= L[j][q] * L[j][q];
            if (!(d > PIVOT_TOL * gjj) || !isfinite(gjj)) {
                bad = true;
                d = 1.0;
            }
            L[j][j] = sqrt(d);
#pragma unroll
            for (int i = j + 1; i < NF; ++i) {
                double v = g[gram_index(j, i)];
#pragma unroll
                for (int q = 0; q < j; ++q) v -= L[i][q] * L[j][q];
                L[i][j] = v / L[j][j];
            }
        }
#pragma unroll
        for (int i = 0; i < NF; ++i) {           // L y = A^T M b
            double v = g[NG + i];
#pragma unroll
            for (int q = 0; q < i; ++q) v -= L[i][q] * y[q];
            y[i] = v / L[i][i];
        }
#pragma unroll
        for (int i = NF - 1; i >= 0; --i) {      // L^T w = y
            double v = y[i];
#pragma unroll
            for (int q = i + 1; q < NF; ++q) v -= L[q][i] * y[q];
            y[i] = v / L[i][i];
        }
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            bad |= !isfinite(y[i]);
            W[(k * 3 + c) * NF + i] = y[i];
        }
        fails[c] = bad ? 1 : 0;
    }
    __syncthreads();
    if (c == 0) {
        const int f = fails[0] | fails[1] | fails[2];
        *flag = k == 0 ? f : (*flag | f);
    }
}

// The last pass: x_n (or the input itself when a fit failed) to out (nullable), and with sums != NULL the per-workgroup sums
//   0 SSE(input, gt)  1 SSE(x_n, gt)  2 selected pixels  3 sum e^2  4 sum |e| / g  5 delta1 hits  6 depth pixels
// (e = g - p in f32; depth pixels: 0.1 < g < 80 and the mask), part layout [sum][workgroup].
__global__ __launch_bounds__(AB) void cc_final_kernel(int64_t P, const float *__restrict__ img, const float *__restrict__ gt,
                                                      const uint8_t *__restrict__ mask, const double *__restrict__ W, int n,
                                                      const int *__restrict__ flag, float *__restrict__ out, const float *__restrict__ pd,
                                                      const float *__restrict__ ld, double *__restrict__ part) {
    __shared__ double s[NS][AB / MTGS_WAVE];
    const int tid = threadIdx.x;
    const bool failed = n > 0 && *flag != 0;
    double acc[NS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int64_t stride = (int64_t)gridDim.x * AB;
    for (int64_t p = (int64_t)blockIdx.x * AB + tid; p < P; p += stride) {
        float x[3], r[3], mf;
        load_pixel(p, img, nullptr, mask, x, r, mf);
        const bool sel = mf != 0.f;
        if (!failed) warp_chain(x, W, n);
        if (out)
            for (int c = 0; c < 3; ++c) out[p * 3 + c] = x[c];
        if (part && sel) {
            for (int c = 0; c < 3; ++c) {
                const double d0 = (double)img[p * 3 + c] - (double)gt[p * 3 + c];
                const double d1 = (double)x[c] - (double)gt[p * 3 + c];
                acc[0] = fma(d0, d0, acc[0]);
                acc[1] = fma(d1, d1, acc[1]);
            }
            acc[2] += 1.0;
            if (pd) {
                const float gd = ld[p], pv = pd[p];
                if (gd > 0.1f && gd < 80.f) {
                    const float e = gd - pv;
                    acc[3] = fma((double)e, (double)e, acc[3]);
                    acc[4] += (double)(fabsf(e) / gd);
                    const float r1 = pv / gd, r2 = gd / pv;
                    acc[5] += (r1 < 1.25f && r2 < 1.25f) ? 1.0 : 0.0;
                    acc[6] += 1.0;
                }
            }
        }
    }
    if (!part) return;
    const int w = tid / MTGS_WAVE, lane = tid % MTGS_WAVE;
    for (int e = 0; e < NS; ++e) {
        const double v = wave_sum(acc[e]);
        if (lane == 0) s[e][w] = v;
    }
    __syncthreads();
    if (tid < NS) part[(int64_t)tid * gridDim.x + blockIdx.x] = s[tid][0] + s[tid][1] + s[tid][2];
}

// metrics[5] = psnr, cc_psnr, depth_RMSE, depth_absRel, depth_delta1 (NaN without depths; 0 / 0 = NaN for empty selections)
__global__ void metrics_finish_kernel(const double *__restrict__ t, int has_depth, float *__restrict__ metrics) {
    if (threadIdx.x != 0) return;
    const double n = 3.0 * t[2];
    metrics[0] = (float)(10.0 * log10(n / t[0]));
    metrics[1] = (float)(10.0 * log10(n / t[1]));
    const double nd = has_depth ? t[6] : nan("");
    metrics[2] = (float)sqrt(t[3] / nd);
    metrics[3] = (float)(t[4] / nd);
    metrics[4] = (float)(t[5] / nd);
}

struct Ws {
    double *part, *total, *W;
    int *flag;
};

size_t ws_bytes_of(int64_t P, int num_iters) {
    const size_t part = (size_t)grid_of(P) * NCE, total = NCE, w = (size_t)(num_iters > 0 ? num_iters : 0) * 3 * NF;
    return (part + total + w) * sizeof(double) + 16;
}

Ws ws_of(void *ws, int64_t P) {
    double *part = (double *)ws;
    double *total = part + (size_t)grid_of(P) * NCE;
    double *W = total + NCE;
    return Ws{part, total, W, nullptr};
}

int run(const char *fn, int64_t P, int num_iters, double eps, const float *img, const float *ref, const uint8_t *mask, float *out,
        const float *pd, const float *ld, float *metrics, void *ws, size_t ws_bytes, void *stream) {
    MTGS_REQUIRE(ws_bytes >= ws_bytes_of(P, num_iters), MTGS_EWORKSPACE, "%s: workspace %zu < %zu bytes", fn, ws_bytes,
                 ws_bytes_of(P, num_iters));
    hipStream_t st = (hipStream_t)stream;
    Ws w = ws_of(ws, P);
    w.flag = (int *)(w.W + (size_t)num_iters * 3 * NF);
    const Thr t{(float)eps, (float)(1.0 - eps)};
    const int nb = grid_of(P);
    for (int k = 0; k < num_iters; ++k) {
        cc_accum_kernel<<<nb, AB, 0, st>>>(P, img, ref, mask, w.W, k, t, w.part);
        MTGS_CHECK_LAUNCH(fn);
        metrics_reduce_kernel<<<NCE, RB, 0, st>>>(nb, w.part, w.total);
        MTGS_CHECK_LAUNCH(fn);
        cc_solve_kernel<<<1, MTGS_WAVE, 0, st>>>(w.total, k, w.W, w.flag);
        MTGS_CHECK_LAUNCH(fn);
    }
    cc_final_kernel<<<nb, AB, 0, st>>>(P, img, ref, mask, w.W, num_iters, w.flag, out, pd, ld, metrics ? w.part : nullptr);
    MTGS_CHECK_LAUNCH(fn);
    if (metrics) {
        metrics_reduce_kernel<<<NS, RB, 0, st>>>(nb, w.part, w.total);
        MTGS_CHECK_LAUNCH(fn);
        metrics_finish_kernel<<<1, MTGS_WAVE, 0, st>>>(w.total, pd ? 1 : 0, metrics);
        MTGS_CHECK_LAUNCH(fn);
    }
    return MTGS_OK;
}

int check_common(const char *fn, int64_t P, int num_iters, double eps) {
    MTGS_REQUIRE(P >= 0, MTGS_EINVAL, "%s: P < 0", fn);
    MTGS_REQUIRE(num_iters >= 0, MTGS_EINVAL, "%s: num_iters < 0 (%d)", fn, num_iters);
    MTGS_REQUIRE(eps >= 0.0 && eps < 0.5, MTGS_EINVAL, "%s: eps outside [0, 0.5)", fn);
    return MTGS_OK;
}

}  // namespace


extern "C" int mtgs_metrics_workspace_bytes(int64_t P, int num_iters, size_t *bytes) {
    MTGS_REQUIRE(P >= 0 && num_iters >= 0 && bytes, MTGS_EINVAL,
                 "mtgs_metrics_workspace_bytes: P < 0, num_iters < 0 or null pointer: bytes");
    *bytes = ws_bytes_of(P, num_iters);
    return MTGS_OK;
}

extern "C" int mtgs_color_correct(int64_t P, int num_iters, double eps, const float *img, const float *ref, const uint8_t *mask,
                                  float *out, void *ws, size_t ws_bytes, void *stream) {
    const char *fn = "mtgs_color_correct";
    if (int rc = check_common(fn, P, num_iters, eps)) return rc;
    if (P == 0) return MTGS_OK;
    MTGS_NONNULL(fn, img); MTGS_NONNULL(fn, ref); MTGS_NONNULL(fn, out); MTGS_NONNULL(fn, ws);
    return run(fn, P, num_iters, eps, img, ref, mask, out, nullptr, nullptr, nullptr, ws, ws_bytes, stream);
}

extern "C" int mtgs_image_metrics(int64_t P, int num_iters, double eps, const float *pred, const float *gt, const uint8_t *mask,
                                  const float *pred_depth, const float *lidar_depth, float *metrics, void *ws, size_t ws_bytes,
                                  void *stream) {
    const char *fn = "mtgs_image_metrics";
    if (int rc = check_common(fn, P, num_iters, eps)) return rc;
    MTGS_REQUIRE(!pred_depth == !lidar_depth, MTGS_EINVAL, "%s: pred_depth and lidar_depth must be given together", fn);
    if (P == 0) return MTGS_OK;
    MTGS_NONNULL(fn, pred); MTGS_NONNULL(fn, gt); MTGS_NONNULL(fn, metrics); MTGS_NONNULL(fn, ws);
    return run(fn, P, num_iters, eps, pred, gt, mask, nullptr, pred_depth, lidar_depth, metrics, ws, ws_bytes, stream);
}
