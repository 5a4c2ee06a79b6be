// seed.hip -- building a Gaussian node from a point cloud on the device (VanillaGaussianSplattingModel.populate_modules,
// mtgs/scene_model/gaussian_model/vanilla_gaussian_splatting.py:114-196): the exact k nearest neighbours of every point
// (k_nearest_sklearn, :372-390) and one fused per-point kernel for scales, rotations, colours and opacities.
//
// mtgs_knn, one call =
//   sort_front (cloud_grid.hpp) bounding box and grid, Morton codes, one stable sort, the sorted points as float4
//   knn_kernel<K>               one thread per query, in Morton order
// A cell of side 2^L finest cells is ONE contiguous range of the sorted array (all codes with the same top 63 - 3L bits), found
// by a binary search on the code prefix.  A query visits the 3x3x3 block of level-L cells around its own, keeps the K
// smallest (d2, index) in registers and accepts when the K-th d2 is STRICTLY below the squared distance to the nearest
// face of the block that has cells behind it; otherwise it goes up one level (the block of level 21 is the whole cloud).
// The first level is chosen per query from the sorted order: the smallest cell that holds the query and the K entries
// before or behind it, minus one.
//
// Exactness.  q(x) = floor(((double)x - lo) * inv) is monotone in x, so a point whose cell lies
// beyond the face with finest coordinate Q has x - lo >= Q * cell * (1 - 2^-50) (two fp64 roundings in q, two in the
// product); the gap from the query to it is evaluated in fp64, lowered by `margin` = 2^-48 of the largest coordinate
// magnitude (its own three roundings are below 2^-51 of it) and rounded DOWN to a float g.  Every point behind that face
// then has |fl(x' - x)| >= g, because fp32 subtraction is monotone and g is a float below the real difference, hence a
// computed d2 >= fl(g * g) by the monotonicity of the fp32 product and sums.  So a K-th d2 below fl(g * g) on all six
// sides cannot be beaten or tied by any point outside the block; a rounding can only cost one more level.
// Distances are fl(a - b) per axis, ((dx dx + dy dy) + dz dz), sqrt: symmetric in the pair, independent of the level,
// of the launch shape and of the run.  Integer work only otherwise; no atomics.
#include "cloud_grid.hpp"

namespace {

constexpr int MAX_K = 8;

template <int K>
__global__ __launch_bounds__(TB) void knn_kernel(int32_t N, const uint64_t *__restrict__ codes, const float4 *__restrict__ pts,
                                                 const Grid *__restrict__ grid, float *__restrict__ dist, int32_t *__restrict__ idx) {
    const int64_t t64 = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (t64 >= N) return;
    const int32_t t = (int32_t)t64;
    const float4 me = pts[t];
    const int32_t self = __float_as_int(me.w);
    if (grid->bad) {                     // the caller reads *status; nothing is searched
        for (int s = 0; s < K; ++s) {
            dist[(int64_t)self * K + s] = NAN;
            if (idx) idx[(int64_t)self * K + s] = -1;
        }
        return;
    }
    const double inv = grid->inv, cell = grid->cell, margin = grid->margin;
    const float p[3] = {me.x, me.y, me.z};
    double lo[3];
    uint32_t q[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = grid->lo[a];
        q[a] = quantise(p[a], lo[a], inv);
    }
    const uint64_t mine = codes[t];
    int L = QBITS;
    if (t >= K) L = min(L, common_level(mine, codes[t - K]));
    if (t + K < N) L = min(L, common_level(mine, codes[t + K]));
    L = max(L - 1, 0);

    float bd[K];
    int32_t bi[K];
    for (;; ++L) {
#pragma unroll
        for (int s = 0; s < K; ++s) { bd[s] = INFINITY; bi[s] = 0x7fffffff; }
        const int32_t ncell = 1 << (QBITS - L);
        const int32_t c[3] = {(int32_t)(q[0] >> L), (int32_t)(q[1] >> L), (int32_t)(q[2] >> L)};
        for (int dz = -1; dz <= 1; ++dz) {
            const int32_t z = c[2] + dz;
            if (z < 0 || z >= ncell) continue;
            for (int dy = -1; dy <= 1; ++dy) {
                const int32_t y = c[1] + dy;
                if (y < 0 || y >= ncell) continue;
                for (int dx = -1; dx <= 1; ++dx) {
                    const int32_t x = c[0] + dx;
                    if (x < 0 || x >= ncell) continue;
                    const uint64_t first = morton((uint32_t)x, (uint32_t)y, (uint32_t)z) << (3 * L);
                    const uint64_t end = first + (1ULL << (3 * L));
                    for (int32_t j = lower_bound(codes, N, first); j < N && codes[j] < end; ++j) {
                        if (j == t) continue;
                        const float4 o = pts[j];
                        const float ex = p[0] - o.x, ey = p[1] - o.y, ez = p[2] - o.z;
                        const float d2 = (ex * ex + ey * ey) + ez * ez;
                        const int32_t oi = __float_as_int(o.w);
                        if (d2 < bd[K - 1] || (d2 == bd[K - 1] && oi < bi[K - 1])) {
                            bd[K - 1] = d2;
                            bi[K - 1] = oi;
#pragma unroll
                            for (int s = K - 1; s > 0; --s) {
                                const bool up = bd[s] < bd[s - 1] || (bd[s] == bd[s - 1] && bi[s] < bi[s - 1]);
                                const float fd = bd[s - 1];
                                const int32_t fi = bi[s - 1];
                                bd[s - 1] = up ? bd[s] : fd;
                                bi[s - 1] = up ? bi[s] : fi;
                                bd[s] = up ? fd : bd[s];
                                bi[s] = up ? fi : bi[s];
                            }
                        }
                    }
                }
            }
        }
        if (L >= QBITS) break;           // the block was the whole cloud
        float bound2 = INFINITY;
        for (int a = 0; a < 3; ++a) {
            const int64_t q_hi = (int64_t)(c[a] + 2) << L;      // first finest coordinate behind the upper face
            if (q_hi <= (int64_t)QMAX) {
                const float g = float_below((lo[a] + ((double)q_hi * cell) * (1.0 - 0x1p-50)) - (double)p[a] - margin);
                bound2 = fminf(bound2, g * g);
            }
            if (c[a] >= 1) {
                const int64_t q_lo = (int64_t)(c[a] - 1) << L;  // the lower face: points below it have a coordinate < q_lo
                const float g = float_below((double)p[a] - (lo[a] + ((double)q_lo * cell) * (1.0 + 0x1p-50)) - margin);
                bound2 = fminf(bound2, g * g);
            }
        }
        if (bd[K - 1] < bound2) break;
    }
#pragma unroll
    for (int s = 0; s < K; ++s) {
        dist[(int64_t)self * K + s] = sqrtf(bd[s]);
        if (idx) idx[(int64_t)self * K + s] = bi[s];
    }
}

template <int K>
void launch_knn(int64_t N, const Ws &w, float *dist, int32_t *idx, hipStream_t st) {
    knn_kernel<K><<<(unsigned)ceil_div64(N, TB), TB, 0, st>>>((int32_t)N, w.codes, w.pts, w.grid, dist, idx);
}

constexpr float C0 = 0.28209479177387814f;

// log(x / (1 - x)) as torch.logit evaluates it in fp32; the logarithm itself is rounded from fp64
__device__ inline float logitf(float x) { return (float)log((double)(x / (1.f - x))); }

// rotate_vector_to_vector([0, 0, 1], n) followed by matrix_to_quaternion (gaussian_model/utils.py:120-199), operation by
// operation in fp32.  With u = (0, 0, 1) the cross-product matrix K = Ru u^T - u Ru^T has K02 = Ru0, K12 = Ru1, K20 = -Ru0,
// K21 = -Ru1 and zeros elsewhere; the zero products of K K are left out where they only add a signed zero to (I + K), which
// is never -0.
__device__ inline void normal_to_quat(const float n[3], float qt[4]) {
    const float nn = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    const float a[3] = {n[0] / nn, n[1] / nn, n[2] / nn};                  // populate_modules normalises,
    const float an = sqrtf((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
    const float r[3] = {a[0] / an, a[1] / an, a[2] / an};                  // rotate_vector_to_vector again
    const float c = (0.f * r[0] + 0.f * r[1]) + 1.f * r[2];
    const float d = 1.f + c, z = 0.f / d;
    float m[3][3];
    m[0][0] = (1.f + 0.f) + (r[0] * -r[0]) / d;
    m[0][1] = (0.f + 0.f) + (r[0] * -r[1]) / d;
    m[0][2] = (0.f + r[0]) + z;
    m[1][0] = (0.f + 0.f) + (r[1] * -r[0]) / d;
    m[1][1] = (1.f + 0.f) + (r[1] * -r[1]) / d;
    m[1][2] = (0.f + r[1]) + z;
    m[2][0] = (0.f + -r[0]) + z;
    m[2][1] = (0.f + -r[1]) + z;
    m[2][2] = (1.f + (r[2] - r[2])) + ((-r[0] * r[0] + -r[1] * r[1]) + 0.f) / d;
    if (fabsf(c - 1.f) < 1.0e-10f)
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) m[i][j] = i == j ? 1.f : 0.f;
    if (fabsf(c + 1.f) < 1.0e-10f)
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) m[i][j] = i == j ? -1.f : -0.f;   // -torch.eye(3)
    const float trace = (m[0][0] + m[1][1]) + m[2][2];
    if (trace > 0.f) {
        const float S = sqrtf(trace + 1.f) * 2.f;
        qt[0] = 0.25f * S;
        qt[1] = (m[2][1] - m[1][2]) / S;
        qt[2] = (m[0][2] - m[2][0]) / S;
        qt[3] = (m[1][0] - m[0][1]) / S;
    } else if (m[0][0] > m[1][1] && m[0][0] > m[2][2]) {
        const float S = sqrtf(((1.f + m[0][0]) - m[1][1]) - m[2][2]) * 2.f;
        qt[0] = (m[2][1] - m[1][2]) / S;
        qt[1] = 0.25f * S;
        qt[2] = (m[0][1] + m[1][0]) / S;
        qt[3] = (m[0][2] + m[2][0]) / S;
    } else if (m[1][1] > m[2][2]) {
        const float S = sqrtf(((1.f + m[1][1]) - m[0][0]) - m[2][2]) * 2.f;
        qt[0] = (m[0][2] - m[2][0]) / S;
        qt[1] = (m[0][1] + m[1][0]) / S;
        qt[2] = 0.25f * S;
        qt[3] = (m[1][2] + m[2][1]) / S;
    } else {
        const float S = sqrtf(((1.f + m[2][2]) - m[0][0]) - m[1][1]) * 2.f;
        qt[0] = (m[1][0] - m[0][1]) / S;
        qt[1] = (m[0][2] + m[2][0]) / S;
        qt[2] = (m[1][2] + m[2][1]) / S;
        qt[3] = 0.25f * S;
    }
}

__global__ __launch_bounds__(TB) void seed_kernel(int64_t N, int k, const float *__restrict__ knn, const float *__restrict__ rgb,
                                                  const float *__restrict__ normals, int sh_degree, int scale_dim,
                                                  float *__restrict__ scales, float *__restrict__ quats, float *__restrict__ dc,
                                                  int64_t dc_stride, float *__restrict__ opac) {
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= N) return;
    float sum = knn[i * k];
    for (int s = 1; s < k; ++s) sum += knn[i * k + s];
    const float avg = sum / (float)k;
    const float ls = (float)log((double)avg);
    for (int s = 0; s < scale_dim; ++s) scales[i * scale_dim + s] = ls;
    if (normals && scale_dim == 3) {
        scales[i * 3 + 2] = (float)log((double)(avg / 10.f));
        const float n[3] = {normals[i * 3], normals[i * 3 + 1], normals[i * 3 + 2]};
        float qt[4];
        normal_to_quat(n, qt);
        for (int s = 0; s < 4; ++s) quats[i * 4 + s] = qt[s];
    }
    for (int ch = 0; ch < 3; ++ch) {
        const float x = rgb[i * 3 + ch] / 255.f;
        dc[i * dc_stride + ch] = sh_degree > 0 ? (x - 0.5f) / C0 : logitf(fminf(fmaxf(x, 1e-10f), 1.f - 1e-10f));
    }
    opac[i] = logitf(0.1f * 1.f);
}

}  // namespace


extern "C" int mtgs_knn_workspace_bytes(int64_t N, int k, size_t *bytes) {
    const char *fn = "mtgs_knn_workspace_bytes";
    MTGS_REQUIRE(N >= 0 && N < ((int64_t)1 << 31), MTGS_EINVAL, "%s: N outside [0, 2^31) (%lld)", fn, (long long)N);
    MTGS_REQUIRE(k >= 1 && k <= MAX_K, MTGS_EINVAL, "%s: k outside [1, %d] (%d)", fn, MAX_K, k);
    MTGS_NONNULL(fn, bytes);
    Ws w;
    if (int rc = layout(N > 0 ? N : 1, nullptr, w)) return rc;
    *bytes = w.total;
    return MTGS_OK;
}

extern "C" int mtgs_knn(int64_t N, int k, const float *points, int64_t row_stride, float *dist, int32_t *idx, int32_t *status,
                        void *ws, size_t ws_bytes, void *stream) {
    const char *fn = "mtgs_knn";
    MTGS_REQUIRE(N >= 0 && N < ((int64_t)1 << 31), MTGS_EINVAL, "%s: N outside [0, 2^31) (%lld)", fn, (long long)N);
    MTGS_REQUIRE(k >= 1 && k <= MAX_K, MTGS_EINVAL, "%s: k outside [1, %d] (%d)", fn, MAX_K, k);
    if (N == 0) return MTGS_OK;
    MTGS_REQUIRE(N > k, MTGS_EINVAL, "%s: N must exceed k (N = %lld, k = %d)", fn, (long long)N, k);
    MTGS_REQUIRE(row_stride >= 3, MTGS_EINVAL, "%s: row_stride < 3 (%lld)", fn, (long long)row_stride);
    MTGS_NONNULL(fn, points); MTGS_NONNULL(fn, dist); MTGS_NONNULL(fn, status); MTGS_NONNULL(fn, ws);
    Ws w;
    if (int rc = layout(N, ws, w)) return rc;
    MTGS_REQUIRE(ws_bytes >= w.total, MTGS_EWORKSPACE, "%s: workspace %zu < %zu bytes", fn, ws_bytes, w.total);
    MTGS_REQUIRE(((uintptr_t)ws & 15) == 0, MTGS_EINVAL, "%s: workspace must be 16-byte aligned", fn);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = sort_front(fn, N, points, row_stride, status, w, st)) return rc;
    switch (k) {
        case 1: launch_knn<1>(N, w, dist, idx, st); break;
        case 2: launch_knn<2>(N, w, dist, idx, st); break;
        case 3: launch_knn<3>(N, w, dist, idx, st); break;
        case 4: launch_knn<4>(N, w, dist, idx, st); break;
        case 5: launch_knn<5>(N, w, dist, idx, st); break;
        case 6: launch_knn<6>(N, w, dist, idx, st); break;
        case 7: launch_knn<7>(N, w, dist, idx, st); break;
        default: launch_knn<8>(N, w, dist, idx, st); break;
    }
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}

extern "C" int mtgs_seed_fwd(int64_t N, int k, const float *knn_dist, const float *rgb, const float *normals, int sh_degree,
                             int scale_dim, float *scales, float *quats, float *features_dc, int64_t dc_row_stride,
                             float *opacities, void *stream) {
    const char *fn = "mtgs_seed_fwd";
    MTGS_REQUIRE(N >= 0, MTGS_EINVAL, "%s: N < 0", fn);
    MTGS_REQUIRE(k >= 1 && k <= MAX_K, MTGS_EINVAL, "%s: k outside [1, %d] (%d)", fn, MAX_K, k);
    MTGS_REQUIRE(sh_degree >= 0 && sh_degree <= MTGS_MAX_SH_DEGREE, MTGS_EINVAL, "%s: sh_degree outside [0, %d] (%d)", fn,
                 MTGS_MAX_SH_DEGREE, sh_degree);
    MTGS_REQUIRE(scale_dim == 1 || scale_dim == 3, MTGS_EINVAL, "%s: scale_dim must be 1 or 3 (%d)", fn, scale_dim);
    MTGS_REQUIRE(dc_row_stride >= 3, MTGS_EINVAL, "%s: dc_row_stride < 3 (%lld)", fn, (long long)dc_row_stride);
    if (N == 0) return MTGS_OK;
    MTGS_NONNULL(fn, knn_dist); MTGS_NONNULL(fn, rgb); MTGS_NONNULL(fn, scales); MTGS_NONNULL(fn, features_dc);
    MTGS_NONNULL(fn, opacities);
    MTGS_REQUIRE(!(normals && scale_dim == 3) || quats, MTGS_EINVAL, "%s: null pointer: quats (normals given)", fn);
    seed_kernel<<<(unsigned)ceil_div64(N, TB), TB, 0, (hipStream_t)stream>>>(N, k, knn_dist, rgb, normals, sh_degree, scale_dim, scales,
                                                                           quats, features_dc, dc_row_stride, opacities);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}
