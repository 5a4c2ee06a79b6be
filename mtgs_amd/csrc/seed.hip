// seed.hip -- building a Gaussian node from a point cloud on the device (VanillaGaussianSplattingModel.populate_modules,
// mtgs/scene_model/gaussian_model/vanilla_gaussian_splatting.py:114-196): the exact k nearest neighbours of every point
// (k_nearest_sklearn, :372-390) and one fused per-point kernel for scales, rotations, colours and opacities.
//
// mtgs_knn, one call =
//   bbox_kernel + grid_kernel   bounding box (fixed-order min / max), the cubic cell size, the non-finite flag
//   morton_kernel               21 bits per axis -> 63-bit Morton code of every point
//   mtgs_sort_pairs             (code, index) sorted once; equal codes stay in index order (stable)
//   gather_kernel               sorted points as float4 (x, y, z, index bits)
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
#include "common.hpp"

#include <math.h>

namespace {

constexpr int TB = 256;
constexpr int MAX_GRID = 1024;
constexpr int QBITS = 21;
constexpr uint32_t QMAX = (1u << QBITS) - 1u;
constexpr int MAX_K = 8;

struct Grid {
    double lo[3];
    double inv;      // finest cells per unit length (0 when the cloud has no extent)
    double cell;     // 1 / inv (0 when inv is 0)
    double margin;   // absolute slack of a face distance evaluated in fp64
    int bad;         // a coordinate is not finite
    int pad;
};

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

int bbox_grid(int64_t N) {
    const int64_t g = ceil_div64(N, TB * 4);
    return (int)(g < 1 ? 1 : (g > MAX_GRID ? MAX_GRID : g));
}

struct Ws {
    Grid *grid;
    float *part;            // [bbox_grid][8]: min xyz, max xyz, bad, unused
    uint64_t *codes_in, *codes;
    int32_t *ids_in, *ids;
    float4 *pts;
    void *sort_ws;
    size_t sort_bytes, total;
};

int layout(int64_t N, void *ws, Ws &w) {
    char *p = (char *)ws;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char *q = p ? p + off : nullptr;
        off += align256(bytes);
        return q;
    };
    w.grid = (Grid *)take(sizeof(Grid));
    w.part = (float *)take((size_t)bbox_grid(N) * 8 * sizeof(float));
    w.codes_in = (uint64_t *)take((size_t)N * 8);
    w.codes = (uint64_t *)take((size_t)N * 8);
    w.ids_in = (int32_t *)take((size_t)N * 4);
    w.ids = (int32_t *)take((size_t)N * 4);
    w.pts = (float4 *)take((size_t)N * 16);
    if (int rc = mtgs_sort_workspace_bytes(N, &w.sort_bytes)) return rc;
    w.sort_ws = take(w.sort_bytes);
    w.total = off;
    return MTGS_OK;
}

__device__ inline float wave_min(float v) {
    for (int o = MTGS_WAVE / 2; o > 0; o >>= 1) v = fminf(v, __shfl_down(v, o, MTGS_WAVE));
    return v;
}
__device__ inline float wave_max(float v) {
    for (int o = MTGS_WAVE / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_down(v, o, MTGS_WAVE));
    return v;
}

// min / max of the finite coordinates and the non-finite flag of block b's share -> part[b][0..6]
__global__ __launch_bounds__(TB) void bbox_kernel(int64_t N, const float *__restrict__ pts, int64_t stride, float *__restrict__ part) {
    __shared__ float s[7][TB / MTGS_WAVE];
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY}, bad = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < N; i += (int64_t)gridDim.x * TB)
        for (int a = 0; a < 3; ++a) {
            const float v = pts[i * stride + a];
            if (isfinite(v)) {
                mn[a] = fminf(mn[a], v);
                mx[a] = fmaxf(mx[a], v);
            } else {
                bad = 1.f;
            }
        }
    const int w = threadIdx.x / MTGS_WAVE, lane = threadIdx.x % MTGS_WAVE;
    for (int a = 0; a < 3; ++a) {
        const float lo = wave_min(mn[a]), hi = wave_max(mx[a]);
        if (lane == 0) { s[a][w] = lo; s[3 + a][w] = hi; }
    }
    bad = wave_max(bad);
    if (lane == 0) s[6][w] = bad;
    __syncthreads();
    if (threadIdx.x < 7) {
        float v = s[threadIdx.x][0];
        for (int j = 1; j < TB / MTGS_WAVE; ++j) v = threadIdx.x < 3 ? fminf(v, s[threadIdx.x][j]) : fmaxf(v, s[threadIdx.x][j]);
        part[blockIdx.x * 8 + threadIdx.x] = v;
    }
}

// one wave: the partials -> Grid and *status
__global__ __launch_bounds__(MTGS_WAVE) void grid_kernel(int nb, const float *__restrict__ part, Grid *__restrict__ grid,
                                                        int32_t *__restrict__ status) {
    float v[7];
    for (int e = 0; e < 7; ++e) {
        float a = e < 3 ? INFINITY : -INFINITY;
        for (int b = threadIdx.x; b < nb; b += MTGS_WAVE) a = e < 3 ? fminf(a, part[b * 8 + e]) : fmaxf(a, part[b * 8 + e]);
        a = e < 3 ? wave_min(a) : wave_max(a);
        v[e] = a;
    }
    if (threadIdx.x != 0) return;
    double ext = 0.0, mag = 0.0;
    for (int a = 0; a < 3; ++a) {
        const double lo = v[a], hi = v[3 + a];
        grid->lo[a] = lo;
        ext = fmax(ext, hi - lo);
        mag = fmax(mag, fmax(fabs(lo), fabs(hi)));
    }
    const bool bad = v[6] != 0.f || !(ext >= 0.0) || !isfinite(ext);
    // hi maps just below 2^21; no extent (all points equal): every point in cell 0, no division
    const bool flat = bad || ext == 0.0;
    grid->inv = flat ? 0.0 : 2097152.0 * (1.0 - 0x1p-40) / ext;
    grid->cell = flat ? 0.0 : 1.0 / grid->inv;
    grid->margin = mag * 0x1p-48;
    grid->bad = bad ? 1 : 0;
    grid->pad = 0;
    *status = bad ? 1 : 0;
}

__device__ inline uint32_t quantise(float x, double lo, double inv) {
    const double u = ((double)x - lo) * inv;
    return u >= (double)QMAX ? QMAX : (u > 0.0 ? (uint32_t)u : 0u);     // NaN -> 0
}

__device__ inline uint64_t spread3(uint32_t v) {
    uint64_t x = v & 0x1fffffu;
    x = (x | x << 32) & 0x1f00000000ffffULL;
    x = (x | x << 16) & 0x1f0000ff0000ffULL;
    x = (x | x << 8) & 0x100f00f00f00f00fULL;
    x = (x | x << 4) & 0x10c30c30c30c30c3ULL;
    x = (x | x << 2) & 0x1249249249249249ULL;
    return x;
}

__device__ inline uint64_t morton(uint32_t x, uint32_t y, uint32_t z) { return spread3(x) | (spread3(y) << 1) | (spread3(z) << 2); }

__global__ __launch_bounds__(TB) void morton_kernel(int64_t N, const float *__restrict__ pts, int64_t stride, const Grid *__restrict__ grid,
                                                    uint64_t *__restrict__ codes, int32_t *__restrict__ ids) {
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= N) return;
    const double inv = grid->inv;
    uint32_t q[3];
    for (int a = 0; a < 3; ++a) q[a] = quantise(pts[i * stride + a], grid->lo[a], inv);
    codes[i] = morton(q[0], q[1], q[2]);
    ids[i] = (int32_t)i;
}

__global__ __launch_bounds__(TB) void gather_kernel(int64_t N, const float *__restrict__ pts, int64_t stride, const int32_t *__restrict__ ids,
                                                    float4 *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (t >= N) return;
    const int32_t i = ids[t];
    out[t] = make_float4(pts[(int64_t)i * stride], pts[(int64_t)i * stride + 1], pts[(int64_t)i * stride + 2], __int_as_float(i));
}

// first position whose code is >= key
__device__ inline int32_t lower_bound(const uint64_t *__restrict__ codes, int32_t n, uint64_t key) {
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (codes[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the largest float <= g for g > 0, else 0
__device__ inline float float_below(double g) {
    if (!(g > 0.0)) return 0.f;
    float f = (float)g;
    if ((double)f > g) f = __uint_as_float(__float_as_uint(f) - 1u);
    return f;
}

// level of the smallest cell that holds both codes: 0 = the same finest cell
__device__ inline int common_level(uint64_t a, uint64_t b) {
    const uint64_t x = a ^ b;
    return x ? (63 - __clzll((long long)x)) / 3 + 1 : 0;
}

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

#define SEED_NONNULL(fn, p) MTGS_REQUIRE((p) != nullptr, MTGS_EINVAL, "%s: null pointer: %s", fn, #p)

extern "C" int mtgs_knn_workspace_bytes(int64_t N, int k, size_t *bytes) {
    const char *fn = "mtgs_knn_workspace_bytes";
    MTGS_REQUIRE(N >= 0 && N < ((int64_t)1 << 31), MTGS_EINVAL, "%s: N outside [0, 2^31) (%lld)", fn, (long long)N);
    MTGS_REQUIRE(k >= 1 && k <= MAX_K, MTGS_EINVAL, "%s: k outside [1, %d] (%d)", fn, MAX_K, k);
    SEED_NONNULL(fn, bytes);
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
    SEED_NONNULL(fn, points); SEED_NONNULL(fn, dist); SEED_NONNULL(fn, status); SEED_NONNULL(fn, ws);
    Ws w;
    if (int rc = layout(N, ws, w)) return rc;
    MTGS_REQUIRE(ws_bytes >= w.total, MTGS_EWORKSPACE, "%s: workspace %zu < %zu bytes", fn, ws_bytes, w.total);
    MTGS_REQUIRE(((uintptr_t)ws & 15) == 0, MTGS_EINVAL, "%s: workspace must be 16-byte aligned", fn);
    hipStream_t st = (hipStream_t)stream;
    const int nb = bbox_grid(N);
    const unsigned blocks = (unsigned)ceil_div64(N, TB);
    bbox_kernel<<<nb, TB, 0, st>>>(N, points, row_stride, w.part);
    MTGS_CHECK_LAUNCH(fn);
    grid_kernel<<<1, MTGS_WAVE, 0, st>>>(nb, w.part, w.grid, status);
    MTGS_CHECK_LAUNCH(fn);
    morton_kernel<<<blocks, TB, 0, st>>>(N, points, row_stride, w.grid, w.codes_in, w.ids_in);
    MTGS_CHECK_LAUNCH(fn);
    if (int rc = mtgs_sort_pairs(N, 3 * QBITS, (int64_t *)w.codes_in, w.ids_in, (int64_t *)w.codes, w.ids, w.sort_ws, w.sort_bytes, stream))
        return rc;
    gather_kernel<<<blocks, TB, 0, st>>>(N, points, row_stride, w.ids, w.pts);
    MTGS_CHECK_LAUNCH(fn);
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
    SEED_NONNULL(fn, knn_dist); SEED_NONNULL(fn, rgb); SEED_NONNULL(fn, scales); SEED_NONNULL(fn, features_dc);
    SEED_NONNULL(fn, opacities);
    MTGS_REQUIRE(!(normals && scale_dim == 3) || quats, MTGS_EINVAL, "%s: null pointer: quats (normals given)", fn);
    seed_kernel<<<(unsigned)ceil_div64(N, TB), TB, 0, (hipStream_t)stream>>>(N, k, knn_dist, rgb, normals, sh_degree, scale_dim, scales,
                                                                           quats, features_dc, dc_row_stride, opacities);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}
