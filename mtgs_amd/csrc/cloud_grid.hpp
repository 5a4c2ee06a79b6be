// cloud_grid.hpp -- the Morton-sorted view of a point cloud that seed.hip (mtgs_knn) and cloud.hip (the outlier filter and the
// voxel grid) search: the bounding box and the cubic grid over it, 63-bit Morton codes, one radix sort and the sorted copy of the
// points, plus the small device helpers of the octree walk.  sort_front, one call =
//   bbox_kernel + grid_kernel   bounding box (fixed-order min / max), the cubic cell size, the non-finite flag
//   morton_kernel               21 bits per axis -> 63-bit Morton code of every point
//   mtgs_sort_pairs             (code, index) sorted once; equal codes stay in index order (stable)
//   gather_kernel               sorted points as float4 (x, y, z, index bits)
// A cell of side 2^L finest cells is ONE contiguous range of the sorted array (all codes with the same top 63 - 3L bits), found
// by a binary search on the code prefix (lower_bound).  Integer work and fixed-order min / max only; no atomics.
#pragma once
#include "common.hpp"

#include <math.h>

namespace {

constexpr int TB = 256;
constexpr int MAX_GRID = 1024;
constexpr int QBITS = 21;
constexpr uint32_t QMAX = (1u << QBITS) - 1u;

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

// The bounding box and the grid alone (*grid, *status; part: [bbox_grid(N)][8] floats): what the voxel grid needs of the front.
inline int bbox_front(const char *fn, int64_t N, const float *points, int64_t row_stride, int32_t *status, float *part, Grid *grid,
                      hipStream_t st) {
    const int nb = bbox_grid(N);
    bbox_kernel<<<nb, TB, 0, st>>>(N, points, row_stride, part);
    MTGS_CHECK_LAUNCH(fn);
    grid_kernel<<<1, MTGS_WAVE, 0, st>>>(nb, part, grid, status);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}

// The whole front: w.grid, *status, the sorted codes w.codes, their original indices w.ids and the sorted points w.pts.
inline int sort_front(const char *fn, int64_t N, const float *points, int64_t row_stride, int32_t *status, const Ws &w, hipStream_t st) {
    const unsigned blocks = (unsigned)ceil_div64(N, TB);
    if (int rc = bbox_front(fn, N, points, row_stride, status, w.part, w.grid, st)) return rc;
    morton_kernel<<<blocks, TB, 0, st>>>(N, points, row_stride, w.grid, w.codes_in, w.ids_in);
    MTGS_CHECK_LAUNCH(fn);
    if (int rc = mtgs_sort_pairs(N, 3 * QBITS, (int64_t *)w.codes_in, w.ids_in, (int64_t *)w.codes, w.ids, w.sort_ws, w.sort_bytes, (void *)st))
        return rc;
    gather_kernel<<<blocks, TB, 0, st>>>(N, points, row_stride, w.ids, w.pts);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}

}  // namespace
