// cloud.hip -- preparing the seeding point cloud on the device (NuPlanDataparser._load_3D_points, mtgs/dataset/nuplan_dataparser.py:
// 460-500): open3d's remove_statistical_outlier and voxel_down_sample, on the Morton-sorted view of cloud_grid.hpp.
//
// mtgs_cloud_outlier, one call =
//   sort_front (cloud_grid.hpp)  bounding box and grid, Morton codes, one stable sort, the sorted points as float4
//   mean_knn_kernel<CAP>         one thread per query, in Morton order: the kk = k - 1 nearest OTHER points -> avg[i]
//   stat_partial / stat_finish   twice: cloud_mean, then std and the threshold (fixed-order fp64 trees, block_reduce.hpp)
//   keep_kernel                  keep[i] = avg[i] > 0 && avg[i] < threshold
// The search is the walk of seed.hip with the list generalised from K <= 8 (a template parameter) to a run-time kk <= 31.
// A cell of side 2^L finest cells is one contiguous range of the sorted array.  A query visits the 3x3x3 block of level-L cells
// around its own, keeps the kk smallest (d2, index) and accepts when the kk-th d2 is STRICTLY below the squared distance to the
// nearest face of the block that has cells behind it; otherwise it goes up one level (the block of level 21 is the whole
// cloud).  The first level is the smallest cell that holds the query and the kk entries before or behind it, minus one.
//
// The list.  CAP registers pairs (d2, index) per thread, CAP = kk rounded up to 8, ascending and RIGHT-ALIGNED: the kk live
// slots are [CAP - kk, CAP), the slots below them hold the sentinel (-inf, -1), which compares below every candidate and so
// never moves.  The kk-th best is then always slot CAP - 1 and every index is a compile-time constant: the list stays in
// VGPRs with no run-time indexing, no scratch and no LDS, so occupancy is set by registers alone.  The compiler reports 70 /
// 113 / 166 / 194 VGPRs for CAP = 8 / 16 / 24 / 32, that is 7 / 4 / 3 / 2 waves per SIMD, no scratch (CAP = 24 serves the
// default nb_neighbors = 20).  A list in LDS would cost 8 CAP bytes per thread, 2.5 waves per SIMD at CAP = 32 and 3.3 at
// CAP = 24, and an LDS round trip per compare-exchange: no better at the sizes that matter, so registers it is.
// An accepted candidate replaces slot CAP - 1 and sinks by CAP - 1 predicated compare-exchanges.
//
// Exactness (DESIGN.md sections 11 and 12).  q(x) = floor(((double)x - lo) * inv) is monotone in x, so a point whose cell lies
// beyond the face with finest coordinate Q has x - lo >= Q * cell * (1 - 2^-50) (two fp64 roundings in q, two in the
// product); the gap from the query to it is evaluated in fp64, lowered by `margin` = 2^-48 of the largest coordinate
// magnitude (its own three roundings are below 2^-51 of it) and rounded DOWN to a float g.  Every point behind that face
// then has |fl(x' - x)| >= g, because fp32 subtraction is monotone and g is a float below the real difference, hence a
// computed d2 >= fl(g * g) by the monotonicity of the fp32 product and sums.  So a kk-th d2 below fl(g * g) on all six
// sides cannot be beaten or tied by any point outside the block; a rounding can only cost one more level.  Nothing in this
// argument depends on the length of the list.  d2 = ((dx dx + dy dy) + dz dz) with dx = fl(a.x - b.x) in fp32, ties by the
// smaller index: the accepted SET of (d2, index) pairs is a function of the cloud alone.
//
// Order of summation.  avg[i] = (sum over the list, ascending (d2, index), of sqrt((double)d2)) / k in fp64, one thread, one
// fixed order: bitwise independent of the level reached, of the launch shape and of the run; and since equal d2 give equal
// terms, permuting the rows of the cloud permutes avg and changes no bit of it.  cloud_mean and std are sums over i in a
// fixed order that depends on N alone (grid-strided partials, a halving tree per block, one more tree over the blocks).
//
// mtgs_cloud_voxel, one call =
//   bbox_front (cloud_grid.hpp)  the minimum corner (fixed-order fp32 min), the non-finite flag
//   voxel_key_kernel             index = floor(((double)p - (min - voxel_size / 2)) / voxel_size) per axis, 21 bits each -> key
//   mtgs_sort_pairs              (key, index) sorted once; equal keys stay in index order (stable)
//   mtgs_scan                    voxel heads (key differs from its predecessor) -> first sorted position of every voxel, M
//   voxel_kernel                 one thread per voxel: sequential fp64 sums of its points in index order, one division
// Compiled with -ffp-contract=off: every operation above rounds once, as the NumPy transcription does.  Integer atomicOr on
// the status word only; no float atomics.
#include "block_reduce.hpp"
#include "cloud_grid.hpp"
#include "scan.hpp"

namespace {

constexpr int MIN_NB = 2, MAX_NB = 32;      // nb_neighbors; the list holds nb_neighbors - 1 <= 31 entries

template <int CAP>
__global__ __launch_bounds__(TB) void mean_knn_kernel(int32_t N, int kk, int k, const uint64_t *__restrict__ codes,
                                                      const float4 *__restrict__ pts, const Grid *__restrict__ grid,
                                                      double *__restrict__ avg) {
    const int64_t t64 = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (t64 >= N) return;
    const int32_t t = (int32_t)t64;
    const float4 me = pts[t];
    const int32_t self = __float_as_int(me.w);
    if (grid->bad) {                     // the caller reads *status; nothing is searched
        avg[self] = NAN;
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
    if (t >= kk) L = min(L, common_level(mine, codes[t - kk]));
    if (t + kk < N) L = min(L, common_level(mine, codes[t + kk]));
    L = max(L - 1, 0);

    float bd[CAP];
    int32_t bi[CAP];
    for (;; ++L) {
#pragma unroll
        for (int s = 0; s < CAP; ++s) {
            const bool live = s >= CAP - kk;
            bd[s] = live ? INFINITY : -INFINITY;
            bi[s] = live ? 0x7fffffff : -1;
        }
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
                        if (d2 < bd[CAP - 1] || (d2 == bd[CAP - 1] && oi < bi[CAP - 1])) {
                            bd[CAP - 1] = d2;
                            bi[CAP - 1] = oi;
#pragma unroll
                            for (int s = CAP - 1; s > 0; --s) {
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
        if (bd[CAP - 1] < bound2) break;  // kk = 0 (N = 1): the sentinel accepts at once
    }
    double sum = 0.0;                    // the query itself is the k-th neighbour, at distance 0
#pragma unroll
    for (int s = 0; s < CAP; ++s)
        if (s >= CAP - kk) sum += sqrt((double)bd[s]);
    avg[self] = sum / (double)k;
}

// PASS 0: the sum of avg over avg > 0;  PASS 1: the sum of (avg - cloud_mean)^2 over avg > 0.  part[b] = block b's share
template <int PASS>
__global__ __launch_bounds__(TB) void stat_partial_kernel(int64_t N, const double *__restrict__ avg, const double *__restrict__ stats,
                                                          double *__restrict__ part) {
    __shared__ double lds[TB];
    const double mean = PASS ? stats[0] : 0.0;
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < N; i += (int64_t)gridDim.x * TB) {
        const double a = avg[i];
        if (a > 0.0) acc += PASS ? (a - mean) * (a - mean) : a;
    }
    const double total = block_tree_sum_f64<TB>(acc, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = total;
}

// one block: PASS 0 -> stats[0] = cloud_mean, stats[3] = valid;  PASS 1 -> stats[1] = std, stats[2] = threshold
template <int PASS>
__global__ __launch_bounds__(TB) void stat_finish_kernel(int nb, const double *__restrict__ part, int64_t N, double std_ratio,
                                                         double *__restrict__ stats) {
    __shared__ double lds[TB];
    double acc = 0.0;
    for (int b = threadIdx.x; b < nb; b += TB) acc += part[b];
    const double total = block_tree_sum_f64<TB>(acc, lds);
    if (threadIdx.x != 0) return;
    if (PASS == 0) {
        stats[0] = total / (double)N;
        stats[3] = (double)N;
    } else {
        const double sd = sqrt(total / (double)(N - 1));          // N = 1: 0 / 0, a NaN threshold, nothing kept
        stats[1] = sd;
        stats[2] = stats[0] + std_ratio * sd;
    }
}

__global__ __launch_bounds__(TB) void keep_kernel(int64_t N, const double *__restrict__ avg, const double *__restrict__ stats,
                                                  uint8_t *__restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= N) return;
    const double a = avg[i];
    keep[i] = a > 0.0 && a < stats[2] ? 1 : 0;
}

template <int CAP>
void launch_mean_knn(int64_t N, int kk, int k, const Ws &w, double *avg, hipStream_t st) {
    mean_knn_kernel<CAP><<<(unsigned)ceil_div64(N, TB), TB, 0, st>>>((int32_t)N, kk, k, w.codes, w.pts, w.grid, avg);
}

// ---- the voxel grid ----

struct VoxelWs {
    Grid *grid;
    float *part;
    uint64_t *keys_in, *keys;
    int32_t *ids_in, *ids, *start;      // start[v]: first sorted position of voxel v
    int64_t *scan_ws, *total;
    void *sort_ws;
    size_t sort_bytes, bytes;
};

int voxel_layout(int64_t N, void *ws, VoxelWs &w) {
    char *p = (char *)ws;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char *q = p ? p + off : nullptr;
        off += align256(bytes);
        return q;
    };
    w.grid = (Grid *)take(sizeof(Grid));
    w.part = (float *)take((size_t)bbox_grid(N) * 8 * sizeof(float));
    w.keys_in = (uint64_t *)take((size_t)N * 8);
    w.keys = (uint64_t *)take((size_t)N * 8);
    w.ids_in = (int32_t *)take((size_t)N * 4);
    w.ids = (int32_t *)take((size_t)N * 4);
    w.start = (int32_t *)take((size_t)N * 4);
    w.scan_ws = (int64_t *)take(mtgs_scan::workspace_bytes(N));
    w.total = (int64_t *)take(sizeof(int64_t));
    if (int rc = mtgs_sort_workspace_bytes(N, &w.sort_bytes)) return rc;
    w.sort_ws = take(w.sort_bytes);
    w.bytes = off;
    return MTGS_OK;
}

// status bits: 1 = a coordinate is not finite (grid_kernel), 2 << axis = the index of that axis needs more than 21 bits
__global__ __launch_bounds__(TB) void voxel_key_kernel(int64_t N, const float *__restrict__ pts, int64_t stride, const Grid *__restrict__ grid,
                                                       double voxel_size, uint64_t *__restrict__ keys, int32_t *__restrict__ ids,
                                                       int32_t *__restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= N) return;
    ids[i] = (int32_t)i;
    if (grid->bad) {
        keys[i] = 0;
        return;
    }
    uint64_t key = 0;
    int over = 0;
    for (int a = 0; a < 3; ++a) {
        const double voxel_min_bound = grid->lo[a] - voxel_size * 0.5;
        double u = floor(((double)pts[i * stride + a] - voxel_min_bound) / voxel_size);
        if (!(u <= (double)QMAX)) {
            over |= 2 << a;
            u = (double)QMAX;
        }
        key = key << QBITS | (uint64_t)(u > 0.0 ? u : 0.0);
    }
    keys[i] = key;
    if (over) atomicOr(status, over);
}

struct HeadValue {
    const uint64_t *keys;
    __device__ int64_t operator()(int64_t t) const { return t == 0 || keys[t] != keys[t - 1] ? 1 : 0; }
};
struct HeadSink {
    int32_t *start;
    __device__ void operator()(int64_t t, int64_t excl, int64_t incl) const {
        if (incl != excl) start[excl] = (int32_t)t;
    }
};

// open3d's AccumulatedPoint: point_ += p, color_ += c per point in ascending original index, then one division by the count
template <bool U8>
__global__ __launch_bounds__(TB) void voxel_kernel(int64_t N, const int64_t *__restrict__ total, const int32_t *__restrict__ start,
                                                   const uint64_t *__restrict__ keys, const int32_t *__restrict__ ids,
                                                   const float *__restrict__ pts, int64_t stride, const void *__restrict__ colors,
                                                   double *__restrict__ out_xyz, double *__restrict__ out_rgb, int32_t *__restrict__ counts,
                                                   int64_t *__restrict__ out_keys, int32_t *__restrict__ n_voxels) {
    const int64_t v = (int64_t)blockIdx.x * TB + threadIdx.x;
    const int64_t M = *total;
    if (v == 0) *n_voxels = (int32_t)M;
    if (v >= M) return;
    const int64_t b = start[v], e = v + 1 < M ? (int64_t)start[v + 1] : N;
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t t = b; t < e; ++t) {
        const int64_t i = ids[t];
        for (int a = 0; a < 3; ++a) {
            s[a] += (double)pts[i * stride + a];
            s[3 + a] += U8 ? (double)((const uint8_t *)colors)[i * 3 + a] / 255.0 : (double)((const float *)colors)[i * 3 + a];
        }
    }
    const double n = (double)(e - b);
    for (int a = 0; a < 3; ++a) {
        out_xyz[v * 3 + a] = s[a] / n;
        out_rgb[v * 3 + a] = s[3 + a] / n;
    }
    counts[v] = (int32_t)(e - b);
    if (out_keys) out_keys[v] = (int64_t)keys[b];
}

size_t stat_part_bytes(int64_t N) { return align256((size_t)bbox_grid(N) * sizeof(double)); }

}  // namespace

#define CLOUD_NB(fn, nb) \
    MTGS_REQUIRE(nb >= MIN_NB && nb <= MAX_NB, MTGS_EINVAL, "%s: nb_neighbors outside [%d, %d] (%d)", fn, MIN_NB, MAX_NB, nb)

extern "C" int mtgs_cloud_outlier_workspace_bytes(int64_t N, int nb_neighbors, size_t *bytes) {
    const char *fn = "mtgs_cloud_outlier_workspace_bytes";
    MTGS_COUNT31(fn, N);
    CLOUD_NB(fn, nb_neighbors);
    MTGS_NONNULL(fn, bytes);
    Ws w;
    if (int rc = layout(N > 0 ? N : 1, nullptr, w)) return rc;
    *bytes = w.total + stat_part_bytes(N);
    return MTGS_OK;
}

extern "C" int mtgs_cloud_outlier(int64_t N, int nb_neighbors, double std_ratio, const float *points, int64_t row_stride, double *avg,
                                  double *stats, uint8_t *keep, int32_t *status, void *ws, size_t ws_bytes, void *stream) {
    const char *fn = "mtgs_cloud_outlier";
    MTGS_COUNT31(fn, N);
    CLOUD_NB(fn, nb_neighbors);
    if (N == 0) return MTGS_OK;
    MTGS_REQUIRE(row_stride >= 3, MTGS_EINVAL, "%s: row_stride < 3 (%lld)", fn, (long long)row_stride);
    MTGS_NONNULL(fn, points); MTGS_NONNULL(fn, avg); MTGS_NONNULL(fn, stats); MTGS_NONNULL(fn, keep); MTGS_NONNULL(fn, status);
    MTGS_NONNULL(fn, ws);
    Ws w;
    if (int rc = layout(N, ws, w)) return rc;
    const size_t need = w.total + stat_part_bytes(N);
    MTGS_REQUIRE(ws_bytes >= need, MTGS_EWORKSPACE, "%s: workspace %zu < %zu bytes", fn, ws_bytes, need);
    MTGS_REQUIRE(((uintptr_t)ws & 15) == 0, MTGS_EINVAL, "%s: workspace must be 16-byte aligned", fn);
    double *part = (double *)((char *)ws + w.total);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = sort_front(fn, N, points, row_stride, status, w, st)) return rc;
    const int k = (int)(N < nb_neighbors ? N : nb_neighbors), kk = k - 1;     // open3d's knn = min(nb_neighbors, N), the query included
    if (kk <= 8) launch_mean_knn<8>(N, kk, k, w, avg, st);
    else if (kk <= 16) launch_mean_knn<16>(N, kk, k, w, avg, st);
    else if (kk <= 24) launch_mean_knn<24>(N, kk, k, w, avg, st);
    else launch_mean_knn<32>(N, kk, k, w, avg, st);
    MTGS_CHECK_LAUNCH(fn);
    const int nb = bbox_grid(N);
    const unsigned blocks = (unsigned)ceil_div64(N, TB);
    stat_partial_kernel<0><<<nb, TB, 0, st>>>(N, avg, stats, part);
    MTGS_CHECK_LAUNCH(fn);
    stat_finish_kernel<0><<<1, TB, 0, st>>>(nb, part, N, std_ratio, stats);
    MTGS_CHECK_LAUNCH(fn);
    stat_partial_kernel<1><<<nb, TB, 0, st>>>(N, avg, stats, part);
    MTGS_CHECK_LAUNCH(fn);
    stat_finish_kernel<1><<<1, TB, 0, st>>>(nb, part, N, std_ratio, stats);
    MTGS_CHECK_LAUNCH(fn);
    keep_kernel<<<blocks, TB, 0, st>>>(N, avg, stats, keep);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}

extern "C" int mtgs_cloud_voxel_workspace_bytes(int64_t N, size_t *bytes) {
    const char *fn = "mtgs_cloud_voxel_workspace_bytes";
    MTGS_COUNT31(fn, N);
    MTGS_NONNULL(fn, bytes);
    VoxelWs w;
    if (int rc = voxel_layout(N > 0 ? N : 1, nullptr, w)) return rc;
    *bytes = w.bytes;
    return MTGS_OK;
}

extern "C" int mtgs_cloud_voxel(int64_t N, double voxel_size, const float *points, int64_t row_stride, const void *colors, int colors_u8,
                                double *out_xyz, double *out_rgb, int32_t *counts, int64_t *out_keys, int32_t *n_voxels,
                                int32_t *status, void *ws, size_t ws_bytes, void *stream) {
    const char *fn = "mtgs_cloud_voxel";
    MTGS_COUNT31(fn, N);
    MTGS_REQUIRE(voxel_size > 0.0 && isfinite(voxel_size), MTGS_EINVAL, "%s: voxel_size must be positive and finite (%g)", fn, voxel_size);
    if (N == 0) return MTGS_OK;
    MTGS_REQUIRE(row_stride >= 3, MTGS_EINVAL, "%s: row_stride < 3 (%lld)", fn, (long long)row_stride);
    MTGS_NONNULL(fn, points); MTGS_NONNULL(fn, colors); MTGS_NONNULL(fn, out_xyz); MTGS_NONNULL(fn, out_rgb); MTGS_NONNULL(fn, counts);
    MTGS_NONNULL(fn, n_voxels); MTGS_NONNULL(fn, status); MTGS_NONNULL(fn, ws);
    VoxelWs w;
    if (int rc = voxel_layout(N, ws, w)) return rc;
    MTGS_REQUIRE(ws_bytes >= w.bytes, MTGS_EWORKSPACE, "%s: workspace %zu < %zu bytes", fn, ws_bytes, w.bytes);
    MTGS_REQUIRE(((uintptr_t)ws & 15) == 0, MTGS_EINVAL, "%s: workspace must be 16-byte aligned", fn);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = bbox_front(fn, N, points, row_stride, status, w.part, w.grid, st)) return rc;
    const unsigned blocks = (unsigned)ceil_div64(N, TB);
    voxel_key_kernel<<<blocks, TB, 0, st>>>(N, points, row_stride, w.grid, voxel_size, w.keys_in, w.ids_in, status);
    MTGS_CHECK_LAUNCH(fn);
    if (int rc = mtgs_sort_pairs(N, 3 * QBITS, (int64_t *)w.keys_in, w.ids_in, (int64_t *)w.keys, w.ids, w.sort_ws, w.sort_bytes, stream))
        return rc;
    mtgs_scan::run(N, HeadValue{w.keys}, HeadSink{w.start}, w.scan_ws, w.total, st);
    MTGS_CHECK_LAUNCH(fn);
    if (colors_u8)
        voxel_kernel<true><<<blocks, TB, 0, st>>>(N, w.total, w.start, w.keys, w.ids, points, row_stride, colors, out_xyz, out_rgb, counts,
                                                  out_keys, n_voxels);
    else
        voxel_kernel<false><<<blocks, TB, 0, st>>>(N, w.total, w.start, w.keys, w.ids, points, row_stride, colors, out_xyz, out_rgb, counts,
                                                   out_keys, n_voxels);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}
