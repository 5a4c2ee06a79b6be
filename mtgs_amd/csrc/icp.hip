// icp.hip -- lidar sweeps registered against a local voxel map (include/mtgs_icp.h states every rule and the arithmetic;
// mtgs_amd.registration): the KISS-ICP odometry of nuplan_scripts/lidar_registration_multi_traversal.py in this project's canonical
// order.
//
// mtgs_icp_downsample, per level =
//   ds_key_kernel          one lane per point: the range test (level one), the voxel key or the sentinel
//   mtgs_sort::sort_pairs  stable 64-bit sort of (key, index): the first of a run is the point of least index in its voxel
//   ds_flag_kernel         heads of runs flagged back at their index
//   mtgs_scan::run         over the flags in index order; the sink moves a kept row to its place: ascending index
// The map is a table of (key, slot) sorted by key plus per-slot point lists.  mtgs_icp_map_insert =
//   ins_key_kernel, sort_pairs, mtgs_scan::run over the heads that are not in the table (their keys compacted),
//   merge_old_kernel / merge_new_kernel (every entry's place in the merged table by rank: its own rank + a lower bound in the other
//   list), insert_kernel (one lane per touched voxel walks its run in offered order), commit_kernel.  The merged table is built on
//   the side of the table that is not in use and the side flips in commit_kernel, so a refused insert leaves the map as it was.
// One ICP iteration = associate_kernel (one lane per source point, 27 binary searches, the 22 non-zero sums per block by the halving
// tree) + finish_kernel (one workgroup: the block partials in fixed order, LDL^T, SE3::exp, the record).
// The only atomics are integer ones on the state words (an OR of status bits, the count of voxels that hold a point): their result
// does not depend on order.  Compiled with -ffp-contract=off: tests/icp_refs.py is compared bit for bit.
#include "common.hpp"
#include "radix_sort.hpp"
#include "scan.hpp"

#include <float.h>
#include <math.h>

namespace {

constexpr int TB = MTGS_ICP_BLOCK;
constexpr int NCOL = 22;                        // the summed columns: contributions 0..14 and 21..27 of the header's list
constexpr uint64_t SENTINEL = 1ull << 63;       // above every key: such rows sort last and head no run
constexpr double GRID_HALF = 1048576.0;         // 2^20
constexpr int ST_VOXELS = 0, ST_STATUS = 1, ST_LIVE = 2, ST_SIDE = 3;

struct Rows {
    const void *p;
    int f64;
    int64_t stride;
};
__device__ __forceinline__ void load_row(const Rows &r, int64_t i, double x[3]) {
    if (r.f64) {
        const double *q = (const double *)r.p + i * r.stride;
        x[0] = q[0]; x[1] = q[1]; x[2] = q[2];
    } else {
        const float *q = (const float *)r.p + i * r.stride;
        x[0] = (double)q[0]; x[1] = (double)q[1]; x[2] = (double)q[2];
    }
}
__device__ __forceinline__ double row34(const double *m, const double x[3]) { return ((m[0] * x[0] + m[1] * x[1]) + m[2] * x[2]) + m[3]; }
__device__ __forceinline__ double sq3(const double a[3], const double b[3]) {
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return (dx * dx + dy * dy) + dz * dz;
}
// v = floor(x / size) per axis; false when one of them is outside [-2^20, 2^20) or NaN
__device__ __forceinline__ bool voxel_of(const double x[3], double size, int64_t v[3]) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double f = floor(x[k] / size);
        if (f >= -GRID_HALF && f < GRID_HALF) v[k] = (int64_t)f; else { v[k] = 0; ok = false; }
    }
    return ok;
}
__device__ __forceinline__ uint64_t key_of(int64_t vx, int64_t vy, int64_t vz) {
    return ((uint64_t)(vx + 1048576) << 42) | ((uint64_t)(vy + 1048576) << 21) | (uint64_t)(vz + 1048576);
}
__device__ __forceinline__ int64_t lower_bound(const uint64_t *__restrict__ keys, int64_t n, uint64_t key) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ int64_t dev_count(int64_t n, const int64_t *n_dev) {
    if (!n_dev) return n;
    const int64_t d = *n_dev;
    return d < 0 ? 0 : (d < n ? d : n);
}

// ---- down-sampling -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TB) void ds_key_kernel(int64_t N, const int64_t *n_dev, Rows rows, int ranged, double min_range, double max_range,
                                                    double size, uint64_t *__restrict__ keys, int32_t *__restrict__ vals,
                                                    int32_t *__restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= N) return;
    uint64_t key = SENTINEL;
    if (i < dev_count(N, n_dev)) {
        double x[3];
        load_row(rows, i, x);
        bool kept = true;
        if (ranged) {
            const double norm = sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
            kept = norm < max_range && norm > min_range;
        }
        if (kept) {
            int64_t v[3];
            if (voxel_of(x, size, v)) key = key_of(v[0], v[1], v[2]);
            else atomicOr(status, MTGS_ICP_OUT_OF_GRID);
        }
    }
    keys[i] = key;
    vals[i] = (int32_t)i;
}

__global__ __launch_bounds__(TB) void ds_flag_kernel(int64_t N, const uint64_t *__restrict__ keys_sorted, const int32_t *__restrict__ order,
                                                     int32_t *__restrict__ flag) {
    const int64_t j = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (j >= N) return;
    const uint64_t key = keys_sorted[j];
    const int32_t i = order[j];
    if (i >= 0 && i < N) flag[i] = (key != SENTINEL && (j == 0 || keys_sorted[j - 1] != key)) ? 1 : 0;
}

struct FlagValue {
    const int32_t *flag;
    int64_t n;
    __device__ int64_t operator()(int64_t i) const { return i < n ? flag[i] : 0; }
};
struct RowSink {                  // row i of `rows` -> row excl of out; its input index beside it
    Rows rows;
    const int32_t *index_in;      // NULL: i itself
    double *out;
    int32_t *index_out, *index_user;
    __device__ void operator()(int64_t i, int64_t excl, int64_t incl) const {
        if (incl == excl) return;
        double x[3];
        load_row(rows, i, x);
        out[excl * 3 + 0] = x[0]; out[excl * 3 + 1] = x[1]; out[excl * 3 + 2] = x[2];
        const int32_t id = index_in ? index_in[i] : (int32_t)i;
        if (index_out) index_out[excl] = id;
        if (index_user) index_user[excl] = id;
    }
};

// ---- the map -----------------------------------------------------------------------------------------------------------------------
struct Map {
    int64_t *state;
    uint64_t *keys[2];
    int32_t *slots[2];
    int32_t *cnt;
    double *pts;
    size_t bytes;
};
inline size_t al(size_t b) { return mtgs_sort::align256(b); }
Map carve_map(int64_t capacity, int maxp, void *base) {
    char *w = (char *)base;
    size_t o = 0;
    Map m;
    m.state = (int64_t *)(w + o); o += al(8 * sizeof(int64_t));
    for (int s = 0; s < 2; ++s) { m.keys[s] = (uint64_t *)(w + o); o += al((size_t)capacity * 8); }
    for (int s = 0; s < 2; ++s) { m.slots[s] = (int32_t *)(w + o); o += al((size_t)capacity * 4); }
    m.cnt = (int32_t *)(w + o); o += al((size_t)capacity * 4);
    m.pts = (double *)(w + o); o += al((size_t)capacity * maxp * 24);
    m.bytes = o;
    return m;
}
// the state words, clamped so that a damaged state cannot send an index outside the table
__device__ __forceinline__ int64_t map_voxels(const Map &m, int64_t capacity) {
    const int64_t n = m.state[ST_VOXELS];
    return n < 0 ? 0 : (n > capacity ? capacity : n);
}
__device__ __forceinline__ int map_side(const Map &m) { return (int)(m.state[ST_SIDE] & 1); }

__global__ __launch_bounds__(TB) void map_init_kernel(Map m, int64_t capacity) {
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i < 8) m.state[i] = 0;
    if (i < capacity) m.cnt[i] = 0;
}

__global__ __launch_bounds__(TB) void ins_key_kernel(Map m, int64_t M, const int64_t *m_dev, Rows rows, const double *__restrict__ pose,
                                                     double size, double *__restrict__ tp, uint64_t *__restrict__ keys,
                                                     int32_t *__restrict__ vals) {
    const int64_t j = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (j >= M) return;
    uint64_t key = SENTINEL;
    if (j < dev_count(M, m_dev)) {
        double x[3], y[3];
        load_row(rows, j, x);
        if (pose) {
#pragma unroll
            for (int k = 0; k < 3; ++k) y[k] = row34(pose + 4 * k, x);
        } else {
            y[0] = x[0]; y[1] = x[1]; y[2] = x[2];
        }
        tp[j * 3 + 0] = y[0]; tp[j * 3 + 1] = y[1]; tp[j * 3 + 2] = y[2];
        int64_t v[3];
        if (voxel_of(y, size, v)) key = key_of(v[0], v[1], v[2]);
        else atomicOr((unsigned long long *)&m.state[ST_STATUS], (unsigned long long)MTGS_ICP_OUT_OF_GRID);
    }
    keys[j] = key;
    vals[j] = (int32_t)j;
}

__device__ __forceinline__ bool is_head(const uint64_t *__restrict__ keys_sorted, int64_t j) {
    const uint64_t key = keys_sorted[j];
    return key != SENTINEL && (j == 0 || keys_sorted[j - 1] != key);
}
struct NewValue {                // 1 for the head of a run whose voxel is not in the table
    Map m;
    int64_t capacity, M;
    const uint64_t *keys_sorted;
    __device__ int64_t operator()(int64_t j) const {
        if (j >= M || !is_head(keys_sorted, j)) return 0;
        const int64_t n = map_voxels(m, capacity);
        const uint64_t *tk = m.keys[map_side(m)];
        const uint64_t key = keys_sorted[j];
        const int64_t at = lower_bound(tk, n, key);
        return (at < n && tk[at] == key) ? 0 : 1;
    }
};
struct NewSink {
    const uint64_t *keys_sorted;
    uint64_t *new_keys;
    __device__ void operator()(int64_t j, int64_t excl, int64_t incl) const {
        if (incl != excl) new_keys[excl] = keys_sorted[j];
    }
};
// the new voxels that go in: *n_new, or -1 when they do not fit
__device__ __forceinline__ int64_t accepted(const Map &m, int64_t capacity, int64_t M, const int64_t *n_new) {
    const int64_t u = *n_new;
    if (u < 0 || u > M || map_voxels(m, capacity) + u > capacity) return -1;
    return u;
}

__global__ __launch_bounds__(TB) void merge_old_kernel(Map m, int64_t capacity, int64_t M, const uint64_t *__restrict__ new_keys,
                                                       const int64_t *__restrict__ n_new) {
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    const int64_t u = accepted(m, capacity, M, n_new), n = map_voxels(m, capacity);
    if (u < 0 || i >= n) return;
    const int side = map_side(m);
    const uint64_t key = m.keys[side][i];
    const int64_t pos = i + lower_bound(new_keys, u, key);
    if (pos >= capacity) return;
    m.keys[side ^ 1][pos] = key;
    m.slots[side ^ 1][pos] = m.slots[side][i];
}
__global__ __launch_bounds__(TB) void merge_new_kernel(Map m, int64_t capacity, int64_t M, const uint64_t *__restrict__ new_keys,
                                                       const int64_t *__restrict__ n_new) {
    const int64_t r = (int64_t)blockIdx.x * TB + threadIdx.x;
    const int64_t u = accepted(m, capacity, M, n_new), n = map_voxels(m, capacity);
    if (u < 0 || r >= u) return;
    const int side = map_side(m);
    const uint64_t key = new_keys[r];
    const int64_t pos = r + lower_bound(m.keys[side], n, key);
    if (pos >= capacity || n + r >= capacity) return;
    m.keys[side ^ 1][pos] = key;
    m.slots[side ^ 1][pos] = (int32_t)(n + r);
    m.cnt[n + r] = 0;
}

// one lane per touched voxel: its run of the sorted offers, in offered order
__global__ __launch_bounds__(TB) void insert_kernel(Map m, int64_t capacity, int maxp, double resolution, int64_t M,
                                                    const uint64_t *__restrict__ keys_sorted, const int32_t *__restrict__ order,
                                                    const double *__restrict__ tp, const int64_t *__restrict__ n_new) {
    const int64_t j0 = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (j0 >= M) return;
    const int64_t u = accepted(m, capacity, M, n_new);
    if (u < 0 || !is_head(keys_sorted, j0)) return;
    const int64_t n = map_voxels(m, capacity) + u;
    const int side = map_side(m) ^ 1;
    const uint64_t key = keys_sorted[j0];
    const int64_t at = lower_bound(m.keys[side], n, key);
    if (at >= n || m.keys[side][at] != key) return;
    const int64_t slot = m.slots[side][at];
    if (slot < 0 || slot >= capacity) return;
    double *list = m.pts + slot * maxp * 3;
    int c = m.cnt[slot];
    c = c < 0 ? 0 : (c > maxp ? maxp : c);
    const int before = c;
    for (int64_t j = j0; j < M && keys_sorted[j] == key; ++j) {
        if (c == maxp) break;                                    // full: every later offer is dropped too
        const int64_t o = order[j];
        if (o < 0 || o >= M) continue;
        const double p[3] = {tp[o * 3 + 0], tp[o * 3 + 1], tp[o * 3 + 2]};
        bool close = false;
        for (int q = 0; q < c && !close; ++q) close = sqrt(sq3(list + q * 3, p)) < resolution;
        if (close) continue;
        list[c * 3 + 0] = p[0]; list[c * 3 + 1] = p[1]; list[c * 3 + 2] = p[2];
        ++c;
    }
    m.cnt[slot] = c;
    if (before == 0 && c > 0) atomicAdd((unsigned long long *)&m.state[ST_LIVE], 1ull);
}

__global__ void commit_kernel(Map m, int64_t capacity, int64_t M, const int64_t *__restrict__ n_new) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int64_t u = accepted(m, capacity, M, n_new);
    if (u < 0) {
        m.state[ST_STATUS] |= MTGS_ICP_MAP_FULL;
        return;
    }
    m.state[ST_VOXELS] = map_voxels(m, capacity) + u;
    m.state[ST_SIDE] = map_side(m) ^ 1;
}

__global__ __launch_bounds__(TB) void prune_kernel(Map m, int64_t capacity, int maxp, const double *__restrict__ origin, double max_d2) {
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= map_voxels(m, capacity)) return;
    const int64_t slot = m.slots[map_side(m)][i];
    if (slot < 0 || slot >= capacity || m.cnt[slot] <= 0) return;
    const double o[3] = {origin[0], origin[1], origin[2]};
    if (sq3(m.pts + slot * maxp * 3, o) >= max_d2) {
        m.cnt[slot] = 0;
        atomicAdd((unsigned long long *)&m.state[ST_LIVE], ~0ull);      // - 1
    }
}

struct ExportValue {
    Map m;
    int64_t capacity;
    int maxp;
    __device__ int64_t operator()(int64_t i) const {
        if (i >= map_voxels(m, capacity)) return 0;
        const int64_t slot = m.slots[map_side(m)][i];
        if (slot < 0 || slot >= capacity) return 0;
        const int c = m.cnt[slot];
        return c < 0 ? 0 : (c > maxp ? maxp : c);
    }
};
struct ExportSink {
    Map m;
    int maxp;
    int64_t rows;
    double *out;
    __device__ void operator()(int64_t i, int64_t excl, int64_t incl) const {
        if (incl == excl || incl > rows) return;
        const double *list = m.pts + (int64_t)m.slots[map_side(m)][i] * maxp * 3;
        for (int64_t q = 0; q < (incl - excl) * 3; ++q) out[excl * 3 + q] = list[q];
    }
};

// ---- one iteration -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TB) void begin_kernel(int64_t S, const int64_t *s_dev, Rows rows, const double *__restrict__ guess,
                                                   double *__restrict__ src, double *__restrict__ record) {
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i < MTGS_ICP_RECORD) {
        const bool one = i == 0 || i == 5 || i == 10 || i == 12 || i == 17 || i == 22;      // T_icp and the increment: identity
        record[i] = one ? 1.0 : 0.0;
    }
    if (i >= dev_count(S, s_dev)) return;
    double x[3];
    load_row(rows, i, x);
#pragma unroll
    for (int k = 0; k < 3; ++k) src[i * 3 + k] = row34(guess + 4 * k, x);
}

// the fixed tree of block_tree_sum_f64 (block_reduce.hpp) over NCOL columns at once: one barrier per level, not NCOL
__device__ __forceinline__ void tree_sum_columns(double (*lds)[TB]) {
    __syncthreads();
    for (int o = TB / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
#pragma unroll
            for (int c = 0; c < NCOL; ++c) lds[c][threadIdx.x] += lds[c][threadIdx.x + o];
        }
        __syncthreads();
    }
}

template <bool LOOP>
__global__ __launch_bounds__(TB) void associate_kernel(Map m, int64_t capacity, int maxp, double vsize, int64_t S, const int64_t *s_dev,
                                                       double *__restrict__ src, Rows rows, double max_distance, double kscale,
                                                       double *__restrict__ record, double *__restrict__ part,
                                                       int32_t *__restrict__ nn_index, double *__restrict__ distance,
                                                       uint8_t *__restrict__ mask) {
    __shared__ double lds[NCOL][TB];
    if (LOOP) {
        if (record[27] != 0.0) return;
        if (m.state[ST_LIVE] <= 0) {          // every block sees it; the finish launch stops on the status
            if (blockIdx.x == 0 && threadIdx.x == 0) record[27] = (double)MTGS_ICP_EMPTY_MAP;
            return;
        }
    }
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    const bool live = i < dev_count(S, s_dev);
    double v[NCOL];
#pragma unroll
    for (int c = 0; c < NCOL; ++c) v[c] = 0.0;
    if (live) {
        double p[3];
        if (LOOP) {
            const double x[3] = {src[i * 3 + 0], src[i * 3 + 1], src[i * 3 + 2]};
#pragma unroll
            for (int k = 0; k < 3; ++k) p[k] = row34(record + 12 + 4 * k, x);
            src[i * 3 + 0] = p[0]; src[i * 3 + 1] = p[1]; src[i * 3 + 2] = p[2];
        } else {
            load_row(rows, i, p);
        }
        double best = DBL_MAX, best2 = INFINITY, q[3] = {0.0, 0.0, 0.0};
        int best_at = -1;
        int64_t vox[3];
        if (voxel_of(p, vsize, vox)) {
            const int64_t n = map_voxels(m, capacity);
            const int side = map_side(m);
            const uint64_t *tk = m.keys[side];
            for (int a = 0; a < 27; ++a) {
                const int64_t vx = vox[0] + a / 9 - 1, vy = vox[1] + (a / 3) % 3 - 1, vz = vox[2] + a % 3 - 1;
                if (vx < -1048576 || vx >= 1048576 || vy < -1048576 || vy >= 1048576 || vz < -1048576 || vz >= 1048576) continue;
                const uint64_t key = key_of(vx, vy, vz);
                const int64_t at = lower_bound(tk, n, key);
                if (at >= n || tk[at] != key) continue;
                const int64_t slot = m.slots[side][at];
                if (slot < 0 || slot >= capacity) continue;
                int c = m.cnt[slot];
                c = c > maxp ? maxp : c;
                const double *list = m.pts + slot * maxp * 3;
                for (int e = 0; e < c; ++e) {
                    const double d2 = sq3(list + e * 3, p);
                    if (!(d2 < best2)) continue;             // sqrt is monotonic: no smaller square, no smaller distance
                    const double d = sqrt(d2);
                    if (d < best) {
                        best = d; best2 = d2; best_at = a * 32 + e;
                        q[0] = list[e * 3 + 0]; q[1] = list[e * 3 + 1]; q[2] = list[e * 3 + 2];
                    }
                }
            }
        }
        const bool hit = best_at >= 0 && best < max_distance;
        if (!LOOP) {
            if (nn_index) nn_index[i] = best_at;
            if (distance) distance[i] = best;
            if (mask) mask[i] = hit ? 1 : 0;
        }
        if (hit) {
            const double rx = p[0] - q[0], ry = p[1] - q[1], rz = p[2] - q[2];
            const double r2 = (rx * rx + ry * ry) + rz * rz;
            const double w = (kscale * kscale) / ((kscale + r2) * (kscale + r2));
            const double ux = w * rx, uy = w * ry, uz = w * rz;
            const double sx = p[0], sy = p[1], sz = p[2];
            v[0] = w; v[1] = w; v[2] = w;
            v[3] = w * sz; v[4] = -(w * sy); v[5] = -(w * sz); v[6] = w * sx; v[7] = w * sy; v[8] = -(w * sx);
            v[9] = w * (sy * sy + sz * sz); v[10] = -(w * (sx * sy)); v[11] = -(w * (sx * sz));
            v[12] = w * (sx * sx + sz * sz); v[13] = -(w * (sy * sz)); v[14] = w * (sx * sx + sy * sy);
            v[15] = ux; v[16] = uy; v[17] = uz;
            v[18] = sy * uz - sz * uy; v[19] = sz * ux - sx * uz; v[20] = sx * uy - sy * ux;
            v[21] = 1.0;
        }
    }
#pragma unroll
    for (int c = 0; c < NCOL; ++c) lds[c][threadIdx.x] = v[c];
    tree_sum_columns(lds);
    if (threadIdx.x < NCOL) part[(int64_t)blockIdx.x * NCOL + threadIdx.x] = lds[threadIdx.x][0];
}

// dx of A dx = b by the header's LDL^T (A symmetric 6 x 6, its lower triangle read)
__device__ void ldlt_solve(const double A[6][6], const double b[6], double x[6]) {
    double L[6][6], d[6], y[6];
    for (int j = 0; j < 6; ++j) {
        double s = A[j][j];
        for (int k = 0; k < j; ++k) s = s - L[j][k] * (L[j][k] * d[k]);
        d[j] = s;
        for (int i = j + 1; i < 6; ++i) {
            double t = A[i][j];
            for (int k = 0; k < j; ++k) t = t - L[i][k] * (L[j][k] * d[k]);
            L[i][j] = t / d[j];
        }
    }
    for (int i = 0; i < 6; ++i) {
        double s = b[i];
        for (int k = 0; k < i; ++k) s = s - L[i][k] * y[k];
        y[i] = s;
    }
    for (int i = 5; i >= 0; --i) {
        double s = y[i] / d[i];
        for (int k = i + 1; k < 6; ++k) s = s - L[k][i] * x[k];
        x[i] = s;
    }
}

// E = SE3::exp(dx) as a 3 x 4 by rows, the header's closed form
__device__ void se3_exp(const double dx[6], double E[12]) {
    const double u[3] = {dx[0], dx[1], dx[2]}, o[3] = {dx[3], dx[4], dx[5]};
    const double t2 = (o[0] * o[0] + o[1] * o[1]) + o[2] * o[2];
    double A, B, C;
    if (t2 < 1e-8) {
        A = 1.0 - t2 / 6.0; B = 0.5 - t2 / 24.0; C = 1.0 / 6.0 - t2 / 120.0;
    } else {
        const double t = sqrt(t2), sn = sin(t), cs = cos(t);
        A = sn / t; B = (1.0 - cs) / t2; C = (t - sn) / (t2 * t);
    }
    const double W[3][3] = {{0.0, -o[2], o[1]}, {o[2], 0.0, -o[0]}, {-o[1], o[0], 0.0}};
    double V[3][3];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            const double W2 = o[a] * o[b] - (a == b ? t2 : 0.0), I = a == b ? 1.0 : 0.0;
            E[a * 4 + b] = I + (A * W[a][b] + B * W2);
            V[a][b] = I + (B * W[a][b] + C * W2);
        }
    for (int a = 0; a < 3; ++a) E[a * 4 + 3] = (V[a][0] * u[0] + V[a][1] * u[1]) + V[a][2] * u[2];
}

template <bool LOOP>
__global__ __launch_bounds__(TB) void finish_kernel(int64_t nblocks, const double *__restrict__ part, double convergence,
                                                    double *__restrict__ record, double *__restrict__ sums_out) {
    __shared__ double lds[NCOL][TB];
    if (LOOP && record[27] != 0.0) return;
    double acc[NCOL];
#pragma unroll
    for (int c = 0; c < NCOL; ++c) acc[c] = 0.0;
    for (int64_t b = threadIdx.x; b < nblocks; b += TB) {
#pragma unroll
        for (int c = 0; c < NCOL; ++c) acc[c] += part[b * NCOL + c];
    }
#pragma unroll
    for (int c = 0; c < NCOL; ++c) lds[c][threadIdx.x] = acc[c];
    tree_sum_columns(lds);
    if (threadIdx.x != 0) return;
    double s[MTGS_ICP_SUMS];
    for (int c = 0; c < MTGS_ICP_SUMS; ++c) s[c] = 0.0;
    for (int c = 0; c < 15; ++c) s[c] = lds[c][0];
    for (int c = 15; c < NCOL; ++c) s[c + 6] = lds[c][0];
    double *out = LOOP ? record + 28 : sums_out;
    for (int c = 0; c < MTGS_ICP_SUMS; ++c) out[c] = s[c];
    if (!LOOP) return;
    record[25] = record[25] + 1.0;
    record[26] = s[27];
    if (!(s[27] > 0.0)) {
        record[24] = 0.0;
        record[27] = (double)MTGS_ICP_DEGENERATE;
        return;
    }
    double A[6][6];
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b) A[a][b] = 0.0;
    A[0][0] = s[0]; A[1][1] = s[1]; A[2][2] = s[2];
    A[4][0] = s[3]; A[5][0] = s[4]; A[3][1] = s[5]; A[5][1] = s[6]; A[3][2] = s[7]; A[4][2] = s[8];
    A[3][3] = s[9]; A[4][3] = s[10]; A[5][3] = s[11]; A[4][4] = s[12]; A[5][4] = s[13]; A[5][5] = s[14];
    double b[6], dx[6];
    for (int a = 0; a < 6; ++a) b[a] = -s[21 + a];
    ldlt_solve(A, b, dx);
    double n2 = dx[0] * dx[0];
    bool finite = isfinite(dx[0]);
    for (int a = 1; a < 6; ++a) {
        n2 = n2 + dx[a] * dx[a];
        finite = finite && isfinite(dx[a]);
    }
    const double norm = sqrt(n2);
    record[24] = norm;
    if (!finite) {
        record[27] = (double)MTGS_ICP_DEGENERATE;
        return;
    }
    double E[12], T[12];
    se3_exp(dx, E);
    for (int a = 0; a < 3; ++a) {
        for (int c = 0; c < 4; ++c) {
            double e = (E[a * 4 + 0] * record[0 + c] + E[a * 4 + 1] * record[4 + c]) + E[a * 4 + 2] * record[8 + c];
            if (c == 3) e = e + E[a * 4 + 3];
            T[a * 4 + c] = e;
        }
    }
    for (int c = 0; c < 12; ++c) {
        record[c] = T[c];
        record[12 + c] = E[c];
    }
    if (norm < convergence) record[27] = (double)MTGS_ICP_CONVERGED;
}

// ---- workspaces ----------------------------------------------------------------------------------------------------------------------
struct DsWs {
    uint64_t *keys, *keys_sorted;
    int32_t *vals, *order, *flag, *index;
    int64_t *partials;
    void *sort_ws;
    size_t sort_bytes, bytes;
};
DsWs carve_ds(int64_t N, void *ws) {
    const int64_t n = N > 0 ? N : 1;
    char *w = (char *)ws;
    size_t o = 0;
    DsWs k;
    k.keys = (uint64_t *)(w + o); o += al(n * 8);
    k.keys_sorted = (uint64_t *)(w + o); o += al(n * 8);
    k.vals = (int32_t *)(w + o); o += al(n * 4);
    k.order = (int32_t *)(w + o); o += al(n * 4);
    k.flag = (int32_t *)(w + o); o += al(n * 4);
    k.index = (int32_t *)(w + o); o += al(n * 4);
    k.partials = (int64_t *)(w + o); o += al(mtgs_scan::workspace_bytes(n));
    k.sort_ws = w + o; k.sort_bytes = mtgs_sort::workspace_bytes<uint64_t>(n); o += al(k.sort_bytes);
    k.bytes = o;
    return k;
}

struct InsWs {
    uint64_t *keys, *keys_sorted, *new_keys;
    int32_t *vals, *order;
    double *tp;
    int64_t *partials, *n_new;
    void *sort_ws;
    size_t sort_bytes, bytes;
};
InsWs carve_ins(int64_t M, void *ws) {
    const int64_t n = M > 0 ? M : 1;
    char *w = (char *)ws;
    size_t o = 0;
    InsWs k;
    k.keys = (uint64_t *)(w + o); o += al(n * 8);
    k.keys_sorted = (uint64_t *)(w + o); o += al(n * 8);
    k.new_keys = (uint64_t *)(w + o); o += al(n * 8);
    k.vals = (int32_t *)(w + o); o += al(n * 4);
    k.order = (int32_t *)(w + o); o += al(n * 4);
    k.tp = (double *)(w + o); o += al(n * 24);
    k.partials = (int64_t *)(w + o); o += al(mtgs_scan::workspace_bytes(n));
    k.n_new = (int64_t *)(w + o); o += al(8);
    k.sort_ws = w + o; k.sort_bytes = mtgs_sort::workspace_bytes<uint64_t>(n); o += al(k.sort_bytes);
    k.bytes = o;
    return k;
}

struct AlignWs {
    double *src, *part;
    int64_t nblocks;
    size_t bytes;
};
AlignWs carve_align(int64_t S, void *ws) {
    const int64_t n = S > 0 ? S : 1;
    char *w = (char *)ws;
    size_t o = 0;
    AlignWs k;
    k.nblocks = ceil_div64(n, TB);
    k.src = (double *)(w + o); o += al(n * 24);
    k.part = (double *)(w + o); o += al((size_t)k.nblocks * NCOL * 8);
    k.bytes = o;
    return k;
}

#define ICP_WS(fn, ws, ws_bytes, need)                                                                             \
    do {                                                                                                            \
        MTGS_NONNULL(fn, ws);                                                                                       \
        MTGS_REQUIRE(((uintptr_t)(ws) & 15) == 0, MTGS_EINVAL, "%s: workspace must be 16-byte aligned", fn);         \
        MTGS_REQUIRE((ws_bytes) >= (need), MTGS_EWORKSPACE, "%s: workspace %zu < %zu bytes", fn, (size_t)(ws_bytes), (size_t)(need)); \
    } while (0)

int check_map(const char *fn, const void *map, int64_t capacity, int max_points) {
    MTGS_NONNULL(fn, map);
    MTGS_REQUIRE(((uintptr_t)map & 15) == 0, MTGS_EINVAL, "%s: map must be 16-byte aligned", fn);
    MTGS_REQUIRE(capacity >= 1 && capacity < ((int64_t)1 << 31), MTGS_EINVAL, "%s: capacity outside [1, 2^31) (%lld)", fn, (long long)capacity);
    MTGS_REQUIRE(max_points >= 1 && max_points <= MTGS_ICP_MAX_POINTS, MTGS_EINVAL, "%s: max_points outside [1, %d] (%d)", fn,
                 MTGS_ICP_MAX_POINTS, max_points);
    return MTGS_OK;
}
int check_rows(const char *fn, int64_t n, const void *points, int64_t row_stride) {
    MTGS_COUNT31(fn, n);
    if (n > 0) {
        MTGS_NONNULL(fn, points);
        MTGS_REQUIRE(row_stride >= 3, MTGS_EINVAL, "%s: row_stride < 3 (%lld)", fn, (long long)row_stride);
    }
    return MTGS_OK;
}
#define ICP_POSITIVE(fn, x) MTGS_REQUIRE((x) > 0.0 && (x) < INFINITY, MTGS_EINVAL, "%s: %s must be positive and finite (%g)", fn, #x, (double)(x))

}  // namespace

extern "C" int mtgs_icp_downsample_workspace_bytes(int64_t N, size_t *bytes) {
    const char *fn = "mtgs_icp_downsample_workspace_bytes";
    MTGS_COUNT31(fn, N);
    MTGS_NONNULL(fn, bytes);
    *bytes = carve_ds(N, nullptr).bytes;
    return MTGS_OK;
}

extern "C" int mtgs_icp_downsample(int64_t N, const void *points, int points_f64, int64_t row_stride, double min_range, double max_range,
                                   double voxel_size, double *frame, double *source, int32_t *frame_index, int32_t *source_index,
                                   int64_t *counts, int32_t *status, void *ws, size_t ws_bytes, void *stream) {
    const char *fn = "mtgs_icp_downsample";
    int rc = check_rows(fn, N, points, row_stride);
    if (rc != MTGS_OK) return rc;
    ICP_POSITIVE(fn, voxel_size);
    MTGS_REQUIRE(min_range == min_range && max_range == max_range, MTGS_EINVAL, "%s: a range is NaN", fn);
    MTGS_NONNULL(fn, counts); MTGS_NONNULL(fn, status);
    MTGS_REQUIRE(((uintptr_t)counts & 7) == 0, MTGS_EINVAL, "%s: counts must be 8-byte aligned", fn);
    const DsWs k = carve_ds(N, ws);
    ICP_WS(fn, ws, ws_bytes, k.bytes);
    hipStream_t st = (hipStream_t)stream;
    rc = mtgs_zero_async(status, sizeof(int32_t), st);
    if (rc != MTGS_OK) return rc;
    if (N == 0) return mtgs_zero_async(counts, 2 * sizeof(int64_t), st);
    MTGS_NONNULL(fn, frame); MTGS_NONNULL(fn, source);
    const unsigned blocks = (unsigned)ceil_div64(N, TB);
    const Rows in{points, points_f64, row_stride}, mid{frame, 1, 3};
    for (int level = 0; level < 2; ++level) {
        const double size = (level == 0 ? 0.5 : 1.5) * voxel_size;
        ds_key_kernel<<<blocks, TB, 0, st>>>(N, level == 0 ? nullptr : counts, level == 0 ? in : mid, level == 0, min_range, max_range, size,
                                             k.keys, k.vals, status);
        MTGS_CHECK_LAUNCH(fn);
        rc = mtgs_sort::sort_pairs<uint64_t>(N, 64, k.keys, k.vals, k.keys_sorted, k.order, k.sort_ws, k.sort_bytes, st, fn);
        if (rc != MTGS_OK) return rc;
        ds_flag_kernel<<<blocks, TB, 0, st>>>(N, k.keys_sorted, k.order, k.flag);
        if (level == 0)
            mtgs_scan::run(N, FlagValue{k.flag, N}, RowSink{in, nullptr, frame, k.index, frame_index}, k.partials, counts, st);
        else
            mtgs_scan::run(N, FlagValue{k.flag, N}, RowSink{mid, k.index, source, nullptr, source_index}, k.partials, counts + 1, st);
        MTGS_CHECK_LAUNCH(fn);
    }
    return MTGS_OK;
}

extern "C" int mtgs_icp_map_bytes(int64_t capacity, int max_points, size_t *bytes) {
    const char *fn = "mtgs_icp_map_bytes";
    MTGS_REQUIRE(capacity >= 1 && capacity < ((int64_t)1 << 31), MTGS_EINVAL, "%s: capacity outside [1, 2^31) (%lld)", fn, (long long)capacity);
    MTGS_REQUIRE(max_points >= 1 && max_points <= MTGS_ICP_MAX_POINTS, MTGS_EINVAL, "%s: max_points outside [1, %d] (%d)", fn,
                 MTGS_ICP_MAX_POINTS, max_points);
    MTGS_NONNULL(fn, bytes);
    *bytes = carve_map(capacity, max_points, nullptr).bytes;
    return MTGS_OK;
}

extern "C" int mtgs_icp_map_init(void *map, size_t map_bytes, int64_t capacity, int max_points, void *stream) {
    const char *fn = "mtgs_icp_map_init";
    const int rc = check_map(fn, map, capacity, max_points);
    if (rc != MTGS_OK) return rc;
    const Map m = carve_map(capacity, max_points, map);
    MTGS_REQUIRE(map_bytes >= m.bytes, MTGS_EWORKSPACE, "%s: map %zu < %zu bytes", fn, map_bytes, m.bytes);
    map_init_kernel<<<(unsigned)ceil_div64(capacity < 8 ? 8 : capacity, TB), TB, 0, (hipStream_t)stream>>>(m, capacity);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}

extern "C" int mtgs_icp_map_insert_workspace_bytes(int64_t M, size_t *bytes) {
    const char *fn = "mtgs_icp_map_insert_workspace_bytes";
    MTGS_COUNT31(fn, M);
    MTGS_NONNULL(fn, bytes);
    *bytes = carve_ins(M, nullptr).bytes;
    return MTGS_OK;
}

extern "C" int mtgs_icp_map_insert(void *map, int64_t capacity, int max_points, double voxel_size, int64_t M, const void *points,
                                   int points_f64, int64_t row_stride, const int64_t *m_dev, const double *pose, void *ws, size_t ws_bytes,
                                   void *stream) {
    const char *fn = "mtgs_icp_map_insert";
    int rc = check_map(fn, map, capacity, max_points);
    if (rc != MTGS_OK) return rc;
    rc = check_rows(fn, M, points, row_stride);
    if (rc != MTGS_OK) return rc;
    ICP_POSITIVE(fn, voxel_size);
    const InsWs k = carve_ins(M, ws);
    ICP_WS(fn, ws, ws_bytes, k.bytes);
    if (M == 0) return MTGS_OK;
    const Map m = carve_map(capacity, max_points, map);
    hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = (unsigned)ceil_div64(M, TB);
    ins_key_kernel<<<blocks, TB, 0, st>>>(m, M, m_dev, Rows{points, points_f64, row_stride}, pose, voxel_size, k.tp, k.keys, k.vals);
    MTGS_CHECK_LAUNCH(fn);
    rc = mtgs_sort::sort_pairs<uint64_t>(M, 64, k.keys, k.vals, k.keys_sorted, k.order, k.sort_ws, k.sort_bytes, st, fn);
    if (rc != MTGS_OK) return rc;
    mtgs_scan::run(M, NewValue{m, capacity, M, k.keys_sorted}, NewSink{k.keys_sorted, k.new_keys}, k.partials, k.n_new, st);
    merge_old_kernel<<<(unsigned)ceil_div64(capacity, TB), TB, 0, st>>>(m, capacity, M, k.new_keys, k.n_new);
    merge_new_kernel<<<blocks, TB, 0, st>>>(m, capacity, M, k.new_keys, k.n_new);
    const double resolution = sqrt(voxel_size * voxel_size / (double)max_points);
    insert_kernel<<<blocks, TB, 0, st>>>(m, capacity, max_points, resolution, M, k.keys_sorted, k.order, k.tp, k.n_new);
    commit_kernel<<<1, 64, 0, st>>>(m, capacity, M, k.n_new);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}

extern "C" int mtgs_icp_map_prune(void *map, int64_t capacity, int max_points, const double *origin, double max_distance, void *stream) {
    const char *fn = "mtgs_icp_map_prune";
    const int rc = check_map(fn, map, capacity, max_points);
    if (rc != MTGS_OK) return rc;
    MTGS_NONNULL(fn, origin);
    MTGS_REQUIRE(max_distance == max_distance, MTGS_EINVAL, "%s: max_distance is NaN", fn);
    const Map m = carve_map(capacity, max_points, map);
    prune_kernel<<<(unsigned)ceil_div64(capacity, TB), TB, 0, (hipStream_t)stream>>>(m, capacity, max_points, origin, max_distance * max_distance);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}

extern "C" int mtgs_icp_map_export_workspace_bytes(int64_t capacity, size_t *bytes) {
    const char *fn = "mtgs_icp_map_export_workspace_bytes";
    MTGS_REQUIRE(capacity >= 1 && capacity < ((int64_t)1 << 31), MTGS_EINVAL, "%s: capacity outside [1, 2^31) (%lld)", fn, (long long)capacity);
    MTGS_NONNULL(fn, bytes);
    *bytes = al(mtgs_scan::workspace_bytes(capacity));
    return MTGS_OK;
}

extern "C" int mtgs_icp_map_export(const void *map, int64_t capacity, int max_points, int64_t rows, double *out, int64_t *total, void *ws,
                                   size_t ws_bytes, void *stream) {
    const char *fn = "mtgs_icp_map_export";
    const int rc = check_map(fn, map, capacity, max_points);
    if (rc != MTGS_OK) return rc;
    MTGS_REQUIRE(rows >= 0, MTGS_EINVAL, "%s: rows < 0 (%lld)", fn, (long long)rows);
    if (rows > 0) MTGS_NONNULL(fn, out);
    MTGS_NONNULL(fn, total);
    MTGS_REQUIRE(((uintptr_t)total & 7) == 0, MTGS_EINVAL, "%s: total must be 8-byte aligned", fn);
    ICP_WS(fn, ws, ws_bytes, al(mtgs_scan::workspace_bytes(capacity)));
    const Map m = carve_map(capacity, max_points, const_cast<void *>(map));
    mtgs_scan::run(capacity, ExportValue{m, capacity, max_points}, ExportSink{m, max_points, rows, out}, (int64_t *)ws, total, (hipStream_t)stream);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}

extern "C" int mtgs_icp_align_workspace_bytes(int64_t S, size_t *bytes) {
    const char *fn = "mtgs_icp_align_workspace_bytes";
    MTGS_COUNT31(fn, S);
    MTGS_NONNULL(fn, bytes);
    *bytes = carve_align(S, nullptr).bytes;
    return MTGS_OK;
}

extern "C" int mtgs_icp_align_begin(int64_t S, const void *source, int source_f64, int64_t row_stride, const int64_t *s_dev,
                                    const double *guess, double *record, void *ws, size_t ws_bytes, void *stream) {
    const char *fn = "mtgs_icp_align_begin";
    const int rc = check_rows(fn, S, source, row_stride);
    if (rc != MTGS_OK) return rc;
    MTGS_NONNULL(fn, guess); MTGS_NONNULL(fn, record);
    const AlignWs k = carve_align(S, ws);
    ICP_WS(fn, ws, ws_bytes, k.bytes);
    begin_kernel<<<(unsigned)k.nblocks, TB, 0, (hipStream_t)stream>>>(S, s_dev, Rows{source, source_f64, row_stride}, guess, k.src, record);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}

extern "C" int mtgs_icp_align_iterate(const void *map, int64_t capacity, int max_points, double voxel_size, int64_t S, const int64_t *s_dev,
                                      double max_distance, double kernel_scale, double convergence, int iterations, double *record,
                                      void *ws, size_t ws_bytes, void *stream) {
    const char *fn = "mtgs_icp_align_iterate";
    const int rc = check_map(fn, map, capacity, max_points);
    if (rc != MTGS_OK) return rc;
    MTGS_COUNT31(fn, S);
    ICP_POSITIVE(fn, voxel_size);
    MTGS_REQUIRE(iterations >= 0 && iterations <= 4096, MTGS_EINVAL, "%s: iterations outside [0, 4096] (%d)", fn, iterations);
    MTGS_NONNULL(fn, record);
    const AlignWs k = carve_align(S, ws);
    ICP_WS(fn, ws, ws_bytes, k.bytes);
    const Map m = carve_map(capacity, max_points, const_cast<void *>(map));
    hipStream_t st = (hipStream_t)stream;
    for (int it = 0; it < iterations; ++it) {
        associate_kernel<true><<<(unsigned)k.nblocks, TB, 0, st>>>(m, capacity, max_points, voxel_size, S, s_dev, k.src, Rows{nullptr, 1, 3},
                                                                    max_distance, kernel_scale, record, k.part, nullptr, nullptr, nullptr);
        finish_kernel<true><<<1, TB, 0, st>>>(k.nblocks, k.part, convergence, record, nullptr);
    }
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}

extern "C" int mtgs_icp_associate(const void *map, int64_t capacity, int max_points, double voxel_size, int64_t S, const void *source,
                                  int source_f64, int64_t row_stride, double max_distance, double kernel_scale, int32_t *nn_index,
                                  double *distance, uint8_t *mask, double *sums, void *ws, size_t ws_bytes, void *stream) {
    const char *fn = "mtgs_icp_associate";
    int rc = check_map(fn, map, capacity, max_points);
    if (rc != MTGS_OK) return rc;
    rc = check_rows(fn, S, source, row_stride);
    if (rc != MTGS_OK) return rc;
    ICP_POSITIVE(fn, voxel_size);
    MTGS_NONNULL(fn, sums);
    const AlignWs k = carve_align(S, ws);
    ICP_WS(fn, ws, ws_bytes, k.bytes);
    const Map m = carve_map(capacity, max_points, const_cast<void *>(map));
    hipStream_t st = (hipStream_t)stream;
    associate_kernel<false><<<(unsigned)k.nblocks, TB, 0, st>>>(m, capacity, max_points, voxel_size, S, nullptr, nullptr,
                                                                 Rows{source, source_f64, row_stride}, max_distance, kernel_scale, nullptr,
                                                                 k.part, nn_index, distance, mask);
    finish_kernel<false><<<1, TB, 0, st>>>(k.nblocks, k.part, 0.0, nullptr, sums);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}
