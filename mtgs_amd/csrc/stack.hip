// stack.hip -- lidar sweeps stacked into a background cloud and one cloud per tracked object (include/mtgs_stack.h states the rule
// and the arithmetic; mtgs_amd.stack): extract_frame_background_instance_lidar and accumulate_background_box_point
// (nuplan_scripts/utils/stack_point_cloud_utils.py) with the per-frame painting and filtering of StackRGBPointCloud
// (nuplan_scripts/stack_RGB_point_cloud.py:89-126, 153-183).
//
// mtgs_stack_split, one call =
//   classify_kernel        one lane per point; the box table (3 x 4 matrix, tight and inflated half sizes, include) staged through LDS
//                          CHUNK boxes at a time; the loop over the boxes is wave-uniform, a lane that has its owner idles; a
//                          workgroup whose lanes all have one stops.  Writes slot, the sort key (dropped = B + 1) and q of an
//                          instance point.
//   mtgs_sort::sort_pairs  stable u32 radix sort of (key, index) on the bits of B + 1: the reference's order of `all_points`
//   offsets_kernel         one thread per group: the lower bound of its key in the sorted keys
//   rows_kernel            one thread per sorted row: the background row as fp64, the box-frame row, zeros past the kept rows; for a
//                          frame also the row to paint (an instance row back through box2lidar)
// mtgs_stack_frame = the above, mtgs_lidar_paint (lidar.hip, unchanged), then
//   mtgs_scan::run         fov of the kept rows as the scanned value; the sink moves a seen row to its place and keeps every row's
//                          exclusive prefix, from which offsets2_kernel reads the new group offsets
//   mtgs_scan::run         label < cutoff over the compacted background: bg_sel and bg_kept for the traversal
// mtgs_stack_plan   = mtgs_scan::run over the (frame, slot) counts in output order
// mtgs_stack_gather = gather_kernel, one launch: a workgroup finds the segment of its first row by binary search in the prefix (as
//                     refine_scene_rows_kernel finds its move) and each lane walks on to its own.
// No atomics on global memory, no allocation, no host read.  Compiled with -ffp-contract=off: the NumPy restatement of
// tests/stack_refs.py is compared bit for bit.
#include "common.hpp"
#include "radix_sort.hpp"
#include "scan.hpp"

namespace {

constexpr int TB = 256;
constexpr int CHUNK = MTGS_STACK_BOX_CHUNK;
constexpr int BOX_ROW = 20;      // 12 matrix, 3 tight, 3 inflated, include, pad

template <class T>
__device__ __forceinline__ void load_point(const T *__restrict__ points, int64_t stride, int64_t i, double x[3]) {
    const T *p = points + i * stride;
    x[0] = (double)p[0];
    x[1] = (double)p[1];
    x[2] = (double)p[2];
}

__device__ __forceinline__ double row34(const double *m, const double x[3]) { return ((m[0] * x[0] + m[1] * x[1]) + m[2] * x[2]) + m[3]; }

template <class T>
__global__ __launch_bounds__(TB) void classify_kernel(int32_t N, const T *__restrict__ points, int64_t stride, int B,
                                                      const double *__restrict__ lidar2box, const double *__restrict__ half_tight,
                                                      const double *__restrict__ half_inflated, const uint8_t *__restrict__ include,
                                                      uint32_t *__restrict__ keys, int32_t *__restrict__ vals,
                                                      int32_t *__restrict__ slot, double *__restrict__ qbuf) {
    __shared__ double s_box[CHUNK * BOX_ROW];
    const int64_t t = (int64_t)blockIdx.x * TB + threadIdx.x;
    const bool live = t < N;
    double x[3] = {0.0, 0.0, 0.0}, q[3] = {0.0, 0.0, 0.0};
    if (live) load_point(points, stride, t, x);
    int32_t mine = 0;
    bool done = !live;
    for (int b0 = 0; b0 < B; b0 += CHUNK) {
        if (__syncthreads_and(done)) break;                // also: the chunk before this one has been consumed
        const int nb = min(CHUNK, B - b0);
        for (int k = threadIdx.x; k < nb * BOX_ROW; k += TB) {
            const int b = b0 + k / BOX_ROW, c = k % BOX_ROW;
            double v = 0.0;
            if (c < 12) v = lidar2box[b * 12 + c];
            else if (c < 15) v = half_tight[b * 3 + (c - 12)];
            else if (c < 18) v = half_inflated[b * 3 + (c - 15)];
            else if (c == 18) v = include ? (include[b] ? 1.0 : 0.0) : 1.0;
            s_box[k] = v;
        }
        __syncthreads();
        for (int b = 0; b < nb; ++b) {                     // wave-uniform
            const double *r = s_box + b * BOX_ROW;
            if (r[18] == 0.0 || done) continue;
            const double q0 = row34(r, x), q1 = row34(r + 4, x), q2 = row34(r + 8, x);
            const double a0 = fabs(q0), a1 = fabs(q1), a2 = fabs(q2);
            if (a0 <= r[15] && a1 <= r[16] && a2 <= r[17]) {        // false on NaN
                done = true;
                if (a0 <= r[12] && a1 <= r[13] && a2 <= r[14]) {
                    mine = 1 + b0 + b;
                    q[0] = q0; q[1] = q1; q[2] = q2;
                } else {
                    mine = -1;
                }
            }
        }
    }
    if (!live) return;
    if (slot) slot[t] = mine;
    keys[t] = mine < 0 ? (uint32_t)(B + 1) : (uint32_t)mine;
    vals[t] = (int32_t)t;
    if (mine > 0) {
        qbuf[t * 3 + 0] = q[0];
        qbuf[t * 3 + 1] = q[1];
        qbuf[t * 3 + 2] = q[2];
    }
}

// offsets[g] = the number of sorted keys below g, g in [0, B + 2)
__global__ __launch_bounds__(TB) void offsets_kernel(int32_t N, int B, const uint32_t *__restrict__ keys_sorted, int64_t *__restrict__ offsets) {
    const int g = blockIdx.x * TB + threadIdx.x;
    if (g >= B + 2) return;
    int32_t lo = 0, hi = N;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (keys_sorted[mid] < (uint32_t)g) lo = mid + 1; else hi = mid;
    }
    offsets[g] = lo;
}

template <class T>
__global__ __launch_bounds__(TB) void rows_kernel(int32_t N, const T *__restrict__ points, int64_t stride, int B,
                                                  const uint32_t *__restrict__ keys_sorted, const int32_t *__restrict__ order,
                                                  const double *__restrict__ qbuf, const double *__restrict__ box2lidar,
                                                  double *__restrict__ rows, double *__restrict__ paint) {
    const int64_t j = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (j >= N) return;
    const uint32_t key = keys_sorted[j];
    const int32_t i = order[j];
    double r[3] = {0.0, 0.0, 0.0}, e[3] = {0.0, 0.0, 0.0};
    if (i >= 0 && i < N) {
        if (key == 0) {
            load_point(points, stride, i, r);
            e[0] = r[0]; e[1] = r[1]; e[2] = r[2];
        } else if (key <= (uint32_t)B) {
            r[0] = qbuf[(int64_t)i * 3 + 0]; r[1] = qbuf[(int64_t)i * 3 + 1]; r[2] = qbuf[(int64_t)i * 3 + 2];
            if (paint) {
                const double *m = box2lidar + (int64_t)(key - 1) * 12;
#pragma unroll
                for (int k = 0; k < 3; ++k) e[k] = row34(m + 4 * k, r);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        rows[j * 3 + k] = r[k];
        if (paint) paint[j * 3 + k] = e[k];
    }
}

// the rows some camera sees, of the kept ones; element n (one past the rows) counts nothing and receives the total
struct FovValue {
    const uint8_t *fov;
    const int64_t *offsets;
    int B;
    int64_t n;
    __device__ int64_t operator()(int64_t j) const { return (j < n && j < offsets[B + 1] && fov[j]) ? 1 : 0; }
};
struct FovSink {
    int32_t *pre;
    const double *rows, *rgb;
    const int32_t *labels;
    double *out_points, *out_rgb;
    int32_t *out_labels;
    __device__ void operator()(int64_t j, int64_t excl, int64_t incl) const {
        pre[j] = (int32_t)excl;
        if (incl == excl) return;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            out_points[excl * 3 + k] = rows[j * 3 + k];
            out_rgb[excl * 3 + k] = rgb[j * 3 + k];
        }
        out_labels[excl] = labels[j];
    }
};
__global__ __launch_bounds__(TB) void offsets2_kernel(int32_t N, int B, const int64_t *__restrict__ offsets, const int32_t *__restrict__ pre,
                                                      int64_t *__restrict__ out_offsets) {
    const int g = blockIdx.x * TB + threadIdx.x;
    if (g >= B + 2) return;
    const int64_t o = offsets[g];
    out_offsets[g] = pre[o < 0 ? 0 : (o > N ? N : o)];
}

struct LabelValue {
    const int32_t *labels;
    const int64_t *out_offsets;
    int cutoff;
    int64_t n;
    __device__ int64_t operator()(int64_t j) const { return (j < n && j < out_offsets[1] && labels[j] < cutoff) ? 1 : 0; }
};
struct LabelSink {
    int32_t *bg_sel;
    __device__ void operator()(int64_t j, int64_t excl, int64_t incl) const {
        if (incl != excl) bg_sel[excl] = (int32_t)j;
    }
};

// ---- the traversal -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t segment_count(const int32_t *seg_frame, const int32_t *seg_slot, int64_t F, const mtgs_stack_frame_desc *frames,
                                                 int64_t s) {
    const int64_t f = seg_frame[s], slot = seg_slot[s];
    if (f < 0 || f >= F) return 0;
    const mtgs_stack_frame_desc &d = frames[f];
    if (slot < 0 || slot >= d.groups) return 0;
    const int64_t c = slot == 0 ? *d.bg_kept : d.offsets[slot + 1] - d.offsets[slot];
    return c > 0 ? c : 0;
}
struct CountValue {
    const int32_t *seg_frame, *seg_slot;
    int64_t F;
    const mtgs_stack_frame_desc *frames;
    int64_t S;
    __device__ int64_t operator()(int64_t s) const { return s < S ? segment_count(seg_frame, seg_slot, F, frames, s) : 0; }
};
struct PrefixSink {
    int64_t *prefix;
    __device__ void operator()(int64_t s, int64_t excl, int64_t) const { prefix[s] = excl; }
};

__global__ __launch_bounds__(TB) void gather_kernel(int32_t S, const int32_t *__restrict__ seg_frame, const int32_t *__restrict__ seg_slot,
                                                    int64_t F, const mtgs_stack_frame_desc *__restrict__ frames,
                                                    const int64_t *__restrict__ prefix, int64_t total, double *__restrict__ xyz,
                                                    double *__restrict__ rgb, int32_t *__restrict__ labels) {
    const int64_t row0 = (int64_t)blockIdx.x * TB;
    int lo = 0, hi = S - 1;                                  // the last segment that starts at or before the workgroup's first row
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (prefix[mid] <= row0) lo = mid; else hi = mid - 1;
    }
    int s = __builtin_amdgcn_readfirstlane(lo);
    const int64_t row = row0 + threadIdx.x;
    if (row >= total || row >= prefix[S]) return;
    while (s < S - 1 && row >= prefix[s + 1]) ++s;
    const int64_t k = row - prefix[s];
    if (k < 0 || k >= segment_count(seg_frame, seg_slot, F, frames, s)) return;
    const mtgs_stack_frame_desc &d = frames[seg_frame[s]];
    const int32_t slot = seg_slot[s];
    double p[3];
    int64_t src;
    if (slot == 0) {
        src = d.bg_sel[k];
        if (src < 0 || src >= d.offsets[1]) return;
        double x[3];
        load_point(d.points, 3, src, x);
#pragma unroll
        for (int c = 0; c < 3; ++c) p[c] = row34(d.lidar2global + 4 * c, x);
    } else {
        src = d.offsets[slot] + k;
        load_point(d.points, 3, src, p);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        xyz[row * 3 + c] = p[c];
        rgb[row * 3 + c] = d.rgb[src * 3 + c];
    }
    labels[row] = d.labels[src];
}

// ---- workspaces --------------------------------------------------------------------------------------------------------------------
inline size_t al(size_t b) { return mtgs_sort::align256(b); }
inline int key_bits_of(int B) {
    int bits = 1;
    while (((int64_t)1 << bits) <= (int64_t)B + 1) ++bits;
    return bits;
}

struct SplitWs {
    uint32_t *keys, *keys_sorted;
    int32_t *vals, *order;
    double *qbuf;
    void *sort_ws;
    size_t sort_bytes, bytes;
};
SplitWs carve_split(int64_t N, void *ws) {
    const int64_t n = N > 0 ? N : 1;
    char *w = (char *)ws;
    size_t o = 0;
    SplitWs k;
    k.keys = (uint32_t *)(w + o); o += al(n * 4);
    k.keys_sorted = (uint32_t *)(w + o); o += al(n * 4);
    k.vals = (int32_t *)(w + o); o += al(n * 4);
    k.order = (int32_t *)(w + o); o += al(n * 4);
    k.qbuf = (double *)(w + o); o += al(n * 24);
    k.sort_ws = w + o; k.sort_bytes = mtgs_sort::workspace_bytes<uint32_t>(n); o += al(k.sort_bytes);
    k.bytes = o;
    return k;
}

struct FrameWs {
    SplitWs split;
    int64_t *offsets, *partials;
    double *rows, *paint, *rgb;
    int32_t *labels, *count, *pre;
    uint8_t *fov;
    size_t bytes;
};
FrameWs carve_frame(int64_t N, int B, void *ws) {
    const int64_t n = N > 0 ? N : 1;
    FrameWs k;
    k.split = carve_split(N, ws);
    char *w = (char *)ws;
    size_t o = k.split.bytes;
    k.offsets = (int64_t *)(w + o); o += al((size_t)(B + 2) * 8);
    k.partials = (int64_t *)(w + o); o += al(mtgs_scan::workspace_bytes(n + 1));
    k.rows = (double *)(w + o); o += al(n * 24);
    k.paint = (double *)(w + o); o += al(n * 24);
    k.rgb = (double *)(w + o); o += al(n * 24);
    k.labels = (int32_t *)(w + o); o += al(n * 4);
    k.count = (int32_t *)(w + o); o += al(n * 4);
    k.pre = (int32_t *)(w + o); o += al((n + 1) * 4);
    k.fov = (uint8_t *)(w + o); o += al(n);
    k.bytes = o;
    return k;
}

#define STACK_BOXES(fn, B) \
    MTGS_REQUIRE(B >= 0 && B <= MTGS_STACK_MAX_BOXES, MTGS_EINVAL, "%s: B outside [0, %d] (%d)", fn, MTGS_STACK_MAX_BOXES, B)

int check_split_inputs(const char *fn, int64_t N, const void *points, int64_t row_stride, int B, const double *lidar2box,
                       const double *half_tight, const double *half_inflated, const void *ws) {
    MTGS_COUNT31(fn, N);
    STACK_BOXES(fn, B);
    if (N > 0) {
        MTGS_NONNULL(fn, points);
        MTGS_REQUIRE(row_stride >= 3, MTGS_EINVAL, "%s: row_stride < 3 (%lld)", fn, (long long)row_stride);
    }
    if (B > 0) {
        MTGS_NONNULL(fn, lidar2box); MTGS_NONNULL(fn, half_tight); MTGS_NONNULL(fn, half_inflated);
    }
    MTGS_NONNULL(fn, ws);
    MTGS_REQUIRE(((uintptr_t)ws & 15) == 0, MTGS_EINVAL, "%s: workspace must be 16-byte aligned", fn);
    return MTGS_OK;
}

// classify, sort, group offsets, rows: N > 0
template <class T>
int split_launch(const char *fn, int32_t N, const T *points, int64_t row_stride, int B, const double *lidar2box, const double *half_tight,
                 const double *half_inflated, const uint8_t *include, const double *box2lidar, const SplitWs &k, int64_t *offsets,
                 int32_t *slot, double *rows, double *paint, hipStream_t st) {
    const unsigned blocks = (unsigned)ceil_div64(N, TB);
    classify_kernel<T><<<blocks, TB, 0, st>>>(N, points, row_stride, B, lidar2box, half_tight, half_inflated, include, k.keys, k.vals, slot,
                                              k.qbuf);
    MTGS_CHECK_LAUNCH(fn);
    const int rc = mtgs_sort::sort_pairs<uint32_t>(N, key_bits_of(B), k.keys, k.vals, k.keys_sorted, k.order, k.sort_ws, k.sort_bytes, st, fn);
    if (rc != MTGS_OK) return rc;
    offsets_kernel<<<(unsigned)ceil_div64(B + 2, TB), TB, 0, st>>>(N, B, k.keys_sorted, offsets);
    rows_kernel<T><<<blocks, TB, 0, st>>>(N, points, row_stride, B, k.keys_sorted, k.order, k.qbuf, box2lidar, rows, paint);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}

}  // namespace

extern "C" int mtgs_stack_split_workspace_bytes(int64_t N, int B, size_t *bytes) {
    const char *fn = "mtgs_stack_split_workspace_bytes";
    MTGS_COUNT31(fn, N);
    STACK_BOXES(fn, B);
    MTGS_NONNULL(fn, bytes);
    *bytes = carve_split(N, nullptr).bytes;
    return MTGS_OK;
}

extern "C" int mtgs_stack_split(int64_t N, const void *points, int points_f64, int64_t row_stride, int B, const double *lidar2box,
                                const double *half_tight, const double *half_inflated, const uint8_t *include, double *out_points,
                                int64_t *offsets, int32_t *slot, void *ws, size_t ws_bytes, void *stream) {
    const char *fn = "mtgs_stack_split";
    const int rc = check_split_inputs(fn, N, points, row_stride, B, lidar2box, half_tight, half_inflated, ws);
    if (rc != MTGS_OK) return rc;
    MTGS_NONNULL(fn, offsets);
    MTGS_REQUIRE(((uintptr_t)offsets & 7) == 0, MTGS_EINVAL, "%s: offsets must be 8-byte aligned", fn);
    const SplitWs k = carve_split(N, ws);
    MTGS_REQUIRE(ws_bytes >= k.bytes, MTGS_EWORKSPACE, "%s: workspace %zu < %zu bytes", fn, ws_bytes, k.bytes);
    hipStream_t st = (hipStream_t)stream;
    if (N == 0) return mtgs_zero_async(offsets, (size_t)(B + 2) * sizeof(int64_t), st);
    MTGS_NONNULL(fn, out_points);
    if (points_f64)
        return split_launch<double>(fn, (int32_t)N, (const double *)points, row_stride, B, lidar2box, half_tight, half_inflated, include, nullptr,
                                    k, offsets, slot, out_points, nullptr, st);
    return split_launch<float>(fn, (int32_t)N, (const float *)points, row_stride, B, lidar2box, half_tight, half_inflated, include, nullptr, k,
                               offsets, slot, out_points, nullptr, st);
}

extern "C" int mtgs_stack_frame_workspace_bytes(int64_t N, int B, size_t *bytes) {
    const char *fn = "mtgs_stack_frame_workspace_bytes";
    MTGS_COUNT31(fn, N);
    STACK_BOXES(fn, B);
    MTGS_NONNULL(fn, bytes);
    *bytes = carve_frame(N, B, nullptr).bytes;
    return MTGS_OK;
}

extern "C" int mtgs_stack_frame(int64_t N, const void *points, int points_f64, int64_t row_stride, int B, const double *lidar2box,
                                const double *box2lidar, const double *half_tight, const double *half_inflated, const uint8_t *include,
                                int C, const double *lidar2imgs, int h, int w, const uint8_t *images, int reverse_channels,
                                const uint8_t *masks, int label_cutoff, double *out_points, double *out_rgb, int32_t *out_labels,
                                int64_t *out_offsets, int32_t *bg_sel, int64_t *bg_kept, int32_t *slot, void *ws, size_t ws_bytes,
                                void *stream) {
    const char *fn = "mtgs_stack_frame";
    int rc = check_split_inputs(fn, N, points, row_stride, B, lidar2box, half_tight, half_inflated, ws);
    if (rc != MTGS_OK) return rc;
    if (B > 0) MTGS_NONNULL(fn, box2lidar);
    MTGS_NONNULL(fn, lidar2imgs); MTGS_NONNULL(fn, images); MTGS_NONNULL(fn, masks);
    MTGS_NONNULL(fn, out_offsets); MTGS_NONNULL(fn, bg_kept);
    MTGS_REQUIRE(((uintptr_t)out_offsets & 7) == 0 && ((uintptr_t)bg_kept & 7) == 0, MTGS_EINVAL,
                 "%s: out_offsets and bg_kept must be 8-byte aligned", fn);
    const FrameWs k = carve_frame(N, B, ws);
    MTGS_REQUIRE(ws_bytes >= k.bytes, MTGS_EWORKSPACE, "%s: workspace %zu < %zu bytes", fn, ws_bytes, k.bytes);
    hipStream_t st = (hipStream_t)stream;
    if (N == 0) {
        rc = mtgs_zero_async(out_offsets, (size_t)(B + 2) * sizeof(int64_t), st);
        return rc != MTGS_OK ? rc : mtgs_zero_async(bg_kept, sizeof(int64_t), st);
    }
    MTGS_NONNULL(fn, out_points); MTGS_NONNULL(fn, out_rgb); MTGS_NONNULL(fn, out_labels); MTGS_NONNULL(fn, bg_sel);
    const int32_t n = (int32_t)N;
    rc = points_f64 ? split_launch<double>(fn, n, (const double *)points, row_stride, B, lidar2box, half_tight, half_inflated, include,
                                           box2lidar, k.split, k.offsets, slot, k.rows, k.paint, st)
                    : split_launch<float>(fn, n, (const float *)points, row_stride, B, lidar2box, half_tight, half_inflated, include,
                                          box2lidar, k.split, k.offsets, slot, k.rows, k.paint, st);
    if (rc != MTGS_OK) return rc;
    rc = mtgs_lidar_paint(N, k.paint, 1, 3, C, lidar2imgs, h, w, images, reverse_channels, masks, k.rgb, k.labels, k.fov, k.count, stream);
    if (rc != MTGS_OK) return rc;
    mtgs_scan::run(N + 1, FovValue{k.fov, k.offsets, B, N}, FovSink{k.pre, k.rows, k.rgb, k.labels, out_points, out_rgb, out_labels},
                   k.partials, nullptr, st);
    offsets2_kernel<<<(unsigned)ceil_div64(B + 2, TB), TB, 0, st>>>(n, B, k.offsets, k.pre, out_offsets);
    mtgs_scan::run(N + 1, LabelValue{out_labels, out_offsets, label_cutoff, N}, LabelSink{bg_sel}, k.partials, bg_kept, st);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}

extern "C" int mtgs_stack_plan_workspace_bytes(int64_t S, size_t *bytes) {
    const char *fn = "mtgs_stack_plan_workspace_bytes";
    MTGS_COUNT31(fn, S);
    MTGS_NONNULL(fn, bytes);
    *bytes = mtgs_scan::workspace_bytes(S + 1);
    return MTGS_OK;
}

extern "C" int mtgs_stack_plan(int64_t S, const int32_t *seg_frame, const int32_t *seg_slot, int64_t F, const mtgs_stack_frame_desc *frames,
                               int64_t *prefix, void *ws, size_t ws_bytes, void *stream) {
    const char *fn = "mtgs_stack_plan";
    MTGS_COUNT31(fn, S);
    MTGS_COUNT31(fn, F);
    MTGS_NONNULL(fn, prefix); MTGS_NONNULL(fn, ws);
    if (S > 0) {
        MTGS_NONNULL(fn, seg_frame); MTGS_NONNULL(fn, seg_slot); MTGS_NONNULL(fn, frames);
    }
    MTGS_REQUIRE(((uintptr_t)ws & 7) == 0 && ((uintptr_t)prefix & 7) == 0, MTGS_EINVAL, "%s: workspace and prefix must be 8-byte aligned", fn);
    const size_t need = mtgs_scan::workspace_bytes(S + 1);
    MTGS_REQUIRE(ws_bytes >= need, MTGS_EWORKSPACE, "%s: workspace %zu < %zu bytes", fn, ws_bytes, need);
    mtgs_scan::run(S + 1, CountValue{seg_frame, seg_slot, F, frames, S}, PrefixSink{prefix}, (int64_t *)ws, nullptr, (hipStream_t)stream);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}

extern "C" int mtgs_stack_gather(int64_t S, const int32_t *seg_frame, const int32_t *seg_slot, int64_t F, const mtgs_stack_frame_desc *frames,
                                 const int64_t *prefix, int64_t total, double *xyz, double *rgb, int32_t *labels, void *stream) {
    const char *fn = "mtgs_stack_gather";
    MTGS_COUNT31(fn, S);
    MTGS_COUNT31(fn, F);
    MTGS_COUNT31(fn, total);
    if (total == 0) return MTGS_OK;
    MTGS_REQUIRE(S > 0, MTGS_EINVAL, "%s: total > 0 without a segment (S = 0)", fn);
    MTGS_NONNULL(fn, seg_frame); MTGS_NONNULL(fn, seg_slot); MTGS_NONNULL(fn, frames); MTGS_NONNULL(fn, prefix);
    MTGS_NONNULL(fn, xyz); MTGS_NONNULL(fn, rgb); MTGS_NONNULL(fn, labels);
    gather_kernel<<<(unsigned)ceil_div64(total, TB), TB, 0, (hipStream_t)stream>>>((int32_t)S, seg_frame, seg_slot, F, frames, prefix, total, xyz,
                                                                                   rgb, labels);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}
