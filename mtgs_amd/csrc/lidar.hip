// lidar.hip -- lidar sweeps through the cameras on the device (include/mtgs_lidar.h states the arithmetic; mtgs_amd.lidar):
// the sparse lidar depth image of a training frame (CustomInputDataset._get_depth_from_lidar, mtgs/dataset/custom_dataset.py:
// 175-201) and the colours and semantic labels of the seeding cloud (get_rgb_point_cloud, mtgs/utils/nuplan_pointcloud.py:28-60;
// get_semantic_point_cloud, nuplan_scripts/utils/nuplan_utils_custom.py:208-265).  Both are N points through a 3 x 4 matrix in
// fp64, a field-of-view test, then a scatter or a gather.
//
// mtgs_lidar_depth, one call =
//   depth_clear_kernel     ws[pixel] = -1
//   depth_scatter_kernel   one thread per point: project, test, atomicMax(ws[pixel], i) -- an integer vector atomic, so the winner
//                          is the largest index whatever the order of arrival (NumPy's "the last assignment wins")
//   depth_resolve_kernel   one thread per pixel: the winner's q_2 again (the same function, the same bits), float32, times scale
// mtgs_lidar_paint, one launch: one thread per point, the cameras looped inside it, so the sum over the seeing cameras is taken in
// camera order and the label is the first seeing camera's with no atomics and no second pass.  A camera the point is not seen by
// costs the projection only.  The matrices are indexed by wave-uniform values only, so they are read by scalar loads.
//
// Texels stay 3 bytes wide.  The four neighbours of a point are two runs of 6 contiguous bytes, every point of a wave somewhere
// else in the image: the cost is the number of cache lines touched (two per point and camera), which a 4-byte texel would not
// change, while widening eight 1920 x 1080 images first would read 50 MB and write 66 MB to serve a sweep that touches a few MB.
//
// Compiled with -ffp-contract=off: every product and sum rounds once, as the NumPy restatement of tests/lidar_refs.py does.
#include "common.hpp"
#include "lidar_sample.hpp"      // load_point, row34 and the per-camera sample that brightness.hip shares

namespace {

constexpr int TB = 256;

struct Mat34 {
    double m[12];
};
struct Mat33 {
    double m[9];
};

__device__ __forceinline__ double row33(const double *m, const double c[3]) { return (m[0] * c[0] + m[1] * c[1]) + m[2] * c[2]; }

// steps 1-6 of mtgs_lidar_depth: the pixel of x, or -1; *q2 is the depth the pixel would take
__device__ __forceinline__ int32_t depth_pixel(const Mat34 &L, const Mat33 &K, const double x[3], int h, int w, double *q2) {
    double cam[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) cam[r] = row34(L.m + 4 * r, x);
    *q2 = row33(K.m + 6, cam);
    if (!(cam[2] > 0.0)) return -1;
    const double u = row33(K.m, cam) / *q2, v = row33(K.m + 3, cam) / *q2;
    if (!(v >= 0.0 && v < (double)h && u >= 0.0 && u < (double)w)) return -1;      // false on NaN
    return (int32_t)v * w + (int32_t)u;                                            // 0 <= u < w, 0 <= v < h: inside ws[h * w]
}

__device__ __forceinline__ void load_mats(const double *__restrict__ lidar2cam, const double *__restrict__ Kd, Mat34 &L, Mat33 &K) {
#pragma unroll
    for (int k = 0; k < 12; ++k) L.m[k] = lidar2cam[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) K.m[k] = Kd[k];
}

__global__ __launch_bounds__(TB) void depth_clear_kernel(int32_t n_pix, int32_t *__restrict__ ws) {
    const int64_t t = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (t < n_pix) ws[t] = -1;
}

template <class T>
__global__ __launch_bounds__(TB) void depth_scatter_kernel(int32_t N, const T *__restrict__ points, int64_t stride,
                                                           const double *__restrict__ lidar2cam, const double *__restrict__ Kd, int h,
                                                           int w, int32_t *__restrict__ ws) {
    const int64_t t = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (t >= N) return;
    Mat34 L;
    Mat33 K;
    load_mats(lidar2cam, Kd, L, K);
    double x[3], q2;
    load_point(points, stride, t, x);
    const int32_t pix = depth_pixel(L, K, x, h, w, &q2);
    if (pix >= 0) atomicMax(ws + pix, (int32_t)t);
}

template <class T>
__global__ __launch_bounds__(TB) void depth_resolve_kernel(int32_t N, const T *__restrict__ points, int64_t stride,
                                                           const double *__restrict__ lidar2cam, const double *__restrict__ Kd, int h,
                                                           int w, float scale, const int32_t *__restrict__ ws,
                                                           float *__restrict__ depth, int32_t *__restrict__ index) {
    const int64_t t = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (t >= (int64_t)h * w) return;
    const int32_t i = ws[t];
    float d = 0.0f;
    if (i >= 0 && i < N) {
        Mat34 L;
        Mat33 K;
        load_mats(lidar2cam, Kd, L, K);
        double x[3], q2;
        load_point(points, stride, i, x);
        depth_pixel(L, K, x, h, w, &q2);
        d = (float)q2 * scale;
    }
    depth[t] = d;
    if (index) index[t] = i;
}

template <class T>
__global__ __launch_bounds__(TB) void paint_kernel(int32_t N, const T *__restrict__ points, int64_t stride, int C,
                                                   const double *__restrict__ mats, int h, int w, const uint8_t *__restrict__ images,
                                                   int reverse, const uint8_t *__restrict__ masks, double *__restrict__ rgb,
                                                   int32_t *__restrict__ labels, uint8_t *__restrict__ fov, int32_t *__restrict__ count) {
    const int64_t t = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (t >= N) return;
    double x[3];
    load_point(points, stride, t, x);
    const int64_t plane = (int64_t)h * w;
    double sum[3] = {0.0, 0.0, 0.0};
    int32_t seen = 0, label = 0;
    for (int c = 0; c < C; ++c) {
        double ix, iy;
        if (!lidar_see(mats + 12 * c, x, h, w, ix, iy)) continue;          // wave-uniform matrix: scalar loads
        if (masks && seen == 0)
            label = masks[c * plane + (int64_t)clampi((int)nearbyint(iy), h - 1) * w + clampi((int)nearbyint(ix), w - 1)];
        if (images) {
            const LidarTaps taps = lidar_taps(images + c * plane * 3, h, w, ix, iy);
#pragma unroll
            for (int k = 0; k < 3; ++k) sum[k] = sum[k] + lidar_tap_value(taps, reverse ? 2 - k : k);
        }
        ++seen;
    }
    if (rgb) {
#pragma unroll
        for (int k = 0; k < 3; ++k) rgb[t * 3 + k] = seen > 0 ? sum[k] / (double)seen : 0.0;
    }
    if (labels) labels[t] = label;
    fov[t] = seen > 0 ? 1 : 0;
    count[t] = seen;
}

}  // namespace

#define LIDAR_HW(fn, h, w)                                                                                                     \
    MTGS_REQUIRE(h >= 1 && w >= 1 && (int64_t)h * w < ((int64_t)1 << 31), MTGS_EINVAL, "%s: h and w must be >= 1 and h * w < 2^31 (%d x %d)", \
                 fn, h, w)

extern "C" int mtgs_lidar_depth_workspace_bytes(int h, int w, size_t *bytes) {
    const char *fn = "mtgs_lidar_depth_workspace_bytes";
    LIDAR_HW(fn, h, w);
    MTGS_NONNULL(fn, bytes);
    *bytes = (size_t)h * w * sizeof(int32_t);
    return MTGS_OK;
}

extern "C" int mtgs_lidar_depth(int64_t N, const void *points, int points_f64, int64_t row_stride, const double *lidar2cam,
                                const double *K, int h, int w, float scale, float *depth, int32_t *index, void *ws, size_t ws_bytes,
                                void *stream) {
    const char *fn = "mtgs_lidar_depth";
    MTGS_COUNT31(fn, N);
    LIDAR_HW(fn, h, w);
    MTGS_NONNULL(fn, lidar2cam); MTGS_NONNULL(fn, K); MTGS_NONNULL(fn, depth); MTGS_NONNULL(fn, ws);
    if (N > 0) {
        MTGS_NONNULL(fn, points);
        MTGS_REQUIRE(row_stride >= 3, MTGS_EINVAL, "%s: row_stride < 3 (%lld)", fn, (long long)row_stride);
    }
    const size_t need = (size_t)h * w * sizeof(int32_t);
    MTGS_REQUIRE(ws_bytes >= need, MTGS_EWORKSPACE, "%s: workspace %zu < %zu bytes", fn, ws_bytes, need);
    MTGS_REQUIRE(((uintptr_t)ws & 3) == 0, MTGS_EINVAL, "%s: workspace must be 4-byte aligned", fn);
    hipStream_t st = (hipStream_t)stream;
    const int32_t n_pix = h * w, n = (int32_t)N;
    const unsigned pix_blocks = (unsigned)ceil_div64(n_pix, TB), pt_blocks = (unsigned)ceil_div64(N, TB);
    int32_t *win = (int32_t *)ws;
    depth_clear_kernel<<<pix_blocks, TB, 0, st>>>(n_pix, win);
    MTGS_CHECK_LAUNCH(fn);
    if (points_f64) {
        const double *p = (const double *)points;
        if (N > 0) depth_scatter_kernel<double><<<pt_blocks, TB, 0, st>>>(n, p, row_stride, lidar2cam, K, h, w, win);
        depth_resolve_kernel<double><<<pix_blocks, TB, 0, st>>>(n, p, row_stride, lidar2cam, K, h, w, scale, win, depth, index);
    } else {
        const float *p = (const float *)points;
        if (N > 0) depth_scatter_kernel<float><<<pt_blocks, TB, 0, st>>>(n, p, row_stride, lidar2cam, K, h, w, win);
        depth_resolve_kernel<float><<<pix_blocks, TB, 0, st>>>(n, p, row_stride, lidar2cam, K, h, w, scale, win, depth, index);
    }
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}

extern "C" int mtgs_lidar_paint(int64_t N, const void *points, int points_f64, int64_t row_stride, int C, const double *lidar2imgs,
                                int h, int w, const uint8_t *images, int reverse_channels, const uint8_t *masks, double *rgb,
                                int32_t *labels, uint8_t *fov, int32_t *count, void *stream) {
    const char *fn = "mtgs_lidar_paint";
    MTGS_COUNT31(fn, N);
    LIDAR_HW(fn, h, w);
    MTGS_REQUIRE(C >= 1 && C <= MTGS_LIDAR_MAX_CAMERAS, MTGS_EINVAL, "%s: C outside [1, %d] (%d)", fn, MTGS_LIDAR_MAX_CAMERAS, C);
    MTGS_REQUIRE((images != nullptr) == (rgb != nullptr), MTGS_EINVAL, "%s: images and rgb go together", fn);
    MTGS_REQUIRE((masks != nullptr) == (labels != nullptr), MTGS_EINVAL, "%s: masks and labels go together", fn);
    if (N == 0) return MTGS_OK;
    MTGS_NONNULL(fn, points); MTGS_NONNULL(fn, lidar2imgs); MTGS_NONNULL(fn, fov); MTGS_NONNULL(fn, count);
    MTGS_REQUIRE(row_stride >= 3, MTGS_EINVAL, "%s: row_stride < 3 (%lld)", fn, (long long)row_stride);
    hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = (unsigned)ceil_div64(N, TB);
    if (points_f64)
        paint_kernel<double><<<blocks, TB, 0, st>>>((int32_t)N, (const double *)points, row_stride, C, lidar2imgs, h, w, images,
                                                    reverse_channels, masks, rgb, labels, fov, count);
    else
        paint_kernel<float><<<blocks, TB, 0, st>>>((int32_t)N, (const float *)points, row_stride, C, lidar2imgs, h, w, images,
                                                   reverse_channels, masks, rgb, labels, fov, count);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}
