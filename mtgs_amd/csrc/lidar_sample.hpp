// lidar_sample.hpp -- one point through one camera, as include/mtgs_lidar.h states it for mtgs_lidar_paint: the projection, the
// `see` test and the four bilinear taps of grid_sample(align_corners = True).  get_rgb_point_cloud and
// adjust_brightness_single_frame are line for line the same there, so paint_kernel (lidar.hip) and brightness_sample_kernel
// (brightness.hip) share this body.  fp64, every operation rounded once: both files are compiled with -ffp-contract=off.
#pragma once
#include "common.hpp"

namespace {

template <class T>
__device__ __forceinline__ void load_point(const T *__restrict__ points, int64_t stride, int64_t i, double x[3]) {
    const T *p = points + i * stride;
    x[0] = (double)p[0];
    x[1] = (double)p[1];
    x[2] = (double)p[2];
}

__device__ __forceinline__ double row34(const double *m, const double x[3]) { return ((m[0] * x[0] + m[1] * x[1]) + m[2] * x[2]) + m[3]; }

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// does the camera of matrix m (3 x 4 by rows, wave-uniform: scalar loads) see x?  If so (ix, iy) is its sampling position
__device__ __forceinline__ bool lidar_see(const double *m, const double x[3], int h, int w, double &ix, double &iy) {
    const double p2 = row34(m + 8, x);
    if (!(p2 > 0.1)) return false;
    const double z = fmin(fmax(p2, 1e-5), 99999.0);
    const double nx = (row34(m, x) / z) / (double)w, ny = (row34(m + 4, x) / z) / (double)h;
    if (!(nx < 1.0 && nx >= 0.0 && ny < 1.0 && ny >= 0.0)) return false;
    ix = (((nx * 2.0 - 1.0) + 1.0) / 2.0) * (double)(w - 1);
    iy = (((ny * 2.0 - 1.0) + 1.0) / 2.0) * (double)(h - 1);
    return true;
}

struct LidarTaps {
    const uint8_t *t00, *t01, *t10, *t11;
    double w00, w01, w10, w11;
};

// the four texels around (ix, iy) of one image [h, w, 3] and their weights
__device__ __forceinline__ LidarTaps lidar_taps(const uint8_t *__restrict__ img, int h, int w, double ix, double iy) {
    const double xf = floor(ix), yf = floor(iy);
    const double fx = ix - xf, fy = iy - yf;
    // ix may round up to w - 1 itself: the neighbour beyond the image has weight 0 and is read at the edge instead
    const int x0 = clampi((int)xf, w - 1), y0 = clampi((int)yf, h - 1), x1 = min(x0 + 1, w - 1), y1 = min(y0 + 1, h - 1);
    LidarTaps t;
    t.t00 = img + ((int64_t)y0 * w + x0) * 3;
    t.t01 = img + ((int64_t)y0 * w + x1) * 3;
    t.t10 = img + ((int64_t)y1 * w + x0) * 3;
    t.t11 = img + ((int64_t)y1 * w + x1) * 3;
    t.w00 = (1.0 - fx) * (1.0 - fy);
    t.w01 = fx * (1.0 - fy);
    t.w10 = (1.0 - fx) * fy;
    t.w11 = fx * fy;
    return t;
}

// the sampled value of channel ch in [0, 1], summed left to right
__device__ __forceinline__ double lidar_tap_value(const LidarTaps &t, int ch) {
    return (((double)t.t00[ch] / 255.0) * t.w00 + ((double)t.t01[ch] / 255.0) * t.w01) + ((double)t.t10[ch] / 255.0) * t.w10 +
           ((double)t.t11[ch] / 255.0) * t.w11;
}

}  // namespace
