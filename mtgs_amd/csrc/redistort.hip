// redistort.hip -- a rendered frame bent back into the raw camera (the evaluation dump in image_saving_mode = "nuplan",
// scene_model/custom_pipeline.py:131-143, through invert_distortion, utils/camera_utils.py:340-356): the map of
// initInverseRectificationMap as a fixed number of fixed-point iterations of the inverse lens model in fp64, and the 8-bit INTER_LINEAR
// sampling of remap, as include/mtgs_redistort.h defines them ([RECALLED]: the project's definition, not a claim about OpenCV's bytes).
// Compiled with -ffp-contract=off: every product, sum and quotient of the map rounds once, as the NumPy restatement
// (tests/redistort_refs.py) does.
//
// redistort_frame_kernel, one launch: undistort.hip's tile -- a workgroup owns TW x TH destination pixels, one thread per pixel, a
// wave one row of 64 neighbours whose source pixels are neighbours too.  A thread evaluates its map entry once (per iteration one fp64
// division and about 25 other fp64 operations), or reads it from the caller's map.  The loop count is a kernel argument: the loop is
// wave-uniform, only the folded-over exit masks lanes.  A float32 source is converted tap by tap with the JPEG encoder's load_sample.
#include "common.hpp"
#include "remap_linear.hpp"
#include "sample_u8.hpp"

namespace {

constexpr int NT = REMAP_NT;

// the rule of the header, in its order; cam is read through wave-uniform addresses
__device__ __forceinline__ void inverse_map_of(const double *__restrict__ cam, int iterations, int i, int j, float &mapx, float &mapy) {
    const double fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3], nfx = cam[4], nfy = cam[5], ncx = cam[6], ncy = cam[7];
    const double k1 = cam[8], k2 = cam[9], p1 = cam[10], p2 = cam[11], k3 = cam[12];
    const double x0 = ((double)j - cx) / fx, y0 = ((double)i - cy) / fy;
    double x = x0, y = y0;
    for (int it = 0; it < iterations; ++it) {
        const double r2 = x * x + y * y;
        const double icdist = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2);
        if (icdist < 0.0) {              // the model has folded over: this lane is done, at its start
            x = x0, y = y0;
            break;
        }
        const double dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x);
        const double dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y;
        x = (x0 - dx) * icdist;
        y = (y0 - dy) * icdist;
    }
    mapx = (float)(nfx * x + ncx);
    mapy = (float)(nfy * y + ncy);
}

__global__ __launch_bounds__(NT) void redistort_frame_kernel(int h, int w, int oh, int ow, const double *__restrict__ cam, int iterations,
                                                             const float *__restrict__ map, const void *__restrict__ src, bool is_float,
                                                             bool round, int64_t s0, int64_t s1, int64_t s2, int channels,
                                                             uint8_t *__restrict__ dst) {
    int i, j;
    if (!remap_pixel_of(oh, ow, i, j)) return;
    const int64_t at = (int64_t)i * ow + j;
    float mapx, mapy;
    if (map != nullptr) {
        mapx = map[2 * at];
        mapy = map[2 * at + 1];
    } else {
        inverse_map_of(cam, iterations, i, j, mapx, mapy);
    }
    const LinearTaps f = linear_taps(mapx, mapy, h, w);
    const int64_t o00 = (int64_t)f.iy * s0 + (int64_t)f.ix * s1;
    for (int k = 0; k < channels; ++k) {
        const int64_t o = o00 + k * s2;
        const int v00 = (f.y0 && f.x0) ? load_sample(src, is_float, round, o) : 0;
        const int v01 = (f.y0 && f.x1) ? load_sample(src, is_float, round, o + s1) : 0;
        const int v10 = (f.y1 && f.x0) ? load_sample(src, is_float, round, o + s0) : 0;
        const int v11 = (f.y1 && f.x1) ? load_sample(src, is_float, round, o + s0 + s1) : 0;
        dst[at * channels + k] = (uint8_t)linear_blend(f, v00, v01, v10, v11);
    }
}

__global__ __launch_bounds__(NT) void redistort_map_kernel(int oh, int ow, const double *__restrict__ cam, int iterations,
                                                           float2 *__restrict__ map) {
    int i, j;
    if (!remap_pixel_of(oh, ow, i, j)) return;
    float mapx, mapy;
    inverse_map_of(cam, iterations, i, j, mapx, mapy);
    map[(int64_t)i * ow + j] = make_float2(mapx, mapy);
}

int check_size(const char *fn, const char *name, int v) {
    MTGS_REQUIRE(v >= 1 && v <= MTGS_UNDISTORT_MAX_SIZE, MTGS_EINVAL, "%s: %s outside [1, %d] (%d)", fn, name, MTGS_UNDISTORT_MAX_SIZE, v);
    return MTGS_OK;
}

int check_iterations(const char *fn, int iterations) {
    MTGS_REQUIRE(iterations >= 0 && iterations <= MTGS_REDISTORT_MAX_ITERATIONS, MTGS_EINVAL, "%s: iterations outside [0, %d] (%d)", fn,
                 MTGS_REDISTORT_MAX_ITERATIONS, iterations);
    return MTGS_OK;
}

}  // namespace


extern "C" int mtgs_redistort_frame(int h, int w, int oh, int ow, const double *cam, int iterations, const float *map, const void *src,
                                    int src_float, int conversion, int64_t stride_y, int64_t stride_x, int64_t stride_c, int channels,
                                    uint8_t *dst, void *stream) {
    const char *fn = "mtgs_redistort_frame";
    if (int rc = check_size(fn, "h", h)) return rc;
    if (int rc = check_size(fn, "w", w)) return rc;
    if (int rc = check_size(fn, "oh", oh)) return rc;
    if (int rc = check_size(fn, "ow", ow)) return rc;
    if (map == nullptr) {
        MTGS_NONNULL(fn, cam);
        if (int rc = check_iterations(fn, iterations)) return rc;
    }
    MTGS_NONNULL(fn, src); MTGS_NONNULL(fn, dst);
    MTGS_REQUIRE(((uintptr_t)cam & 7) == 0, MTGS_EINVAL, "%s: cam must be 8-byte aligned", fn);
    MTGS_REQUIRE(((uintptr_t)map & 3) == 0, MTGS_EINVAL, "%s: map must be 4-byte aligned", fn);
    MTGS_REQUIRE(src_float == 0 || src_float == 1, MTGS_EINVAL, "%s: src_float must be 0 or 1 (%d)", fn, src_float);
    MTGS_REQUIRE(!src_float || ((uintptr_t)src & 3) == 0, MTGS_EINVAL, "%s: src must be 4-byte aligned when src_float is set", fn);
    MTGS_REQUIRE(conversion == MTGS_PRESENT_U8_TRUNCATE || conversion == MTGS_PRESENT_U8_ROUND, MTGS_EINVAL,
                 "%s: conversion must be MTGS_PRESENT_U8_TRUNCATE or MTGS_PRESENT_U8_ROUND (%d)", fn, conversion);
    MTGS_REQUIRE(channels == 1 || channels == 3, MTGS_EUNSUPPORTED, "%s: channels must be 1 or 3 (%d)", fn, channels);
    redistort_frame_kernel<<<remap_tiles(oh, ow), NT, 0, (hipStream_t)stream>>>(h, w, oh, ow, cam, iterations, map, src, src_float != 0,
                                                                               conversion == MTGS_PRESENT_U8_ROUND, stride_y, stride_x,
                                                                               stride_c, channels, dst);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}

extern "C" int mtgs_redistort_map(int oh, int ow, const double *cam, int iterations, float *map, void *stream) {
    const char *fn = "mtgs_redistort_map";
    if (int rc = check_size(fn, "oh", oh)) return rc;
    if (int rc = check_size(fn, "ow", ow)) return rc;
    if (int rc = check_iterations(fn, iterations)) return rc;
    MTGS_NONNULL(fn, cam); MTGS_NONNULL(fn, map);
    MTGS_REQUIRE(((uintptr_t)cam & 7) == 0, MTGS_EINVAL, "%s: cam must be 8-byte aligned", fn);
    MTGS_REQUIRE(((uintptr_t)map & 7) == 0, MTGS_EINVAL, "%s: map must be 8-byte aligned", fn);
    redistort_map_kernel<<<remap_tiles(oh, ow), NT, 0, (hipStream_t)stream>>>(oh, ow, cam, iterations, (float2 *)map);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}
