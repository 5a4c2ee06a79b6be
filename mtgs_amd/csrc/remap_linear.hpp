// remap_linear.hpp -- what the two remap kernels (undistort.hip, redistort.hip) share: the tile's pixel of a thread, a float32 map
// coordinate as an integer, and MTGS_UNDISTORT_LINEAR's footprint -- five fractional bits, four taps, each inside or zero -- as
// include/mtgs_undistort.h defines it.  Integer arithmetic after the one float32 product.
#pragma once
#include "common.hpp"

constexpr int REMAP_TW = MTGS_UNDISTORT_TILE_W, REMAP_TH = MTGS_UNDISTORT_TILE_H, REMAP_NT = REMAP_TW * REMAP_TH;
static_assert(REMAP_TW == MTGS_WAVE && REMAP_NT <= 1024, "a wave is one row of a tile");

// an integral float32 coordinate as an int; anything with !(|f| < 2^30), non-finite included, becomes a coordinate far outside
__device__ __forceinline__ int remap_coord(float f) { return fabsf(f) < 1073741824.0f ? (int)f : -(1 << 30); }

__device__ __forceinline__ bool remap_pixel_of(int oh, int ow, int &i, int &j) {
    j = (int)blockIdx.x * REMAP_TW + (int)(threadIdx.x % REMAP_TW);
    i = (int)blockIdx.y * REMAP_TH + (int)(threadIdx.x / REMAP_TW);
    return i < oh && j < ow;
}

static inline dim3 remap_tiles(int oh, int ow) { return dim3((unsigned)ceil_div64(ow, REMAP_TW), (unsigned)ceil_div64(oh, REMAP_TH)); }

// the 2 x 2 footprint of one map entry in a source of h x w: its top-left pixel, which of its taps are inside, their weights
struct LinearTaps {
    int ix, iy;
    bool x0, x1, y0, y1;
    int w00, w01, w10, w11;
};

__device__ __forceinline__ LinearTaps linear_taps(float mapx, float mapy, int h, int w) {
    const int sx = remap_coord(rintf(__fmul_rn(mapx, 32.0f))), sy = remap_coord(rintf(__fmul_rn(mapy, 32.0f)));
    LinearTaps t;
    t.ix = sx >> 5, t.iy = sy >> 5;
    const int a = sx & 31, b = sy & 31;
    t.x0 = t.ix >= 0 && t.ix < w, t.x1 = t.ix + 1 >= 0 && t.ix + 1 < w, t.y0 = t.iy >= 0 && t.iy < h, t.y1 = t.iy + 1 >= 0 && t.iy + 1 < h;
    t.w00 = (32 - a) * (32 - b) * 32, t.w01 = a * (32 - b) * 32, t.w10 = (32 - a) * b * 32, t.w11 = a * b * 32;
    return t;
}

__device__ __forceinline__ int linear_blend(const LinearTaps &t, int v00, int v01, int v10, int v11) {
    return (t.w00 * v00 + t.w01 * v01 + t.w10 * v10 + t.w11 * v11 + 16384) >> 15;
}
