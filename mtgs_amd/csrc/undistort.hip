// undistort.hip -- lens undistortion of a training frame (CustomInputDataset._undistort_image, mtgs/dataset/custom_dataset.py:99-152):
// the map of initUndistortRectifyMap in fp64 and the 8-bit INTER_LINEAR / INTER_NEAREST sampling of remap, as include/mtgs_undistort.h
// defines them ([RECALLED]: the project's definition, not a claim about OpenCV's bytes).  Compiled with -ffp-contract=off: every
// product and every sum of the map rounds once, as the NumPy restatement (tests/undistort_refs.py) does.
//
// undistort_frame_kernel, one launch for every plane of a frame: a workgroup owns a tile of TW x TH destination pixels, one thread
// per pixel, a wave one row of 64 neighbours -- their source pixels are neighbours too (the distortion is smooth), so a wave's taps
// fall into a few cache lines and its stores are contiguous.  A thread evaluates its map entry once (about 30 fp64 operations: far
// below what the loads cost) and walks the plane table, which lives in the kernel's arguments: the plane loop and the branch on
// the operation are wave-uniform.  Nothing but the planes is read or written: no map in memory, unless the caller passes one.
#include "common.hpp"
#include "remap_linear.hpp"

namespace {

constexpr int NT = REMAP_NT, MAXC = 3;

struct PlaneTable {
    mtgs_undistort_plane p[MTGS_UNDISTORT_MAX_PLANES];
    int n;
};

// the closed form of the header, in its order; cam is read through wave-uniform addresses
__device__ __forceinline__ void map_of(const double *__restrict__ cam, int i, int j, float &mapx, float &mapy) {
    const double fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3], nfx = cam[4], nfy = cam[5], ncx = cam[6], ncy = cam[7];
    const double k1 = cam[8], k2 = cam[9], p1 = cam[10], p2 = cam[11], k3 = cam[12];
    const double x = ((double)j - ncx) / nfx, y = ((double)i - ncy) / nfy;
    const double x2 = x * x, y2 = y * y, r2 = x2 + y2, _2xy = 2.0 * x * y;
    const double kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2;
    const double xd = x * kr + p1 * _2xy + p2 * (r2 + 2.0 * x2);
    const double yd = y * kr + p1 * (r2 + 2.0 * y2) + p2 * _2xy;
    mapx = (float)(fx * xd + cx);
    mapy = (float)(fy * yd + cy);
}

__global__ __launch_bounds__(NT) void undistort_frame_kernel(PlaneTable t, int h, int w, int oh, int ow, const double *__restrict__ cam,
                                                             const float *__restrict__ map) {
    int i, j;
    if (!remap_pixel_of(oh, ow, i, j)) return;
    const int64_t at = (int64_t)i * ow + j;
    float mapx, mapy;
    if (map != nullptr) {
        mapx = map[2 * at];
        mapy = map[2 * at + 1];
    } else {
        map_of(cam, i, j, mapx, mapy);
    }
    // INTER_NEAREST: the source pixel, or none
    const int nx = remap_coord(rintf(mapx)), ny = remap_coord(rintf(mapy));
    const bool inside = nx >= 0 && nx < w && ny >= 0 && ny < h;
    // INTER_LINEAR: five fractional bits, four taps, each inside or zero
    const LinearTaps f = linear_taps(mapx, mapy, h, w);

    for (int q = 0; q < t.n; ++q) {
        const mtgs_undistort_plane &p = t.p[q];
        const int64_t s0 = p.src_stride[0], s1 = p.src_stride[1], s2 = p.src_stride[2];
        if (p.op == MTGS_UNDISTORT_LINEAR) {
            const uint8_t *s = (const uint8_t *)p.src;
            const int64_t o00 = (int64_t)f.iy * s0 + (int64_t)f.ix * s1;
            for (int k = 0; k < p.channels; ++k) {
                const int64_t o = o00 + k * s2;
                const int v00 = (f.y0 && f.x0) ? s[o] : 0, v01 = (f.y0 && f.x1) ? s[o + s1] : 0;
                const int v10 = (f.y1 && f.x0) ? s[o + s0] : 0, v11 = (f.y1 && f.x1) ? s[o + s0 + s1] : 0;
                const int v = linear_blend(f, v00, v01, v10, v11);
                if (p.out_float) ((float *)p.dst)[at * p.channels + k] = __fdiv_rn((float)v, 255.0f);
                else ((uint8_t *)p.dst)[at * p.channels + k] = (uint8_t)v;
            }
        } else if (p.op == MTGS_UNDISTORT_NEAREST) {
            const int64_t o = (int64_t)ny * s0 + (int64_t)nx * s1;
            if (p.elem_bytes == 4) {
                for (int k = 0; k < p.channels; ++k)
                    ((uint32_t *)p.dst)[at * p.channels + k] = inside ? ((const uint32_t *)p.src)[o + k * s2] : 0u;
            } else {
                for (int k = 0; k < p.channels; ++k)
                    ((uint8_t *)p.dst)[at * p.channels + k] = inside ? ((const uint8_t *)p.src)[o + k * s2] : (uint8_t)0;
            }
        } else {
            bool ok = inside;
            if (ok && p.src != nullptr) ok = ((const uint8_t *)p.src)[(int64_t)ny * s0 + (int64_t)nx * s1] == 0;
            ((uint8_t *)p.dst)[at] = ok ? 1 : 0;
        }
    }
}

__global__ __launch_bounds__(NT) void undistort_map_kernel(int oh, int ow, const double *__restrict__ cam, float2 *__restrict__ map) {
    int i, j;
    if (!remap_pixel_of(oh, ow, i, j)) return;
    float mapx, mapy;
    map_of(cam, i, j, mapx, mapy);
    map[(int64_t)i * ow + j] = make_float2(mapx, mapy);
}

int check_size(const char *fn, const char *name, int v) {
    MTGS_REQUIRE(v >= 1 && v <= MTGS_UNDISTORT_MAX_SIZE, MTGS_EINVAL, "%s: %s outside [1, %d] (%d)", fn, name, MTGS_UNDISTORT_MAX_SIZE, v);
    return MTGS_OK;
}

}  // namespace


extern "C" int mtgs_undistort_frame(int h, int w, int oh, int ow, const double *cam, const float *map, int n_planes,
                                    const mtgs_undistort_plane *planes, void *stream) {
    const char *fn = "mtgs_undistort_frame";
    if (int rc = check_size(fn, "h", h)) return rc;
    if (int rc = check_size(fn, "w", w)) return rc;
    if (int rc = check_size(fn, "oh", oh)) return rc;
    if (int rc = check_size(fn, "ow", ow)) return rc;
    MTGS_REQUIRE(n_planes >= 1 && n_planes <= MTGS_UNDISTORT_MAX_PLANES, MTGS_EINVAL, "%s: n_planes outside [1, %d] (%d)", fn,
                 MTGS_UNDISTORT_MAX_PLANES, n_planes);
    MTGS_NONNULL(fn, planes);
    if (map == nullptr) MTGS_NONNULL(fn, cam);
    MTGS_REQUIRE(((uintptr_t)cam & 7) == 0, MTGS_EINVAL, "%s: cam must be 8-byte aligned", fn);
    MTGS_REQUIRE(((uintptr_t)map & 3) == 0, MTGS_EINVAL, "%s: map must be 4-byte aligned", fn);
    PlaneTable t{};
    t.n = n_planes;
    for (int q = 0; q < n_planes; ++q) {
        const mtgs_undistort_plane &p = planes[q];
        MTGS_REQUIRE(p.dst != nullptr, MTGS_EINVAL, "%s: null pointer: planes[%d].dst", fn, q);
        MTGS_REQUIRE(p.op >= MTGS_UNDISTORT_LINEAR && p.op <= MTGS_UNDISTORT_VALID, MTGS_EINVAL, "%s: planes[%d].op unknown (%d)", fn, q, p.op);
        MTGS_REQUIRE(p.op == MTGS_UNDISTORT_VALID || p.src != nullptr, MTGS_EINVAL, "%s: null pointer: planes[%d].src", fn, q);
        if (p.op == MTGS_UNDISTORT_LINEAR) {
            MTGS_REQUIRE(p.elem_bytes == 1, MTGS_EUNSUPPORTED, "%s: planes[%d].elem_bytes must be 1 for LINEAR (%d)", fn, q, p.elem_bytes);
            MTGS_REQUIRE(p.channels == 1 || p.channels == 3, MTGS_EUNSUPPORTED, "%s: planes[%d].channels must be 1 or 3 for LINEAR (%d)", fn, q, p.channels);
            MTGS_REQUIRE(!p.out_float || ((uintptr_t)p.dst & 3) == 0, MTGS_EINVAL, "%s: planes[%d].dst must be 4-byte aligned", fn, q);
        } else if (p.op == MTGS_UNDISTORT_NEAREST) {
            MTGS_REQUIRE(p.elem_bytes == 1 || p.elem_bytes == 4, MTGS_EUNSUPPORTED, "%s: planes[%d].elem_bytes must be 1 or 4 (%d)", fn, q, p.elem_bytes);
            MTGS_REQUIRE(p.channels >= 1 && p.channels <= MAXC, MTGS_EUNSUPPORTED, "%s: planes[%d].channels outside [1, %d] (%d)", fn, q, MAXC, p.channels);
            MTGS_REQUIRE(p.elem_bytes != 4 || (((uintptr_t)p.dst | (uintptr_t)p.src) & 3) == 0, MTGS_EINVAL,
                         "%s: planes[%d].src and .dst must be 4-byte aligned", fn, q);
        }
        t.p[q] = p;
    }
    undistort_frame_kernel<<<remap_tiles(oh, ow), NT, 0, (hipStream_t)stream>>>(t, h, w, oh, ow, cam, map);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}

extern "C" int mtgs_undistort_map(int oh, int ow, const double *cam, float *map, void *stream) {
    const char *fn = "mtgs_undistort_map";
    if (int rc = check_size(fn, "oh", oh)) return rc;
    if (int rc = check_size(fn, "ow", ow)) return rc;
    MTGS_NONNULL(fn, cam); MTGS_NONNULL(fn, map);
    MTGS_REQUIRE(((uintptr_t)cam & 7) == 0, MTGS_EINVAL, "%s: cam must be 8-byte aligned", fn);
    MTGS_REQUIRE(((uintptr_t)map & 7) == 0, MTGS_EINVAL, "%s: map must be 8-byte aligned", fn);
    undistort_map_kernel<<<remap_tiles(oh, ow), NT, 0, (hipStream_t)stream>>>(oh, ow, cam, (float2 *)map);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}
