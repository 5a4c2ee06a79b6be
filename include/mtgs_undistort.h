#ifndef MTGS_UNDISTORT_H
#define MTGS_UNDISTORT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- lens undistortion of a training frame on the device (mtgs_amd/csrc/undistort.hip; mtgs_amd.undistort): what
 * CustomInputDataset._undistort_image (mtgs/dataset/custom_dataset.py:99-152) does with cv2.initUndistortRectifyMap and up to five
 * cv2.remap calls on the host, and what stack_RGB_point_cloud.py:53,64 does in front of the painting.  A header of its own, included
 * by mtgs_rast.h; its reviewed record is tests/golden/abi_signatures_undistort.txt.  Additive: it changed neither
 * MTGS_RAST_ABI_VERSION nor MTGS_RAST_HOT_ABI_VERSION.  Conventions (device pointers, `stream`, return codes, mtgs_rast_last_error)
 * are mtgs_rast.h's.
 *
 * [RECALLED] cv2 was not available to run.  The rule below is OpenCV's as recalled, and it is THIS PROJECT'S DEFINITION: nothing
 * here claims byte equality with OpenCV.  tests/undistort_refs.py restates it in NumPy and pins it with known answers that do not
 * depend on the recall.  NOT covered: INTER_CUBIC (used only in front of UniDepth, generate_dense_depth.py:198-220), the rational,
 * thin-prism and tilt coefficients (more than five), decoding PNG files.  adjust_brightness is mtgs_brightness.h.
 *
 * cam: DEVICE double[MTGS_UNDISTORT_CAM_DOUBLES] = fx, fy, cx, cy (the source camera), fx', fy', cx', cy' (the new camera), k1, k2,
 * p1, p2, k3 (k3 = 0 for four coefficients).  It lives on the device so that a captured launch follows a camera written later.
 *
 * The map of destination pixel (row i, column j), in fp64, ONE ROUNDING PER OPERATION (compiled with -ffp-contract=off), in this
 * order (initUndistortRectifyMap(K, D, None, K', size, CV_32FC2); OpenCV walks a row by repeated addition of the inverse matrix's
 * column, the closed form is used here because it is parallel -- the defined deviation):
 *   x = (j - cx') / fx'            y = (i - cy') / fy'
 *   x2 = x*x; y2 = y*y; r2 = x2 + y2; _2xy = 2*x*y
 *   kr = 1 + ((k3*r2 + k2)*r2 + k1)*r2
 *   xd = x*kr + p1*_2xy + p2*(r2 + 2*x2)
 *   yd = y*kr + p1*(r2 + 2*y2) + p2*_2xy
 *   mapx = (float32)(fx*xd + cx)   mapy = (float32)(fy*yd + cy)
 * A caller that has a map of its own (cv2's, say) passes it as `map`, float32 [oh, ow, 2] = (mapx, mapy), and `cam` is not read.
 *
 * A coordinate f (float32, after rint) with !(|f| < 2^30) -- non-finite ones included -- is OUTSIDE the source; no coordinate of a
 * source pixel is near that (sizes are at most MTGS_UNDISTORT_MAX_SIZE).
 *
 * MTGS_UNDISTORT_LINEAR (INTER_LINEAR, 8 bit, BORDER_CONSTANT 0): src uint8 [h, w, channels], channels 1 or 3.
 *   sx = rint(mapx * 32.0f) in float32, ties to even; sy likewise; ix = sx >> 5, iy = sy >> 5 (arithmetic); a = sx & 31, b = sy & 31
 *   out = ((32-a)(32-b)*32 * s[iy, ix] + a(32-b)*32 * s[iy, ix+1] + (32-a)b*32 * s[iy+1, ix] + ab*32 * s[iy+1, ix+1] + 16384) >> 15
 *   per channel; each of the four taps on its own reads 0 outside the source.  dst uint8 (out_float = 0) or float32 (out_float = 1:
 *   (float)byte / 255.0f, one correctly rounded division).
 * MTGS_UNDISTORT_NEAREST (INTER_NEAREST): dst[i, j, k] = src[rint(mapy), rint(mapx), k] (rint in float32, ties to even), 0 outside;
 *   elem_bytes 1 (uint8, bool) or 4 (int32), channels 1 .. 3.
 * MTGS_UNDISTORT_VALID: dst uint8 [oh, ow] = 1 where the NEAREST source pixel is inside the source and (src == NULL or
 *   src[that pixel, channel 0] == 0), else 0: the nearest remap of an all-255 plane followed by astype(bool), and with src the ego
 *   mask (uint8 or bool, nonzero on the ego vehicle) the rule of _get_ego_mask joined to it.
 *
 * mtgs_undistort_frame: n_planes <= MTGS_UNDISTORT_MAX_PLANES planes of one source size h x w to one size oh x ow in ONE launch, from
 * a HOST array of mtgs_undistort_plane (copied into the launch).  A workgroup of MTGS_UNDISTORT_TILE_W x MTGS_UNDISTORT_TILE_H
 * threads owns a tile of that many destination pixels; a thread evaluates the map of its pixel once and serves every plane from
 * it, so that no map is stored.  src_stride = (row, column, channel) in ELEMENTS, any value (also 0 or negative) as long as every
 * element lies in the allocation; dst is contiguous [oh, ow, channels].  No atomics, no host read, capturable in a HIP graph.
 *
 * mtgs_undistort_map: map float32 [oh, ow, 2] = (mapx, mapy) of the closed form above.
 *
 * Limits: 1 <= h, w, oh, ow <= MTGS_UNDISTORT_MAX_SIZE.  The host checks name the bad argument. */
#define MTGS_UNDISTORT_TILE_W 64
#define MTGS_UNDISTORT_TILE_H 4
#define MTGS_UNDISTORT_MAX_PLANES 8
#define MTGS_UNDISTORT_MAX_SIZE 16384
#define MTGS_UNDISTORT_CAM_DOUBLES 13
enum { MTGS_UNDISTORT_LINEAR = 0, MTGS_UNDISTORT_NEAREST = 1, MTGS_UNDISTORT_VALID = 2 };

typedef struct mtgs_undistort_plane {
    const void *src;
    void *dst;
    int64_t src_stride[3];
    int32_t op, elem_bytes, channels, out_float;
} mtgs_undistort_plane;

int mtgs_undistort_frame(int h, int w, int oh, int ow, const double *cam, const float *map, int n_planes,
                         const mtgs_undistort_plane *planes, void *stream);
int mtgs_undistort_map(int oh, int ow, const double *cam, float *map, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MTGS_UNDISTORT_H */
