#ifndef MTGS_REDISTORT_H
#define MTGS_REDISTORT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- a rendered frame bent back into the raw camera on the device (mtgs_amd/csrc/redistort.hip; mtgs_amd.undistort.redistort_image,
 * mtgs_amd.evaldump): what the evaluation dump in image_saving_mode = "nuplan" does on the host (scene_model/custom_pipeline.py:131-143)
 * with invert_distortion (utils/camera_utils.py:340-356): cv2.getOptimalNewCameraMatrix, cv2.initInverseRectificationMap and
 * cv2.remap(INTER_LINEAR) on the frame it took to the host and turned into bytes.  A header of its own, included by mtgs_rast.h; its
 * reviewed record is tests/golden/abi_signatures_redistort.txt.  Additive: it changed neither MTGS_RAST_ABI_VERSION nor
 * MTGS_RAST_HOT_ABI_VERSION.  Conventions (device pointers, `stream`, return codes, mtgs_rast_last_error) are mtgs_rast.h's.
 *
 * [RECALLED] cv2 was not available to run.  The rule below is OpenCV's as recalled, and it is THIS PROJECT'S DEFINITION: nothing
 * here claims byte equality with OpenCV.  tests/redistort_refs.py restates it in NumPy and tests/test_redistort_host.py pins it
 * with known answers that do not depend on the recall.
 *
 * cam: the same DEVICE double[MTGS_UNDISTORT_CAM_DOUBLES] as mtgs_undistort.h's = fx, fy, cx, cy (the raw camera, cx and cy half a
 * pixel smaller than the dataset's), fx', fy', cx', cy' (the new camera, WITHOUT the half pixel added back: what invert_distortion
 * passes), k1, k2, p1, p2, k3.  The roles are swapped: the image that is READ (h x w) has the new camera's geometry, the image that
 * is WRITTEN (oh x ow) the raw one's.
 *
 * The map of destination pixel (row i, column j) of the raw image, in fp64, ONE ROUNDING PER OPERATION (compiled with
 * -ffp-contract=off), in this order -- the fixed-point iteration of the inverse lens model, exactly mtgs_amd.undistort's
 * _undistort_points plus the folded-over rule:
 *   x0 = (j - cx) / fx        y0 = (i - cy) / fy          x = x0, y = y0
 *   repeat `iterations` times:
 *       r2 = x*x + y*y
 *       icdist = 1 / (1 + ((k3*r2 + k2)*r2 + k1)*r2)
 *       if icdist < 0:  x = x0, y = y0, stop                 [RECALLED: the model has folded over; per pixel]
 *       dx = 2*p1*x*y + p2*(r2 + 2*x*x)      dy = p1*(r2 + 2*y*y) + 2*p2*x*y          (products and sums left to right)
 *       x = (x0 - dx)*icdist      y = (y0 - dy)*icdist
 *   mapx = (float32)(fx'*x + cx')      mapy = (float32)(fy'*y + cy')
 * iterations lies in [0, MTGS_REDISTORT_MAX_ITERATIONS]; 0 is the plain change of camera.  There is NO convergence test.  5 is the
 * rule as recalled and the default of the Python layer, and it has NOT converged for a nuPlan-like lens: with D = (-0.356, 0.173,
 * -0.0002, 0.0003, -0.052), fx = fy = 1545, c = (959.5, 559.5) at 1920 x 1080, the forward model of mtgs_undistort.h applied to the
 * result misses the pixel it started from by at most
 *       iterations      5          10          20          40
 *       worst error     0.82 px    5.3e-3 px   2.2e-7 px   4e-13 px        (at the image corners; the mean at 5 is 0.026 px)
 * A NaN coefficient makes every map entry NaN (NaN < 0 is false: the iteration goes on), which is OUTSIDE below.
 *
 * Sampling is MTGS_UNDISTORT_LINEAR's rule, unchanged: sx = rint(mapx * 32.0f) in float32, ties to even; ix = sx >> 5, a = sx & 31
 * (y likewise); out = ((32-a)(32-b)*32 * s[iy, ix] + a(32-b)*32 * s[iy, ix+1] + (32-a)b*32 * s[iy+1, ix] + ab*32 * s[iy+1, ix+1]
 * + 16384) >> 15 per channel; each of the four taps on its own reads 0 outside the source; a coordinate f (float32, after rint)
 * with !(|f| < 2^30), non-finite ones included, is outside.
 *
 * src: uint8 (src_float = 0) or float32 (src_float = 1) [h, w, channels], channels 1 or 3, strides (row, column, channel) in
 * ELEMENTS of any value, also 0 or negative, as long as every element lies in the allocation.  A float32 tap is converted to a byte
 * BEFORE the interpolation, by the conversion mtgs_jpeg_encode applies on load (one device function serves both): NaN -> 0, clamp to
 * [0, 1], one correctly rounded product with 255, with conversion = MTGS_PRESENT_U8_ROUND one correctly rounded sum with 0.5, then
 * truncation (MTGS_PRESENT_U8_TRUNCATE is the evaluation dump's (x * 255).astype(uint8)).  dst: contiguous uint8 [oh, ow, channels].
 *
 * mtgs_redistort_frame: ONE launch; a workgroup of MTGS_UNDISTORT_TILE_W x MTGS_UNDISTORT_TILE_H threads owns a tile of that many
 * destination pixels, a wave is one row of 64 neighbours; a thread evaluates its map entry once, or reads it from `map` (float32
 * [oh, ow, 2] = (mapx, mapy), e.g. mtgs_redistort_map's or cv2's own) when that is not NULL -- then `cam` and `iterations` are not
 * used.  The loop count is an argument, so the loop is wave-uniform; the folded-over exit is per lane.  No atomics, no LDS, no host
 * read; capturable in a HIP graph, and a captured launch follows a `cam` written later.
 *
 * mtgs_redistort_map: map float32 [oh, ow, 2] = (mapx, mapy) of the rule above.
 *
 * NOT covered: INTER_CUBIC, more than five distortion coefficients, RGBA, a coverage mask of the pixels that read outside the
 * source, writing files and symbolic links, and fusing the remap into the JPEG encoder's first launch (the intermediate uint8 frame
 * is written once and read once: profiles/redistort.txt has what it costs).
 *
 * Limits: 1 <= h, w, oh, ow <= MTGS_UNDISTORT_MAX_SIZE.  The host checks name the bad argument. */
#define MTGS_REDISTORT_MAX_ITERATIONS 64

int mtgs_redistort_frame(int h, int w, int oh, int ow, const double *cam, int iterations, const float *map, const void *src,
                         int src_float, int conversion, int64_t stride_y, int64_t stride_x, int64_t stride_c, int channels,
                         uint8_t *dst, void *stream);
int mtgs_redistort_map(int oh, int ow, const double *cam, int iterations, float *map, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MTGS_REDISTORT_H */
