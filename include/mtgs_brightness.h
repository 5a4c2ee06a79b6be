#ifndef MTGS_BRIGHTNESS_H
#define MTGS_BRIGHTNESS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- camera brightness equalisation on the device (mtgs_amd/csrc/brightness.hip; mtgs_amd.brightness): adjust_brightness and
 * adjust_brightness_single_frame of nuplan_scripts/utils/nuplan_utils_custom.py:334-431 -- the V channel of every camera's image
 * scaled by one factor per camera (the dataset's `v_adjust_factors`, mtgs/dataset/custom_dataset.py:26-32, 90-92; the point stack,
 * stack_RGB_point_cloud.py:81-87), and the estimate of those factors from the lidar points two neighbouring cameras both see.  A
 * header of its own, included by mtgs_rast.h; its reviewed record is tests/golden/abi_signatures_brightness.txt.  Additive: it
 * changed neither MTGS_RAST_ABI_VERSION nor MTGS_RAST_HOT_ABI_VERSION.  Conventions (device pointers, `stream`, return codes,
 * mtgs_rast_last_error) are mtgs_rast.h's.
 *
 * ======== mtgs_brightness_adjust: cvtColor(RGB2HSV) -> V * factor -> cvtColor(HSV2RGB), 8 bit, per pixel, ONE launch ========
 *
 * [RECALLED] cv2 was not available to run.  The two colour conversions below are OpenCV's 8-bit ones as recalled, and they are THIS
 * PROJECT'S DEFINITION: nothing here claims byte equality with OpenCV.  tests/brightness_refs.py restates the rule in NumPy and
 * pins it with known answers that do not depend on the recall.  The scaling in the middle is the reference's own NumPy line.
 * NOT covered: decoding PNG files, RGBA images, COLOR_*2HSV_FULL (H in 0..255) and the float HSV conversions, changes of hue or
 * saturation.
 *
 * The rule for a pixel (r, g, b) of bytes; bgr != 0 swaps the first and the third channel on the way in and on the way out.
 *
 * RGB -> HSV [RECALLED], integer arithmetic with hsv_shift = 12 and the tables, for i = 1 .. 255,
 *   sdiv[i] = rint((255 << 12) / (double)i)      hdiv[i] = rint((180 << 12) / (6.0 * i))      sdiv[0] = hdiv[0] = 0
 * (rint: ties to even, of the double quotient; built at compile time):
 *   v = max(r, g, b); vmin = min(r, g, b); d = v - vmin
 *   s = (d * sdiv[v] + 2048) >> 12
 *   h = (v == r) ? g - b : (v == g) ? b - r + 2*d : r - g + 4*d            (that order of tests)
 *   h = (h * hdiv[d] + 2048) >> 12                                         (an arithmetic shift of a negative product)
 *   if h < 0: h += 180
 * so that 0 <= h < 180 and 0 <= s <= 255.  H and S pass through as those bytes.
 *
 * The scaling (the reference's): V' = (uint8) trunc(min(max((double)v * factor, 0.0), 255.0)) in fp64.  A NaN product (a NaN
 * factor, or 0 * inf) gives V' = 0: the defined deviation, NumPy's cast of NaN being undefined.
 *
 * HSV -> RGB [RECALLED], fp32, ONE ROUNDING PER OPERATION (compiled with -ffp-contract=off), in this order:
 *   hf = (float)h * (float)(6.0 / 180.0); sf = (float)s * (1.0f / 255.0f); vf = (float)V' * (1.0f / 255.0f)
 *   if s == 0: r = g = b = vf
 *   else:
 *     sector = floor(hf); f = hf - sector                                  (h < 180, so 0 <= sector <= 5)
 *     tab = { vf, vf*(1 - sf), vf*(1 - sf*f), vf*(1 - sf*(1 - f)) }
 *     (b, g, r) = tab[ {1,3,0}, {1,0,2}, {3,0,1}, {0,2,1}, {0,1,3}, {2,1,0} ][sector]
 *   byte = clamp(rint(x * 255.0f), 0, 255), ties to even
 * Factor 1.0 is NOT the identity (the round trip changes a channel by up to 5); it runs whatever the factor, as the reference's.
 * The largest channel of the result is V' for every colour, and a gray stays gray.
 *
 * src: uint8, C images of h x w pixels of 3 channels, strides (image, row, column, channel) in BYTES, any value (also 0 or
 * negative, any alignment) as long as every element lies in the allocation.  factors: DEVICE double, image c reads
 * factors[c * factor_stride] (factor_stride 0: one factor for all), read by the kernel so that a captured launch follows a factor
 * written later and the estimate's output feeds it with no host read.  dst: contiguous [C, h, w, 3], uint8 (out_float = 0) or
 * float32 (out_float = 1: (float)byte / 255.0f, one correctly rounded division); it must not overlap src.
 *
 * Two paths that give the same bytes.  DWORD: when every image is contiguous and dword-aligned (channel stride 1, column stride 3,
 * row stride 3 w, src, dst and the image stride multiples of 4 -- of 16 for a float32 dst --, and C == 1 or h w a multiple of 4), a
 * thread takes 4 pixels as three dword loads and three dword stores (three 16-byte stores with out_float); the h w % 4 last pixels
 * go byte by byte.  STRIDED: every other layout, one pixel per thread, byte by byte.  force_strided != 0 takes the strided path on
 * any layout (measurements, tests).  No LDS, no atomics, no host read, capturable in a HIP graph.
 *
 * ======== mtgs_brightness_estimate: adjust_brightness_single_frame, three launches, fp64 with integer sums ========
 *
 * Nothing recalled: of the HSV conversion the reference reads V only, and V = max(R, G, B).
 *
 * pairs: DEVICE int32 [P, 3] = (cam1, cam2, side), in the order the chain walks them.  side 0: the fallback strips are the LEFT
 * `strip` columns of cam1 ([:, :strip]) and the RIGHT ones of cam2 ([:, -strip:]); side 1 the reverse.  The slices are Python's: a
 * strip of an image with w < strip is the whole image.  images uint8 [C, h, w, 3] contiguous, any channel order (a max does not
 * care); points and lidar2imgs as mtgs_lidar_paint takes them.
 *
 * 1 strips: for every pair and both of its cameras, partial sums of V = max of the three bytes over the strip's pixels, row slab by
 *   row slab, into ws; also clears the overlap sums.
 * 2 sample: one thread per point, the cameras in ascending order; projection, `see` test and bilinear sample EXACTLY
 *   mtgs_lidar_paint's (one shared body, csrc/lidar_sample.hpp); per seeing camera V = max_k (uint8) trunc(value_k * 255.0).  For
 *   every pair a point both cameras see adds 1 to n[p], its V in cam1 to s1[p], its V in cam2 to s2[p]: reduced over the
 *   workgroup, then one integer atomicAdd per sum.  Integers below 2^39: any order gives the same bits.  Skipped when N = 0.
 * 3 solve: one thread, the reference's chain in fp64 in its order.  has = {camera 0}, factor[0] = 1.0.  For p = 0 .. P - 1:
 *     (a, na, b, nb) = (s1, n, s2, n) if n[p] >= min_overlap else (strip1, h * min(strip, w), strip2, the same count)
 *     v_ratio = (a / na) / (b / nb)                     (np.mean of integers below 2^53 is their exact sum over their count)
 *     base = factor[cam1] if cam1 in has else 1.0;  ratio = base * v_ratio
 *     factor[cam2] = ratio if cam2 not in has else (factor[cam2] + ratio) / 2;  has += {cam2}
 *   A camera no pair reaches keeps 1.0 (the defined deviation: the reference raises KeyError).  Then every factor is divided by
 *   mean = np.mean(factors) = sum / C with NumPy's pairwise sum of a contiguous array: for C < 8 left to right from 0.0, else r[j]
 *   = a[j] (j < 8), r[j] += a[i + j] for i = 8, 16, .. while i + 8 <= C, ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then
 *   the C % 8 last ones left to right.  A zero mean or an all-black strip gives inf or NaN as IEEE has it.
 *
 * factors: double [C].  stats: int64 [P, 5] = n, s1, s2, strip1, strip2 per pair (always written: it holds the sums).  ws:
 * mtgs_brightness_estimate_workspace_bytes(P) bytes, 8-byte aligned.  No host read, no float atomics, bitwise reproducible,
 * capturable in a HIP graph.
 *
 * Limits: 1 <= C <= MTGS_BRIGHTNESS_MAX_IMAGES (adjust) or MTGS_BRIGHTNESS_MAX_CAMERAS (estimate); 1 <= h, w and h * w < 2^31;
 * 0 <= N < 2^31; 1 <= P <= MTGS_BRIGHTNESS_MAX_PAIRS; strip >= 1; min_overlap >= 0.  The host checks name the bad argument; the pair
 * table is on the device and is the caller's to check (mtgs_amd.brightness.pair_table does). */
#define MTGS_BRIGHTNESS_MAX_IMAGES 65535
#define MTGS_BRIGHTNESS_MAX_CAMERAS 16
#define MTGS_BRIGHTNESS_MAX_PAIRS 64
#define MTGS_BRIGHTNESS_STRIP_SLABS 16

int mtgs_brightness_adjust(int C, int h, int w, const uint8_t *src, int64_t image_stride, int64_t row_stride, int64_t col_stride,
                           int64_t channel_stride, const double *factors, int64_t factor_stride, int bgr, int out_float,
                           int force_strided, void *dst, void *stream);
int mtgs_brightness_estimate_workspace_bytes(int P, size_t *bytes);
int mtgs_brightness_estimate(int64_t N, const void *points, int points_f64, int64_t row_stride, int C, const double *lidar2imgs,
                             int h, int w, const uint8_t *images, int P, const int32_t *pairs, int strip, int min_overlap,
                             double *factors, int64_t *stats, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MTGS_BRIGHTNESS_H */
