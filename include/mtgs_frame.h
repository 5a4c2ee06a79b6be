#ifndef MTGS_FRAME_H
#define MTGS_FRAME_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- training frames at a stage's resolution on the device (mtgs_amd/csrc/frame.hip; mtgs_amd.frame): what
 * CustomInputDataset._resize_data (mtgs/dataset/custom_dataset.py:279-304) does with up to five Pillow resizes on the host, and the
 * mask preparation that feeds them (:203-274).  A header of its own, included by mtgs_rast.h; its reviewed record is
 * tests/golden/abi_signatures_frame.txt.  Additive: it changed neither MTGS_RAST_ABI_VERSION nor MTGS_RAST_HOT_ABI_VERSION.
 * Conventions (device pointers, `stream`, return codes, mtgs_rast_last_error) are mtgs_rast.h's.  Covered: Pillow's BILINEAR
 * resampling of 8-bit and of float32 ("F") images, its NEAREST resampling, and the masks of NumPy's rules below.  NOT covered:
 * decoding the depth PNG, RGBA (Pillow premultiplies it around the resize); cv2.remap undistortion is mtgs_undistort.h, adjust_brightness mtgs_brightness.h.
 *
 * Tables.  Every resampler reads HOST-built tables that live on the device (mtgs_amd.frame builds and keeps them per shape).
 *   bounds[n_out][2] int32 = (first source index, taps) of one axis; coef[n_out][ksize] its taps' coefficients, ksize >= every
 *   taps.  8-bit: int32 coefficients, Pillow's normalize_coeffs_8bpc, 22 fractional bits.  float32: the normalised double weights
 *   of precompute_coeffs, NOT quantised.  A kernel clamps (first, taps) to the source before it follows them.
 *   sy[oh], sx[ow] int32: the source row / column of Pillow's NEAREST (repeated addition in double), clamped likewise.
 *
 * mtgs_frame_resize_u8: src uint8 [h, w, c], c = 1 .. 3, strides in ELEMENTS (any, also 0 or negative as long as every element
 * lies in the allocation) -> dst [oh, ow, c] contiguous, uint8 (out_float = 0) or float32 (out_float = 1: (float)byte / 255.0f,
 * one correctly rounded division).  ImagingResample, exactly: the horizontal pass first, each value
 *   clip8((2^21 + sum_i k_i px_i) >> 22)            (int32; >> arithmetic; clip8 to [0, 255])
 * ROUNDED TO uint8, then the vertical pass by the same formula over the rounded rows.  A pass whose size does not change
 * (w == ow, resp. h == oh) is the identity and reads no table.
 *
 * mtgs_frame_resize_f32: src float32 [h, w, c] likewise -> dst float32 [oh, ow, c].  Per value ss = 0.0; ss += (double)px_i * k_i
 * in tap order in double, every product and every sum rounded once (compiled with -ffp-contract=off: (double)float * double is
 * not exact, a fused multiply-add changes bits); the horizontal result is rounded to float32 before the vertical pass, whose
 * result is rounded to float32 again.  An identity pass copies the bits.
 *
 * Both: ONE launch.  A workgroup of 512 threads owns an output tile of MTGS_FRAME_TILE_W x MTGS_FRAME_TILE_H pixels; it walks
 * the source rows its tile needs in chunks of MTGS_FRAME_CHUNK_ROWS, filters each chunk horizontally into LDS (rounded) and adds
 * the chunk's vertical taps to its outputs' accumulators in ascending row order, so that tap counts are unbounded in both
 * directions (400 -> 3 has 266) and the two rounding points are Pillow's.  Rows whose pixels are contiguous (stride_c = 1,
 * stride_w = c) and whose tile reads at most MTGS_FRAME_RAW_ROW_BYTES - 8 bytes of a row are staged into LDS by aligned dword
 * loads (which, for 8-bit rows, may touch up to 3 bytes on either side of the row's span, inside the same aligned dword); any
 * other layout is read element by element.  The tile's rows of the tables are kept in LDS when a filter has at most 8 taps.
 * Calling it twice (h, w -> h, ow -> oh, ow) gives the two-launch form with an intermediate image; the results are the same
 * bytes (profiles/frame.txt has both timed).  No atomics, no host read, capturable in a HIP graph.
 *
 * mtgs_frame_nearest: n_planes <= MTGS_FRAME_MAX_PLANES planes of one source size h x w to one size oh x ow in ONE launch, from a
 * HOST array of mtgs_frame_plane (copied into the launch) and a HOST 256-bit label set labels[32] (label l is bit l & 7 of
 * byte l >> 3; NULL = empty).  With (ys, xs) = (sy[y], sx[x]) and valid = (valid == NULL || valid[ys, xs] != 0):
 *   MTGS_FRAME_COPY      dst[y, x, k] = src[ys, xs, k], k < channels, elem_bytes 1 (uint8, bool) or 4 (int32); valid ignored
 *   MTGS_FRAME_INSTANCE  dst int32 [oh, ow] = valid ? src[ys, xs, 0] + 256 * src[ys, xs, 1] : 0          (src uint8, panoptic)
 *   MTGS_FRAME_SEMANTIC  dst uint8 [oh, ow] = valid ? src[ys, xs, 0] : 255                                (src uint8)
 *   MTGS_FRAME_MASK      dst uint8 [oh, ow] = valid && !(src[ys, xs, 0] in labels) ? 1 : 0                (src uint8)
 * (a pointwise rule commutes with a gather: this equals "prepare at full size, then resize"; the semantic channel of a panoptic
 * map is src + 2 channel strides).  dst is contiguous; src_stride = (row, column, channel) and valid_stride = (row, column) in
 * ELEMENTS.  One thread per output pixel and plane.
 *
 * Limits: 1 <= h, w, oh, ow <= MTGS_FRAME_MAX_SIZE; 1 <= c, channels <= 3.  The host checks name the bad argument. */
#define MTGS_FRAME_TILE_W 64
#define MTGS_FRAME_TILE_H 16
#define MTGS_FRAME_CHUNK_ROWS 40
#define MTGS_FRAME_RAW_ROW_BYTES 640
#define MTGS_FRAME_MAX_PLANES 8
#define MTGS_FRAME_MAX_SIZE 1048576
enum { MTGS_FRAME_COPY = 0, MTGS_FRAME_INSTANCE = 1, MTGS_FRAME_SEMANTIC = 2, MTGS_FRAME_MASK = 3 };

typedef struct mtgs_frame_plane {
    const void *src;
    const uint8_t *valid;
    void *dst;
    int64_t src_stride[3];
    int64_t valid_stride[2];
    int32_t op, elem_bytes, channels, reserved;
} mtgs_frame_plane;

int mtgs_frame_resize_u8(int h, int w, int c, const uint8_t *src, int64_t stride_h, int64_t stride_w, int64_t stride_c, int oh,
                         int ow, const int32_t *hbounds, const int32_t *hcoef, int hk, const int32_t *vbounds, const int32_t *vcoef,
                         int vk, int out_float, void *dst, void *stream);
int mtgs_frame_resize_f32(int h, int w, int c, const float *src, int64_t stride_h, int64_t stride_w, int64_t stride_c, int oh,
                          int ow, const int32_t *hbounds, const double *hcoef, int hk, const int32_t *vbounds, const double *vcoef,
                          int vk, float *dst, void *stream);
int mtgs_frame_nearest(int h, int w, int oh, int ow, const int32_t *sy, const int32_t *sx, int n_planes,
                       const mtgs_frame_plane *planes, const uint8_t *labels, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MTGS_FRAME_H */
