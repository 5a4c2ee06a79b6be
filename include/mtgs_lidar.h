#ifndef MTGS_LIDAR_H
#define MTGS_LIDAR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- lidar sweeps through the cameras on the device (mtgs_amd/csrc/lidar.hip; mtgs_amd.lidar): the sparse lidar depth image of a
 * training frame (CustomInputDataset._get_depth_from_lidar, mtgs/dataset/custom_dataset.py:175-201) and the colours and semantic
 * labels of the seeding cloud (get_rgb_point_cloud, mtgs/utils/nuplan_pointcloud.py:28-60; get_semantic_point_cloud,
 * nuplan_scripts/utils/nuplan_utils_custom.py:208-265).  A header of its own, included by mtgs_rast.h; its reviewed record is
 * tests/golden/abi_signatures_lidar.txt.  Additive: it changed neither MTGS_RAST_ABI_VERSION nor MTGS_RAST_HOT_ABI_VERSION.
 * Conventions (device pointers, `stream`, return codes, mtgs_rast_last_error) are mtgs_rast.h's.
 *
 * All arithmetic is fp64, every operation rounded once (compiled with -ffp-contract=off).  points[N, 3] are float32
 * (points_f64 = 0; converted exactly) or float64 (points_f64 = 1) rows of stride row_stride ELEMENTS (>= 3), the three
 * coordinates contiguous.  A point is x = (x0, x1, x2); a matrix row m applied to it is ((m0 x0 + m1 x1) + m2 x2) + m3.
 * Matrices are float64 on the DEVICE, 3 x 4 by rows (12 values); they are read through uniform loads.
 *
 * mtgs_lidar_depth: depth[h, w] float32 and, if index is not NULL, index[h, w] int32.
 *   cam_r = row r of lidar2cam applied to x; the point is kept if cam_2 > 0
 *   q_r   = (K[r][0] cam_0 + K[r][1] cam_1) + K[r][2] cam_2 for K[3, 3] by rows (9 values)
 *   u = q_0 / q_2, v = q_1 / q_2; kept if v >= 0, v < h, u >= 0, u < w (all false on NaN); only then the pixel ((int)u, (int)v)
 *   a pixel takes (float)q_2 of the LARGEST point index that lands in it (NumPy's fancy assignment: the last one wins), times
 *   `scale` in fp32; a pixel no point lands in is 0.0f and its index -1.
 *   Launches: clear (ws[pixel] = -1), scatter (one thread per point, a vector atomicMax of the point's index on ws[pixel]:
 *   order-independent), resolve (one thread per pixel recomputes q_2 of the winner).  No host read, no float atomics, bitwise
 *   reproducible, capturable in a HIP graph.  ws: mtgs_lidar_depth_workspace_bytes(h, w) bytes (h * w int32), 4-byte aligned.
 *
 * mtgs_lidar_paint: one launch, one thread per point, the cameras c = 0 .. C - 1 in ascending order inside the thread.
 *   p_r = row r of lidar2imgs[c] applied to x; see = p_2 > 0.1; z = min(max(p_2, 1e-5), 99999)
 *   nx = (p_0 / z) / w, ny = (p_1 / z) / h; see &= nx < 1 & nx >= 0 & ny < 1 & ny >= 0
 *   ix = (((nx 2 - 1) + 1) / 2) (w - 1), iy likewise with h (grid_sample's align_corners = True)
 *   colour (images[C, h, w, 3] uint8, not NULL): x0 = floor(ix), fx = ix - x0, y0 and fy likewise; a texel is byte / 255.0;
 *     value = t00 ((1 - fx)(1 - fy)) + t01 (fx (1 - fy)) + t10 ((1 - fx) fy) + t11 (fx fy), summed left to right, t01 the
 *     neighbour in x and t10 the neighbour in y (clamped to the image, where its weight is 0); the running sum over the seeing
 *     cameras in camera order is divided once by their count; rgb[N, 3] float64 is 0 where no camera sees the point;
 *     reverse_channels != 0 writes channel 2 - k of the image to rgb[.., k] (BGR images)
 *   label (masks[C, h, w] uint8, not NULL): the texel at (nearbyint(iy), nearbyint(ix)), ties to even, of the FIRST camera
 *     that sees the point; labels[N] int32 is 0 where none does
 *   count[N] int32 = the number of cameras that see the point; fov[N] uint8 = count > 0.
 *   rgb may be NULL iff images is, labels iff masks is.  The projection is done once for both.
 *
 * Limits: 0 <= N < 2^31 (N = 0: the depth image is all zeros, paint does nothing); 1 <= h, w and h * w < 2^31; 1 <= C <=
 * MTGS_LIDAR_MAX_CAMERAS.  The host checks name the bad argument. */
#define MTGS_LIDAR_MAX_CAMERAS 64

int mtgs_lidar_depth_workspace_bytes(int h, int w, size_t *bytes);
int mtgs_lidar_depth(int64_t N, const void *points, int points_f64, int64_t row_stride, const double *lidar2cam, const double *K,
                     int h, int w, float scale, float *depth, int32_t *index, void *ws, size_t ws_bytes, void *stream);
int mtgs_lidar_paint(int64_t N, const void *points, int points_f64, int64_t row_stride, int C, const double *lidar2imgs, int h,
                     int w, const uint8_t *images, int reverse_channels, const uint8_t *masks, double *rgb, int32_t *labels,
                     uint8_t *fov, int32_t *count, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MTGS_LIDAR_H */
