#ifndef MTGS_STACK_H
#define MTGS_STACK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- lidar sweeps stacked into a background cloud and one cloud per tracked object, on the device (mtgs_amd/csrc/stack.hip;
 * mtgs_amd.stack): StackRGBPointCloud (nuplan_scripts/stack_RGB_point_cloud.py:89-126, 153-183) with
 * extract_frame_background_instance_lidar and accumulate_background_box_point (nuplan_scripts/utils/stack_point_cloud_utils.py).
 * A header of its own, included by mtgs_rast.h; its reviewed record is tests/golden/abi_signatures_stack.txt.  Additive: it
 * changed neither MTGS_RAST_ABI_VERSION nor MTGS_RAST_HOT_ABI_VERSION.  Conventions (device pointers, `stream`, return codes,
 * mtgs_rast_last_error) are mtgs_rast.h's.
 *
 * All arithmetic is fp64, every operation rounded once (compiled with -ffp-contract=off).  points[N, 3] are float32
 * (points_f64 = 0; converted exactly) or float64 (points_f64 = 1) rows of stride row_stride ELEMENTS (>= 3).  A 3 x 4 matrix by
 * rows (12 float64 on the DEVICE) applied to (x, y, z) is, per row k, ((m_k0 x + m_k1 y) + m_k2 z) + m_k3.
 *
 * The boxes of a frame are B rows of five device arrays: lidar2box[B, 12] and box2lidar[B, 12] (3 x 4 by rows), half_tight[B, 3] =
 * size / 2, half_inflated[B, 3] = (size + fill) / 2, include[B] uint8 (NULL: every box counts).  The host builds them; the kernels
 * never see a box.
 *
 * The rule (the reference's sequential loop over the boxes, per point): of the included boxes in ascending order, q = lidar2box_b
 * applied to the point; the OWNER is the first box with |q_k| <= half_inflated_b[k] for k = 0, 1, 2.  If |q_k| <= half_tight_b[k]
 * holds as well the point is an instance point of b with box-frame coordinates q; otherwise it is DROPPED (it lies in the margin
 * of b and never reaches a later box).  A point without an owner is background.  Every <= is false on NaN.
 *   slot[i] = 0 background, 1 + b instance of box b, -1 dropped.
 *
 * mtgs_stack_split: classify (one lane per point, the box table staged through LDS MTGS_STACK_BOX_CHUNK boxes at a time, the loop
 *   over the boxes wave-uniform), a stable sort of (slot, index) with the u32 radix sort on ceil(log2(B + 2)) key bits (dropped
 *   points sort last), group offsets by a binary search per group, then one row move.
 *   out_points[N, 3] float64: the background rows as they came (converted to float64), then the box-frame rows of box 0, box 1, ...,
 *   indices ascending inside every group; the rows from offsets[B + 1] on (as many as were dropped) are zero.
 *   offsets[B + 2] int64 on the device: group g is rows [offsets[g], offsets[g + 1]), g = 0 the background; offsets[B + 1] = the
 *   number of points kept.  slot[N] int32 may be NULL.
 *
 * mtgs_stack_frame: the split, then the rows to paint (a background row itself; an instance row back through
 *   InstanceObject.points_ego, e_k = ((R_k0 q_0 + R_k1 q_1) + R_k2 q_2) + t_k with box2lidar: the reference paints the round-tripped
 *   point), mtgs_lidar_paint on them (mtgs_lidar.h: C, lidar2imgs, h, w, images, reverse_channels, masks as there, all required),
 *   then a stable compaction that keeps the rows some camera sees, group by group.
 *   out_points[N, 3] (background: lidar frame; instances: BOX frame), out_rgb[N, 3] float64, out_labels[N] int32 hold the kept rows;
 *   out_offsets[B + 2] int64 their groups; rows from out_offsets[B + 1] on are unspecified.
 *   bg_sel[N] int32: the ascending rows r < out_offsets[1] with out_labels[r] < label_cutoff; bg_kept[1] int64 their number (what
 *   the traversal keeps of this frame's background).
 *   No host read, no global atomics, no allocation: a frame can be captured in a HIP graph.  N = 0 and B = 0 are valid.
 *
 * mtgs_stack_plan / mtgs_stack_gather: the traversal.  frames[F] (device) describes the outputs of F mtgs_stack_frame calls and each
 *   frame's lidar2global.  Segment s (seg_frame[s], seg_slot[s], device int32[S]) is group seg_slot of frame seg_frame, listed in
 *   OUTPUT order: the backgrounds of the frames in frame order, then, track by track, the track's groups in frame order.  A
 *   background segment (slot 0) counts bg_kept rows, any other its group's rows.
 *   plan: prefix[S + 1] int64 = the exclusive prefix sum of the segment counts, prefix[S] the total: ONE scan.  The host reads the
 *   entries it needs to size the outputs (the only host read of a traversal).
 *   gather: one launch over `total` output rows (total <= prefix[S]; rows beyond it are not written).  A workgroup finds the segment
 *   of its first row by binary search in prefix and walks on from there.  A background row r of frame f is row bg_sel[r] of the
 *   frame through lidar2global_f, g_k = ((L_k0 x + L_k1 y) + L_k2 z) + L_k3; an instance row is copied.  xyz[total, 3], rgb[total, 3]
 *   float64, labels[total] int32.
 *
 * Limits: 0 <= N < 2^31; 0 <= B <= MTGS_STACK_MAX_BOXES; 0 <= S, F < 2^31; 0 <= total < 2^31.  The host checks name the bad
 * argument.  Workspaces are 16-byte aligned. */
#define MTGS_STACK_MAX_BOXES 1024
#define MTGS_STACK_BOX_CHUNK 64

typedef struct mtgs_stack_frame_desc {
    const double *points;   /* out_points of the frame */
    const double *rgb;      /* out_rgb */
    const int32_t *labels;  /* out_labels */
    const int64_t *offsets; /* out_offsets[B + 2] */
    const int32_t *bg_sel;
    const int64_t *bg_kept;
    int64_t groups;         /* B + 1: the slots a segment of this frame may name */
    double lidar2global[12];
} mtgs_stack_frame_desc;

int mtgs_stack_split_workspace_bytes(int64_t N, int B, size_t *bytes);
int mtgs_stack_split(int64_t N, const void *points, int points_f64, int64_t row_stride, int B, const double *lidar2box,
                     const double *half_tight, const double *half_inflated, const uint8_t *include, double *out_points,
                     int64_t *offsets, int32_t *slot, void *ws, size_t ws_bytes, void *stream);
int mtgs_stack_frame_workspace_bytes(int64_t N, int B, size_t *bytes);
int mtgs_stack_frame(int64_t N, const void *points, int points_f64, int64_t row_stride, int B, const double *lidar2box,
                     const double *box2lidar, const double *half_tight, const double *half_inflated, const uint8_t *include, int C,
                     const double *lidar2imgs, int h, int w, const uint8_t *images, int reverse_channels, const uint8_t *masks,
                     int label_cutoff, double *out_points, double *out_rgb, int32_t *out_labels, int64_t *out_offsets,
                     int32_t *bg_sel, int64_t *bg_kept, int32_t *slot, void *ws, size_t ws_bytes, void *stream);
int mtgs_stack_plan_workspace_bytes(int64_t S, size_t *bytes);
int mtgs_stack_plan(int64_t S, const int32_t *seg_frame, const int32_t *seg_slot, int64_t F, const mtgs_stack_frame_desc *frames,
                    int64_t *prefix, void *ws, size_t ws_bytes, void *stream);
int mtgs_stack_gather(int64_t S, const int32_t *seg_frame, const int32_t *seg_slot, int64_t F, const mtgs_stack_frame_desc *frames,
                      const int64_t *prefix, int64_t total, double *xyz, double *rgb, int32_t *labels, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MTGS_STACK_H */
