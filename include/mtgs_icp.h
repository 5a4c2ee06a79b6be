#ifndef MTGS_ICP_H
#define MTGS_ICP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- lidar sweeps registered against a local voxel map on the device (mtgs_amd/csrc/icp.hip; mtgs_amd.registration): the KISS-ICP
 * odometry of nuplan_scripts/lidar_registration_multi_traversal.py (thirdparty/kiss-icp: Preprocessing, VoxelUtils, VoxelHashMap,
 * Registration) in a CANONICAL ORDER of this project's own.  A header of its own, included by mtgs_rast.h; its reviewed record is
 * tests/golden/abi_signatures_icp.txt.  Additive: it changed neither MTGS_RAST_ABI_VERSION nor MTGS_RAST_HOT_ABI_VERSION.
 * Conventions (device pointers, `stream`, return codes, mtgs_rast_last_error) are mtgs_rast.h's.
 *
 * Nothing here is compared with the kiss-icp binary (it needs Eigen, Sophus, TBB and tsl::robin_map).  The reference returns a
 * down-sampled cloud in the iteration order of a hash map and sums under tbb::parallel_reduce, so its own result changes from
 * run to run; the canonical order below is pinned by the NumPy restatement tests/icp_refs.py instead, bit for bit wherever no
 * sin / cos is involved.
 *
 * All arithmetic is fp64, every operation rounded once (compiled with -ffp-contract=off).  Point rows are float32 (f64 = 0,
 * converted exactly) or float64 (f64 = 1) of stride row_stride ELEMENTS (>= 3).  A 3 x 4 matrix by rows (12 float64 on the DEVICE)
 * applied to (x, y, z) is, per row k, ((m_k0 x + m_k1 y) + m_k2 z) + m_k3.  sq(a, b) of two points is, with d = a - b per axis,
 * (d_x d_x + d_y d_y) + d_z d_z.
 *
 * Voxels.  The voxel of p at size s is v_k = floor(p_k / s): an fp64 division, then floor.  Its key is
 * ((v_x + 2^20) << 42) | ((v_y + 2^20) << 21) | (v_z + 2^20); a point with some v_k outside [-2^20, 2^20) (a NaN among them) sets
 * status bit MTGS_ICP_OUT_OF_GRID and takes no further part.
 *
 * mtgs_icp_downsample: points[N, 3] -> frame[<= N, 3] and source[<= N, 3] float64.
 *   kept      : min_range < sqrt((x x + y y) + z z) < max_range
 *   level one : of the kept points, the one of least input index in every voxel of size 0.5 voxel_size, in ascending input index
 *               (`frame`, counts[0] rows; frame_index[N] int32, nullable: their input indices)
 *   level two : the same rule at size 1.5 voxel_size over `frame` in that order (`source`, counts[1] rows; source_index[N] int32,
 *               nullable: input indices again)
 *   Per level: keys, the stable 64-bit pair sort of (key, index), heads of runs flagged back at their index, one scan, one gather.
 *   counts[2] int64 and status[1] int32 stay on the device; rows beyond the counts are unspecified.
 *
 * The map.  One device allocation of mtgs_icp_map_bytes(capacity, max_points) bytes, set up by mtgs_icp_map_init: a table of
 * (key, slot) sorted by key, a point list of at most max_points (<= MTGS_ICP_MAX_POINTS) float64 points per slot, and state[4] int64
 * at its start: {voxels in the table, status bits, voxels that hold a point, the side of the table in use}.
 *   insert : every offered point (through `pose`, a 3 x 4 on the device, when given) gets its voxel at voxel_size; (key, offered
 *            index) go through the stable pair sort; the voxels that are not in the table are merged into it by rank (two binary
 *            searches per entry, no atomics) and take the next slots in ascending key; then ONE LANE PER TOUCHED VOXEL walks its
 *            offered points in offered order: a point is dropped when the list holds max_points, or when some held point q has
 *            sqrt(sq(q, p)) < sqrt(voxel_size voxel_size / max_points); otherwise appended.  If the new voxels do not fit, status
 *            bit MTGS_ICP_MAP_FULL is set and the map is left exactly as it was.
 *   prune  : a voxel whose FIRST point q has sq(q, origin) >= max_distance max_distance is emptied.  It keeps its key and slot and
 *            behaves like an absent voxel from then on; a later insert fills it again from empty.
 *   export : the points by ascending key, then list order; total[1] int64 on the device.
 *   The contents are a function of the sequence of inserts and prunes alone: per voxel an ordered list.
 *
 * One ICP iteration is two launches over source[S, 3] (a working copy in the workspace, made by mtgs_icp_align_begin through the
 * initial guess) and record[MTGS_ICP_RECORD] float64 on the device:
 *   record[0..11]  T_icp, 3 x 4 by rows      record[12..23] the increment the next association applies first
 *   record[24] |dx|   record[25] iterations run   record[26] correspondences of the last iteration   record[27] status bits
 *   record[28..55] the 28 sums of the last iteration, in the order below
 * associate (one lane per source point): p <- increment applied to p, in place.  The 27 voxels around the voxel of p are searched
 *   in the order i, j, k from -1 to +1 (x outermost), each in list order; the nearest neighbour q minimises sqrt(sq(q, p)) with
 *   strict <, so the first of equal distances wins.  It is a correspondence when that distance < max_distance, strictly.  With
 *   r = p - q, r2 = (r_x r_x + r_y r_y) + r_z r_z, w = (k k) / ((k + r2) (k + r2)) for the kernel scale k, u = w r per axis, and
 *   s = p, its 28 contributions are
 *     0: w          1: w          2: w                                  JTJ (0,0) (1,1) (2,2)
 *     3: w s_z      4: -(w s_y)   5: -(w s_z)   6: w s_x   7: w s_y   8: -(w s_x)      JTJ (0,4) (0,5) (1,3) (1,5) (2,3) (2,4)
 *     9: w (s_y s_y + s_z s_z)   10: -(w (s_x s_y))   11: -(w (s_x s_z))               JTJ (3,3) (3,4) (3,5)
 *    12: w (s_x s_x + s_z s_z)   13: -(w (s_y s_z))   14: w (s_x s_x + s_y s_y)        JTJ (4,4) (4,5) (5,5)
 *    15..20: 0                                              JTJ (0,1) (0,2) (1,2) (0,3) (1,4) (2,5), identically zero, not summed
 *    21: u_x   22: u_y   23: u_z   24: s_y u_z - s_z u_y   25: s_z u_x - s_x u_z   26: s_x u_y - s_y u_x      JTr
 *    27: 1                                                                                                   the count
 *   (J = [I | -hat(s)], JTJ = J^T w J, JTr = J^T w r.)  A lane without a correspondence contributes zeros.  Every column is summed
 *   over the block of MTGS_ICP_BLOCK lanes by the halving tree of block_tree_sum_f64 (lds[t] += lds[t + o], o = 128, 64, ..., 1).
 * finish (one workgroup): thread t adds the partials of blocks t, t + 256, ... in that order to 0, the same tree sums the threads.
 *   Then JTJ dx = -JTr by LDL^T without pivoting, j = 0..5:
 *     d_j = A_jj - sum_{k<j} L_jk (L_jk d_k);   L_ij = (A_ij - sum_{k<j} L_ik (L_jk d_k)) / d_j   (k ascending, each term subtracted
 *     in turn);   y_i = b_i - sum_{k<i} L_ik y_k;   z_i = y_i / d_i;   dx_i = z_i - sum_{k>i} L_ki dx_k  (i descending, k ascending).
 *   E = SE3::exp(dx), dx = (upsilon, omega), in closed form: t2 = (o_x o_x + o_y o_y) + o_z o_z, t = sqrt(t2);
 *     t2 < 1e-8: A = 1 - t2 / 6, B = 0.5 - t2 / 24, C = 1 / 6 - t2 / 120;  else A = sin t / t, B = (1 - cos t) / t2,
 *     C = (t - sin t) / (t2 t);  with W = hat(omega), W2_ab = o_a o_b - (a == b ? t2 : 0):  R = I + (A W + B W2),
 *     V = I + (B W + C W2), each entry (a == b ? 1 : 0) + (A W_ab + B W2_ab);  translation_a = (V_a0 u_x + V_a1 u_y) + V_a2 u_z.
 *   T_icp <- E T_icp (rotation entries (e_0 m_0 + e_1 m_1) + e_2 m_2, translation that sum + the translation of E), increment <- E,
 *   |dx| = sqrt of the six squares added in order, iterations += 1; status bit MTGS_ICP_CONVERGED when |dx| < convergence.
 *   With no correspondence, or a dx that is not finite, status bit MTGS_ICP_DEGENERATE is set and T_icp is left as it was (the
 *   reference would go on with NaN poses: a defined deviation).  A map without a point sets MTGS_ICP_EMPTY_MAP before anything else.
 *   Once a status bit is set every later launch returns at its first instruction: mtgs_icp_align_iterate launches `iterations`
 *   pairs back to back, and the host reads the record once per such group.
 * mtgs_icp_associate: one association of source as given (no increment) with the per-point results for the tests: nn_index[S] int32
 *   = 32 (9 (i + 1) + 3 (j + 1) + (k + 1)) + list position, -1 without a neighbour; distance[S] float64 (DBL_MAX without);
 *   mask[S] uint8 the correspondences; sums[28].
 *
 * No allocation, no host read, no floating-point atomics; every result is bitwise reproducible from run to run.
 * Limits: 0 <= N, M, S < 2^31; 1 <= capacity < 2^31; 1 <= max_points <= MTGS_ICP_MAX_POINTS.  Workspaces are 16-byte aligned. */
#define MTGS_ICP_MAX_POINTS 32
#define MTGS_ICP_BLOCK 256
#define MTGS_ICP_RECORD 64
#define MTGS_ICP_SUMS 28
#define MTGS_ICP_GRID_BITS 21

#define MTGS_ICP_OUT_OF_GRID 1   /* downsample status[0] and map state[1] */
#define MTGS_ICP_MAP_FULL 2      /* map state[1] */

#define MTGS_ICP_CONVERGED 1     /* record[27] */
#define MTGS_ICP_DEGENERATE 2
#define MTGS_ICP_EMPTY_MAP 4

int mtgs_icp_downsample_workspace_bytes(int64_t N, size_t *bytes);
int mtgs_icp_downsample(int64_t N, const void *points, int points_f64, int64_t row_stride, double min_range, double max_range,
                        double voxel_size, double *frame, double *source, int32_t *frame_index, int32_t *source_index,
                        int64_t *counts, int32_t *status, void *ws, size_t ws_bytes, void *stream);

int mtgs_icp_map_bytes(int64_t capacity, int max_points, size_t *bytes);
int mtgs_icp_map_init(void *map, size_t map_bytes, int64_t capacity, int max_points, void *stream);
int mtgs_icp_map_insert_workspace_bytes(int64_t M, size_t *bytes);
int mtgs_icp_map_insert(void *map, int64_t capacity, int max_points, double voxel_size, int64_t M, const void *points,
                        int points_f64, int64_t row_stride, const int64_t *m_dev, const double *pose, void *ws, size_t ws_bytes,
                        void *stream);
int mtgs_icp_map_prune(void *map, int64_t capacity, int max_points, const double *origin, double max_distance, void *stream);
int mtgs_icp_map_export_workspace_bytes(int64_t capacity, size_t *bytes);
int mtgs_icp_map_export(const void *map, int64_t capacity, int max_points, int64_t rows, double *out, int64_t *total, void *ws,
                        size_t ws_bytes, void *stream);

int mtgs_icp_align_workspace_bytes(int64_t S, size_t *bytes);
int mtgs_icp_align_begin(int64_t S, const void *source, int source_f64, int64_t row_stride, const int64_t *s_dev,
                         const double *guess, double *record, void *ws, size_t ws_bytes, void *stream);
int mtgs_icp_align_iterate(const void *map, int64_t capacity, int max_points, double voxel_size, int64_t S, const int64_t *s_dev,
                           double max_distance, double kernel_scale, double convergence, int iterations, double *record, void *ws,
                           size_t ws_bytes, void *stream);
int mtgs_icp_associate(const void *map, int64_t capacity, int max_points, double voxel_size, int64_t S, const void *source,
                       int source_f64, int64_t row_stride, double max_distance, double kernel_scale, int32_t *nn_index,
                       double *distance, uint8_t *mask, double *sums, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MTGS_ICP_H */
