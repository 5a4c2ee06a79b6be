#ifndef MTGS_CROP_H
#define MTGS_CROP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- rendering inside an oriented crop box (mtgs_amd/csrc/crop.hip): MTGSSceneModel.get_gaussians / get_gaussian_params
 * (mtgs_scene_graph.py:457-459, 493-495) -- `crop_ids = crop_box.within(means)`, then `v[crop_ids]` per collected tensor.
 * Additive block: it changed neither MTGS_RAST_ABI_VERSION nor MTGS_RAST_HOT_ABI_VERSION (no existing kernel or signature changes).
 * It is a header of its own, included by mtgs_rast.h: tests/golden/abi_signatures.txt is the reviewed record of mtgs_rast.h's
 * own declarations, and this block has its record in tests/golden/abi_signatures_crop.txt.  Conventions (device pointers
 * unless marked HOST, `stream`, return codes, mtgs_rast_last_error) are mtgs_rast.h's.
 * mtgs_crop_select: means: rows of three floats, row_stride floats apart (>= 3), so a [N, 4][:, :3] view is read in place.
 *   box: 15 HOST floats = the 3x4 world->box matrix m by rows, then the half sizes h[3].  For row i, p = (x, y, z),
 *     q_k = ((m_k0 * x + m_k1 * y) + m_k2 * z) + m_k3     in fp32, in that order, every operation rounded once,
 *   and the row is kept iff -h_k < q_k && q_k < h_k for k = 0..2: both comparisons strict, so a NaN coordinate drops the row
 *   and h_k = 0 keeps nothing.  keep_ids (int32, [N] capacity) = the kept row indices in ASCENDING order (the order of a
 *   boolean-mask index, which keeps a render of the compacted set bit-identical); count (DEVICE int64 [1], 8-byte aligned) =
 *   their number; mask (u8 [N], nullable) = 1 where kept, else 0; keep_ids beyond count is not written.
 *   ws: mtgs_crop_workspace_bytes(N) bytes, 8-byte aligned, no initialisation.  0 <= N < 2^31; N = 0 writes count = 0 and
 *   nothing else.  Three launches (mtgs_scan_*'s prefix sum with the decision as its value); no atomics, no allocation, no
 *   host read: bitwise reproducible and graph-capturable.
 * mtgs_crop_gather: dst_j[r, :] = src_j[keep_ids[r], :] for r < n_keep and j < n_tensors, ONE launch for the whole table.
 *   src, dst: HOST arrays of n_tensors DEVICE addresses (4-byte aligned; rows contiguous and row_bytes[j] apart, dst_j with
 *   room for n_keep rows); row_bytes: HOST array, each a multiple of 4 in [4, 2^30] (a float row of any width, an int64 as
 *   8 bytes).  The table travels as a kernel argument: nothing is uploaded.  1 <= n_tensors <= 16; n_keep (HOST: the caller
 *   has read count to size dst) <= n_rows = the rows of every src_j; an index outside [0, n_rows) is not followed and its
 *   destination row is not written.  n_keep = 0 is a no-op.
 * The host checks name the bad argument (mtgs_rast_last_error). */
int mtgs_crop_workspace_bytes(int64_t N, size_t *bytes);
int mtgs_crop_select(int64_t N, const float *means, int64_t row_stride, const float *box, int32_t *keep_ids, int64_t *count,
                     uint8_t *mask, void *ws, size_t ws_bytes, void *stream);
int mtgs_crop_gather(int64_t n_keep, int64_t n_rows, const int32_t *keep_ids, int n_tensors, const uint64_t *src,
                     const uint64_t *dst, const int64_t *row_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MTGS_CROP_H */
