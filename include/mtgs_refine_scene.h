#ifndef MTGS_REFINE_SCENE_H
#define MTGS_REFINE_SCENE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- densification on the device: refinement_after for EVERY node of a scene graph in one pass (SURVEY.md section 8f, rank 2;
 * mtgs_amd/csrc/refine.hip; mtgs_amd.densify.refine_scene, and refine_gaussians for ONE node: the one-entry case of the table).
 * Restates refinement_after / split_gaussians / dup_gaussians / cull_gaussians + the optimizer surgery of
 * mtgs/scene_model/gaussian_model/vanilla_gaussian_splatting.py:392-446, 476-699 per node, with the node's own thresholds, seed,
 * phase and cull rule (skybox_gaussian_splatting.py:130-163: the sky node replaces the far rule's constants).
 * The only refinement entry points since MTGS_RAST_ABI_VERSION 29, which removed the single-node mtgs_refine_classify / _apply /
 * _rows; MTGS_RAST_HOT_ABI_VERSION stays 7.  A header of its own, included by mtgs_rast.h; its reviewed record is
 * tests/golden/abi_signatures_refine_scene.txt.  Conventions (device pointers unless marked HOST, `stream`, return codes,
 * mtgs_rast_last_error) are mtgs_rast.h's.
 *
 * The nodes that take part (densify or cull-only phase, n > 0) follow each other in a table in DEVICE memory (8-byte aligned);
 * node j owns elements [start, start + n) of the scene-wide arrays counts / flags / incl (start = running sum of n) and
 * workgroups [first_block, first_block + ceil(n / 256)) of the classify and index launches.  A workgroup finds its node by
 * binary search over first_block.  Columns (kinds) of a node with S = options[0] split samples: 0 old row kept | 1 + s child
 * of sample s kept | 1 + S duplicate kept; the scene has n_columns = 2 + max S of them, a node's unused ones are zero.
 * thresholds[6]: densify_grad_thresh, densify_size_thresh, split_screen_size, cull_alpha_thresh, cull_scale_thresh,
 *   cull_screen_size.  options[5]: n_split_samples (1..4), split by screen size (step < stop_screen_size_at), cull by world size
 *   (step > refine_every * reset_alpha_every), cull by screen size, clone_sample_means.  Cull rule: far = |mean| > far_radius,
 *   thresh = (far ? far_factor : 1) * cull_scale_thresh in fp32 (100 / 40: VanillaGaussianSplattingModel).
 * Flag byte of a Gaussian: bit 0 old row kept | bit 1 + s child of sample s kept | bit 1 + S duplicate kept | bit 7 split parent.
 * phase MTGS_REFINE_DENSIFY: split / duplicate / cull; samples: Philox4x32-10 keyed by (seed, step, NODE-LOCAL index, slot) --
 *   identical on every rank, and for a node alone or inside any scene.  Output order: old rows, then children sample-major, then
 *   duplicates (the reference's).
 * phase MTGS_REFINE_CULL_ONLY: only column 0 can be 1 (cull_gaussians() without a split mask); the statistics pointers are
 *   not followed unless options[3] (screen-size rule), which reads max_2dsize.
 * mtgs_refine_scene_classify: counts[(n_columns + 1), n_total] i32 -- the columns above, then the split-parent bit -- and
 *   flags[n_total] u8 (the byte above); parents (nullable, u8 [n_total]) = 1 where a child or the duplicate is
 *   kept.  The caller takes an INCLUSIVE prefix sum of every counts row over the whole concatenation (incl, int64) and reads
 *   its values at the nodes' last elements: the one host read.  From them it fills, per node: scan_base[k] = incl[k] just
 *   before the node (0 for the first), col_base[k] = node-local first output row of column k, n_out, out_start (running sum
 *   of n_out) and out_first_block (running sum of ceil(n_out / 256)).
 * mtgs_refine_scene_apply (table filled as above): src_index[n_out_total] i32 (NODE-LOCAL source row) and kind[n_out_total]
 *   u8 of every output row, and out_means / out_scales[n_out_total, 3]; node j's rows are [out_start, out_start + n_out).
 * mtgs_refine_scene_rows: every remaining tensor of every node in ONE launch.  One mtgs_refine_move per (node, tensor):
 *   dst[r, :] = op(src[src_index[out_start + r], :]) for r < n_rows, rows of `width` dwords (1 .. 32768), src / dst 4-byte
 *   aligned and contiguous.  op COPY | ZERO_NEW (0 where kind != 0: Adam moments of new Gaussians) | CLAMP_MAX (v > clamp_max
 *   ? clamp_max : v: the opacity reset) | ZERO_ALL (src is not read: opacity moments at a reset).  Workgroup b of the launch
 *   works on MTGS_REFINE_MOVE_DWORDS consecutive dwords of the move with first_block <= b; first_block = running sum of
 *   ceil((n_rows * width + 3) / MTGS_REFINE_MOVE_DWORDS) (the slack of 3 covers the shift that makes every 16-byte store aligned).
 * Limits: n_total and n_out_total < 2^31.  No atomics: bitwise reproducible.  n_nodes = 0 / n_moves = 0 / empty scenes are no-ops.
 * The host checks name the bad argument (mtgs_rast_last_error). */
#define MTGS_REFINE_MAX_COLUMNS 6
#define MTGS_REFINE_MOVE_DWORDS 8192
enum { MTGS_REFINE_DENSIFY = 1, MTGS_REFINE_CULL_ONLY = 2 };
enum { MTGS_REFINE_COPY = 0, MTGS_REFINE_ZERO_NEW = 1, MTGS_REFINE_CLAMP_MAX = 2, MTGS_REFINE_ZERO_ALL = 3 };

typedef struct mtgs_refine_node {
    int64_t n, first_block, start;
    int64_t n_out, out_first_block, out_start;      /* after the host read */
    int64_t scan_base[MTGS_REFINE_MAX_COLUMNS];     /* after the host read */
    int64_t col_base[MTGS_REFINE_MAX_COLUMNS];      /* after the host read */
    const float *means, *scales, *quats, *opacities;
    const float *xys_grad_norm, *vis_counts, *max_2dsize;
    uint64_t seed;
    float thresholds[6];
    float far_radius, far_factor;
    int32_t options[5];
    int32_t phase;
} mtgs_refine_node;

typedef struct mtgs_refine_move {
    int64_t n_rows, first_block, out_start;
    int64_t n_src;                                  /* rows of src: an index outside [0, n_src) gives a zero row */
    const void *src;
    void *dst;
    int32_t width, op;
    float clamp_max;
    int32_t reserved;
} mtgs_refine_move;

int mtgs_refine_scene_table_bytes(size_t *node_bytes, size_t *move_bytes);
int mtgs_refine_scene_classify(int n_nodes, const mtgs_refine_node *table, int64_t total_blocks, int64_t n_total, int n_columns,
                               int64_t step, int32_t *counts, uint8_t *flags, uint8_t *parents, void *stream);
int mtgs_refine_scene_apply(int n_nodes, const mtgs_refine_node *table, int64_t total_blocks, int64_t out_blocks, int64_t n_total,
                            int64_t n_out_total, int n_columns, int64_t step, const uint8_t *flags, const int64_t *incl,
                            int32_t *src_index, uint8_t *kind, float *out_means, float *out_scales, void *stream);
int mtgs_refine_scene_rows(int n_moves, const mtgs_refine_move *moves, int64_t total_blocks, const int32_t *src_index,
                           const uint8_t *kind, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MTGS_REFINE_SCENE_H */
