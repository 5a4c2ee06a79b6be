#ifndef MTGS_PRESENT_H
#define MTGS_PRESENT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- presenting rendered frames on the device (mtgs_amd/csrc/present.hip; mtgs_amd.present): what the viewer thread and the
 * offline render tool do to the outputs of get_outputs_for_camera before a frame leaves the device -- nerfstudio's apply_colormap /
 * apply_depth_colormap, the split view, the concatenation of several outputs, the uint8 conversion, the padding to the client's
 * aspect, and the resized depth for the viewer's compositing (custom_viewer/render_state_machine.py:174-190, 240-310,
 * tools/render.py:131-165).  A header of its own, included by mtgs_rast.h; its reviewed record is
 * tests/golden/abi_signatures_present.txt.  Additive: it changed neither MTGS_RAST_ABI_VERSION nor MTGS_RAST_HOT_ABI_VERSION.
 * Conventions (device pointers unless marked HOST, `stream`, return codes, mtgs_rast_last_error) are mtgs_rast.h's.
 *
 * A frame is out[out_h, out_w, 3], uint8 or float32, written whole by ONE launch of mtgs_present_compose.  Up to
 * MTGS_PRESENT_MAX_PANELS panels (a HOST table, passed on as a kernel argument) fill rectangles of it: panel j covers output rows
 * [y0, y0 + h) and columns [x0, x0 + w); output pixel (y, x) of it shows source pixel (y - y0, src_x0 + x - x0).  Pixels no panel
 * covers are 0 (the padding); column split_column (-1: none) is split_color[3] (HOST) in every row a panel covers.  The first panel
 * of the table that covers a pixel shows there.
 * A panel's source is src[src_h, src_w, C], contiguous: kind RGB C = 3 float32, shown unchanged | FLOAT C = 1 float32, the
 * float colormap | DEPTH C = 1 float32, the depth colormap, `accumulation` [src_h, src_w] float32 nullable | BOOL C = 1 byte,
 * white where non-zero, black elsewhere.
 * Arithmetic, every operation fp32 and rounded once, in this order:
 *   DEPTH  near, far = near_plane, far_plane, or where that is NaN the source's min, max (mtgs_present_stats);
 *          inv = 1.0f / (float)((far - near) + 1e-10 in double); v = clip((d - (float)near) * inv, 0, 1), NaN kept; then as FLOAT;
 *          then with an accumulation a, per channel c = c * a + (1 - a) (three roundings)
 *   FLOAT  if normalize: v = v - lo, v = v / ((hi - lo) + 1e-9f) with lo, hi the min and max over the whole source of v as it
 *          enters this step (for DEPTH: the clipped values of the source's extrema, since every step before is monotone);
 *          v = v * (float)(colormap_max - colormap_min in double) + (float)colormap_min (two roundings); v = clip(v, 0, 1);
 *          if invert: v = 1 - v; NaN -> 0; lut == NULL ("gray"): (v, v, v), otherwise lut[(int)(v * 255)] of lut[256, 3] float32
 *   A NaN anywhere in a source whose min / max is taken makes both NaN (torch.min / torch.max), hence every pixel of the panel.
 * Output: float32 as computed, or uint8 of x' = x clamped to [0, 1] with NaN -> 0: TRUNCATE (uint8)(x' * 255), the viewer's
 * `(x * 255).type(torch.uint8)` | ROUND (uint8)(x' * 255 + 0.5f), a video writer's conversion.
 *
 * mtgs_present_stats: ONE launch for the table: per-workgroup (min, max) partials of every source whose extrema compose needs
 *   (DEPTH with near_plane or far_plane NaN, FLOAT or DEPTH with normalize) into ws (mtgs_present_workspace_bytes, 8-byte
 *   aligned).  Compose re-reduces them in a fixed order: no atomics, no host read, bitwise reproducible.  A table that needs
 *   none launches nothing, and compose then does not read ws (it may be NULL).
 * mtgs_present_depth_resize: dst[out_h, out_w] = scale * bilinear(src[in_h, in_w]) as torch's upsample_bilinear2d with
 *   align_corners = False: r = (float)in / (float)out, s = max(r * (i + 0.5f) - 0.5f, 0), i0 = (int)s, i1 = i0 + (i0 < in - 1),
 *   l1 = s - i0, l0 = 1 - l1 per axis; value = h0 * (w0 * a + w1 * b) + h1 * (w0 * c + w1 * d).
 * Limits: out_h * out_w and every src_h * src_w < 2^31.  Empty frames are no-ops.  The host checks name the bad argument. */
#define MTGS_PRESENT_MAX_PANELS 8
#define MTGS_PRESENT_STAT_BLOCKS 256
enum { MTGS_PRESENT_RGB = 0, MTGS_PRESENT_FLOAT = 1, MTGS_PRESENT_DEPTH = 2, MTGS_PRESENT_BOOL = 3 };
enum { MTGS_PRESENT_U8_TRUNCATE = 0, MTGS_PRESENT_U8_ROUND = 1, MTGS_PRESENT_F32 = 2 };

typedef struct mtgs_present_panel {
    const void *src;
    const float *accumulation;      /* DEPTH only, nullable */
    const float *lut;               /* FLOAT and DEPTH: [256, 3], or NULL for gray */
    double near_plane, far_plane;   /* DEPTH: NaN = the source's min / max */
    double colormap_min, colormap_max;
    int32_t kind, normalize, invert;
    int32_t src_h, src_w, src_x0;
    int32_t y0, x0, h, w;
} mtgs_present_panel;

int mtgs_present_workspace_bytes(size_t *bytes, size_t *panel_bytes);
int mtgs_present_stats(int n_panels, const mtgs_present_panel *panels, void *ws, size_t ws_bytes, void *stream);
int mtgs_present_compose(int n_panels, const mtgs_present_panel *panels, int out_h, int out_w, int split_column,
                         const float *split_color, int format, void *out, const void *ws, size_t ws_bytes, void *stream);
int mtgs_present_depth_resize(int in_h, int in_w, const float *src, int out_h, int out_w, float scale, float *dst, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MTGS_PRESENT_H */
