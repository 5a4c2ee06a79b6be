#ifndef MTGS_LPIPS_H
#define MTGS_LPIPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the LPIPS metric (AlexNet backbone) on the device (mtgs_amd/csrc/lpips.hip; mtgs_amd.lpips): what
 * LearnedPerceptualImagePatchSimilarity(normalize=True) computes in get_metrics_dict on every training step and for every
 * evaluation image (mtgs_scene_graph.py:323-325, 779-782, 1066-1069).  A header of its own, included by mtgs_rast.h; its reviewed
 * record is tests/golden/abi_signatures_lpips.txt.  Additive: it changed neither MTGS_RAST_ABI_VERSION nor
 * MTGS_RAST_HOT_ABI_VERSION.  Conventions (device pointers unless marked HOST, `stream`, return codes, mtgs_rast_last_error) are
 * mtgs_rast.h's.  Forward only, no atomics, no host read: bitwise reproducible and graph-capturable.
 *
 * The definition (tests/lpips_refs.py restates it in fp64), on two [H, W, 3] float32 images and a nullable [H, W] byte mask:
 *   x = img where mask != 0, else 0;  if normalize: x = 2x - 1;  x = (x - shift[c]) / scale[c],
 *       shift = (-.030, -.088, -.188), scale = (.458, .449, .450)
 *   five taps, each after a ReLU; convolutions with bias and ZERO padding of the scaled tensor:
 *       conv 11x11 stride 4 pad 2, 3 -> 64 | maxpool 3x3 stride 2, conv 5x5 pad 2, 64 -> 192 | maxpool 3x3 stride 2, conv 3x3 pad 1,
 *       192 -> 384 | conv 3x3 pad 1, 384 -> 256 | conv 3x3 pad 1, 256 -> 256
 *   per tap and pixel: u = f / n over the channels with n = sqrt(sum f^2 + 1e-8) (MTGS_LPIPS_NORM_SQRT_EPS_INSIDE) or
 *       n = sqrt(sum f^2) + 1e-10 (MTGS_LPIPS_NORM_EPS_OUTSIDE); d = sum_c lin[c] (u0[c] - u1[c])^2; the tap's term is the mean of d
 *       over its pixels; the result is the sum of the five terms, one float32 at out[0].
 *
 * Activations are NHWC with both images in one array, [n, h, w, C] with n = 2 inside mtgs_lpips.  A convolution is an implicit GEMM
 * on v_mfma_f32_32x32x2_f32: M = n * oh * ow, N = cout, K = kh * kw * cin in the order (kh, kw, cin), each output element ONE
 * k-ordered fp32 fma chain (K is not split), then + bias and the ReLU.  Weights are packed [K][cout] (mtgs_lpips_repack, from
 * torch's [cout, cin, kh, kw]); cout must be a multiple of 32.
 * `weights` of mtgs_lpips is ONE array: for each of the five layers its packed weights [K][cout], its bias [cout] and its lin
 * vector [cout], in this order, 16-byte aligned (mtgs_lpips_weight_floats = its length).
 * mtgs_lpips_conv_first is the first layer's form: it reads pred, gt and the mask and applies the input transform on load.
 * mtgs_lpips_maxpool: 3x3, stride 2, no padding, [n, h, w, c] -> [n, (h - 3) / 2 + 1, (w - 3) / 2 + 1, c], c a multiple of 4.
 * Limits: H, W >= 31 for mtgs_lpips (smaller images leave no pixel after the second pool); every array < 2^31 elements.
 * ws: mtgs_lpips_workspace_bytes(H, W), 16-byte aligned. */
enum { MTGS_LPIPS_NORM_SQRT_EPS_INSIDE = 0, MTGS_LPIPS_NORM_EPS_OUTSIDE = 1 };
#define MTGS_LPIPS_MIN_SIDE 31

int mtgs_lpips_workspace_bytes(int H, int W, size_t *bytes);
int mtgs_lpips_weight_floats(size_t *floats);
int mtgs_lpips_repack(int cout, int cin, int kh, int kw, const float *w, float *packed, void *stream);
int mtgs_lpips_conv(int n, int h, int w, int cin, int cout, int kh, int kw, int stride, int pad, const float *in, const float *packed,
                    const float *bias, int relu, float *out, void *stream);
int mtgs_lpips_conv_first(int H, int W, const float *pred, const float *gt, const uint8_t *mask, int normalize, int cout, int kh,
                          int kw, int stride, int pad, const float *packed, const float *bias, int relu, float *out, void *stream);
int mtgs_lpips_maxpool(int n, int h, int w, int c, const float *in, float *out, void *stream);
int mtgs_lpips(int H, int W, const float *pred, const float *gt, const uint8_t *mask, const float *weights, int normalize, int norm,
               float *out, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MTGS_LPIPS_H */
