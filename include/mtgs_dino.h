#ifndef MTGS_DINO_H
#define MTGS_DINO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the DINOv2 similarity metric on the device (mtgs_amd/csrc/dino.hip; mtgs_amd.dino): what mtgs/utils/dinov2.py's
 * DINOv2Similarity.similarity computes in get_metrics_dict and get_image_metrics_and_images under the key dinov2_sim
 * (mtgs_scene_graph.py:747-804, 1010-1092).  A header of its own, included by mtgs_rast.h; its reviewed record is
 * tests/golden/abi_signatures_dino.txt.  Additive: it changed neither MTGS_RAST_ABI_VERSION nor MTGS_RAST_HOT_ABI_VERSION.
 * Conventions (device pointers unless marked HOST, `stream`, return codes, mtgs_rast_last_error) are mtgs_rast.h's.  Forward only,
 * no atomics, no host read, no allocation, one stream: bitwise reproducible and graph-capturable.
 *
 * [RECALL] Three things are recalled, not checked -- neither torchvision nor the DINOv2 hub code was available to run:
 * torchvision's to_pil_image / Resize / CenterCrop / ToTensor / Normalize, the hub model's forward_features, and the hub
 * state-dict key names (mtgs_amd/dino.py).  Pillow's resampling is NOT recalled: it is restated and compared with Pillow bit for bit
 * (tests/dino_refs.py, tests/golden/dino_preprocess.npz).
 *
 * The definition (tests/dino_refs.py restates it), on two [H, W, 3] float32 images in [0, 1] and a nullable [H, W] byte mask
 * (non-zero = visible; NULL = all visible), for a network of width dim, dim / heads = 64, `depth` blocks, patch = 14, image = S =
 * G * patch, mlp_ratio = 4, layer-norm eps ln_eps (the hub's dinov2_vitb14: 768 / 12 / 12 / 14 / 518 / 1e-6; G = 37, T = 1 + G^2 =
 * 1370 tokens):
 * 1. byte = trunc(clamp(x, 0, 1) * 255) (pic.mul(255).byte(); THE CLAMP IS OURS: a value outside [0, 1] wraps in the reference and
 *    saturates here).  Resize the short side to S with Pillow's BILINEAR: output size (S, int(S * long / short)), unchanged when the
 *    short side is S.  Centre crop to S x S at offsets int(round((size - S) / 2.0)) with Python's round (half to even).  Then
 *    x / 255 and (x - 0.5) / 0.5 in fp32.
 *    Pillow's BILINEAR on 8-bit RGB is a two-pass resample.  Per axis: scale = in / out, fs = max(scale, 1), support = fs; for output
 *    xx: center = (xx + 0.5) * scale, xmin = max(int(center - support + 0.5), 0), xmax = min(int(center + support + 0.5), in); tap
 *    weights max(0, 1 - |(x + xmin - center + 0.5) * (1 / fs)|), normalised in double, each quantised as int(w * 2^22 + 0.5); a sum
 *    starts at 2^21, is shifted right by 22 and clipped to [0, 255]; the horizontal pass goes first and is rounded to 8 bits before
 *    the vertical one.  The caller builds the tables on the HOST in double and hands them over as ONE device int32 array
 *    `tables`, restricted to the cropped window, hk / vk = the largest tap count of the horizontal / vertical axis:
 *        hb [S][2]  (first source column, tap count) of window column x      hc [S][hk]  its quantised weights (0 beyond the count)
 *        vb [S][2], vc [S][vk]  the same for window row y
 *        mx [S], my [S]  source column / row of the mask's NEAREST resize (below)
 *    in this order: S * (6 + hk + vk) ints.  The kernels do integer arithmetic only and clamp every source index into the image.
 * 2. Mask: a byte image, 255 where the mask is non-zero; Pillow's NEAREST resize to the same output size: the source index per axis is
 *    int(xo), xo starting at 0.5 * in / out and advanced by REPEATED ADDITION of in / out in double; the same crop.  The weight of
 *    patch (py, px) is the count of non-zero pixels of its 14 x 14 block / 196.  weights [G^2 + 1]: the patch weights, then their sum,
 *    which is (total count) / 196 in ONE rounding.
 * 3. forward_features(...)["x_norm_patchtokens"]: patch embedding = a 14 x 14 stride-14 convolution 3 -> dim with bias; the class
 *    token is prepended and pos_embed [T][dim] added WITHOUT interpolation; `depth` blocks x += ls1 * proj(attention(norm1(x))),
 *    x += ls2 * fc2(gelu(fc1(norm2(x)))): qkv with bias, q scaled by 64^-0.5 before q k^T, softmax over the keys, GELU in the
 *    exact (erf) form; a final layer norm; rows 1 .. G^2 are kept.
 * 4. Per patch cos = sum_c (a_c / max(|a|, 1e-8)) (b_c / max(|b|, 1e-8)) (torch.nn.functional.cosine_similarity of torch 2.x);
 *    result = sum(cos * weight) / sum(weight), exactly 0.0 when sum(weight) <= 1e-6, decided on the device; one float32 at out[0].
 *
 * mtgs_dino_preprocess writes the normalised values as the patch matrix [2 * G^2, 3 * 14 * 14] in the convolution's (c, ky, kx)
 * order (row = image * G^2 + py * G + px), so the patch embedding is a plain GEMM with K = 588; `bytes` (nullable) receives the
 * resized and cropped bytes [2, S, S, 3].
 * mtgs_dino_linear: out [M, N] = epilogue(a [M, K] row-major x w [K][N] packed), on v_mfma_f32_32x32x2_f32.  K is never split over
 * lanes, waves or workgroups: each output is computed by one lane as k-ordered fp32 fma chains of 128 k's, whose sums are added in k
 * order (K <= 128: ONE chain); a single chain over K = 3072 lost a factor of three against the fp32 CPU restatement on 768-wide
 * features.  M arbitrary, N a multiple of 64, K a multiple of 4; w and out 16-byte aligned.
 *    MTGS_DINO_EPI_BIAS            acc + bias[n]
 *    MTGS_DINO_EPI_BIAS_GELU       gelu(acc + bias[n])
 *    MTGS_DINO_EPI_SCALE_RESIDUAL  out[m][n] += gamma[n] * (acc + bias[n])            (in place: out holds the residual)
 *    MTGS_DINO_EPI_PATCH_EMBED     M = 2 * G^2 rows -> out [2 * tokens, N]: row image * tokens + 1 + p = acc + bias[n] + pos[1 + p][n];
 *                                  the two class rows image * tokens = cls[n] + pos[0][n] are written by the same launch
 *    gamma / pos / cls are read by the epilogue that names them only (NULL otherwise); tokens = T = 1 + G^2.
 * mtgs_dino_layernorm: one wave per row of [M, D], two passes (the mean, then the variance about the mean) in a fixed order; D a
 * multiple of 64, at most 1024.
 * mtgs_dino_attention: qkv [n, T, 3 * heads * 64] (per row q | k | v, each heads x 64) -> out [n, T, heads * 64]; one workgroup per
 * (image, head, 128 query rows), K and V streamed through LDS in blocks of 32 keys, q k^T and p v on the MFMA unit, online softmax
 * with the running maximum, keys beyond T masked in the last block; nothing of size [T, T] is written.  qkv 16-byte aligned.
 * mtgs_dino_tail: step 4 on feature rows a, b [G^2, D] and weights [G^2 + 1]; scratch [G^2] floats.
 * mtgs_dino_features: steps 1 and 3 -> features [2, G^2, dim].  mtgs_dino_similarity: the whole metric.
 *
 * `weights` of the network is ONE float array, 16-byte aligned (mtgs_dino_weight_floats = its length), linear layers packed
 * [K][N] (torch's [out, in] transposed):
 *    patch_embed [588][dim] (K in the order (c, ky, kx)), its bias [dim], cls_token [dim], pos_embed [T][dim];
 *    per block: norm1 weight, bias [dim]; qkv [dim][3 dim], bias [3 dim]; proj [dim][dim], bias [dim]; ls1 gamma [dim];
 *               norm2 weight, bias [dim]; fc1 [dim][4 dim], bias [4 dim]; fc2 [4 dim][dim], bias [dim]; ls2 gamma [dim];
 *    norm weight, bias [dim].
 * ws: mtgs_dino_workspace_bytes(cfg), 16-byte aligned: the patch matrix, the token stream, one layer-norm / attention output, one
 * buffer for qkv and the MLP's hidden layer, the patch weights and the per-patch terms (about 57 MB at ViT-B / 518). */
typedef struct mtgs_dino_config {
    int dim, heads, depth, patch, image, mlp_ratio;
    float ln_eps;
} mtgs_dino_config;

enum { MTGS_DINO_EPI_BIAS = 0, MTGS_DINO_EPI_BIAS_GELU = 1, MTGS_DINO_EPI_SCALE_RESIDUAL = 2, MTGS_DINO_EPI_PATCH_EMBED = 3 };
#define MTGS_DINO_PATCH 14
#define MTGS_DINO_HEAD_DIM 64
#define MTGS_DINO_MAX_DIM 1024

int mtgs_dino_weight_floats(const mtgs_dino_config *cfg, size_t *floats);
int mtgs_dino_workspace_bytes(const mtgs_dino_config *cfg, size_t *bytes);
int mtgs_dino_preprocess(int H, int W, int S, const float *pred, const float *gt, const int32_t *tables, int hk, int vk, uint8_t *bytes,
                         float *patches, void *stream);
int mtgs_dino_patch_weights(int H, int W, int S, const uint8_t *mask, const int32_t *tables, int hk, int vk, float *weights, void *stream);
int mtgs_dino_linear(int M, int K, int N, const float *a, const float *w, const float *bias, int epilogue, const float *gamma,
                     const float *pos, const float *cls, int tokens, float *out, void *stream);
int mtgs_dino_layernorm(int M, int D, float eps, const float *in, const float *w, const float *b, float *out, void *stream);
int mtgs_dino_attention(int n, int T, int heads, const float *qkv, float *out, void *stream);
int mtgs_dino_tail(int G2, int D, const float *a, const float *b, const float *weights, float *scratch, float *out, void *stream);
int mtgs_dino_features(const mtgs_dino_config *cfg, int H, int W, const float *pred, const float *gt, const int32_t *tables, int hk, int vk,
                       const float *weights, float *features, void *ws, size_t ws_bytes, void *stream);
int mtgs_dino_similarity(const mtgs_dino_config *cfg, int H, int W, const float *pred, const float *gt, const uint8_t *mask,
                         const int32_t *tables, int hk, int vk, const float *weights, float *out, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MTGS_DINO_H */
