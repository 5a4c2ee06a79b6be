#ifndef MTGS_JPEG_H
#define MTGS_JPEG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- encoding presented frames as baseline JPEG on the device (mtgs_amd/csrc/jpeg.hip; mtgs_amd.jpeg): the step after
 * mtgs_present_compose in the viewer thread (custom_viewer/render_state_machine.py:276-310, set_background_image(format="jpeg")),
 * in the evaluation image dump (scene_model/custom_pipeline.py:98-143, Pillow's save at its defaults: quality 75, 4:2:0) and in
 * the render tool (tools/render.py:729-734).  A header of its own, included by mtgs_rast.h; its reviewed record is
 * tests/golden/abi_signatures_jpeg.txt.  Additive: it changed neither MTGS_RAST_ABI_VERSION nor MTGS_RAST_HOT_ABI_VERSION.
 * Conventions (device pointers unless marked HOST, `stream`, return codes, mtgs_rast_last_error) are mtgs_rast.h's.
 *
 * The stream: baseline sequential DCT, 8 bits, YCbCr, ONE interleaved scan, the Annex K Huffman tables, no restart markers;
 * byte for byte what libjpeg's integer path (Pillow 12.2.0 with libjpeg-turbo) writes for the same pixels, quality and
 * subsampling.  Integer arithmetic throughout, 32 bits:
 *   header   SOI | APP0 JFIF 1.01, no units, density 1:1, no thumbnail | DQT 0 | DQT 1 | SOF0 (Y 2x2 or 1x1 on table 0, Cb and
 *            Cr 1x1 on table 1) | DHT DC 0, AC 0, DC 1, AC 1 | SOS: always MTGS_JPEG_HEADER_BYTES bytes
 *   tables   scale = 5000 / q for q < 50, otherwise 200 - 2 q; entry = clamp((base * scale + 50) / 100, 1, 255) of the Annex K
 *            luminance (table 0, Y) and chrominance (table 1, Cb and Cr) base tables; written in zigzag order
 *   input    uint8, or float32 x -> x' = x clamped to [0, 1] with NaN -> 0, TRUNCATE (uint8)(x' * 255) | ROUND
 *            (uint8)(x' * 255 + 0.5f): MTGS_PRESENT_U8_TRUNCATE / _ROUND of mtgs_present.h, each operation rounded once
 *   colour   F(x) = (int)(x * 65536 + 0.5):  Y  = (F(.299) R + F(.587) G + F(.114) B + 32768) >> 16
 *            Cb = (-F(.16874) R - F(.33126) G + F(.5) B + (128 << 16) + 32767) >> 16
 *            Cr = (F(.5) R - F(.41869) G - F(.08131) B + (128 << 16) + 32767) >> 16
 *   geometry 4:2:0: chroma is ceil(W/2) x ceil(H/2), MCUs of 16 x 16 pixels = Y00 Y01 Y10 Y11 Cb Cr; 4:4:4: MCUs of 8 x 8 = Y Cb
 *            Cr; a component has ceil(w_c / 8) x ceil(h_c / 8) REAL blocks; the MCU grid is ceil(W / side) x ceil(H / side)
 *   edges    inside real blocks the last column and, for Y, the last row are repeated.  Chroma at 4:2:0: rows are repeated at
 *            full resolution only up to an even height; below that the last DOWNSAMPLED row is repeated
 *   h2v2     (a + b + c + d + bias) >> 2, bias 1 in even output columns, 2 in odd ones
 *   dummy    a block of an MCU beyond its component's real blocks (Y at 4:2:0 only): every AC 0, DC the quantised DC of the
 *            block before it in the same MCU -- not the transform of repeated pixels; it predicts like any other block
 *   DCT      sample - 128; jfdctint's "islow" butterfly, CONST_BITS 13, PASS1_BITS 2, rows then columns, every descale
 *            (x + (1 << (n - 1))) >> n; constants 2446 3196 4433 6270 7373 9633 12299 15137 16069 16819 20995 25172; results
 *            are 8 times the DCT
 *   quantise sign(c) * ((|c| + (d >> 1)) / d), d = 8 * entry: an integer division, no reciprocal
 *   entropy  DC difference to the previous block of the component in scan order (0 for the first); category = bit length of
 *            |v|, then the low `category` bits of v, or of v - 1 for v < 0; AC as (run << 4 | category) with ZRL (0xF0) per 16
 *            zeros before a non-zero coefficient and EOB (0x00) if zeros remain at the end
 *   bytes    bits MSB first; the last partial byte padded with 1-bits; 0x00 after every 0xFF, the padded byte included; EOI
 *
 * Launches (all on `stream`, no host read, no atomics on floating point, bitwise reproducible; capturable in a HIP graph):
 *   blocks   one workgroup per MCU: pixels -> int16 coefficients in zigzag order, in scan order, dummy blocks included, and the
 *            bits of each block's AC codes
 *   offsets  a prefix sum over the blocks' code lengths (the DC difference is taken inside it): each block's bit offset, the total
 *   clear    zeroes the packed words the total covers and copies the header to data
 *   pack     one wave per block assembles its codes in LDS at its bit offset; whole words are stored, the first and the last
 *            word of a block are merged into the zeroed buffer by a vector atomic OR (order-independent)
 *   stuff    a prefix sum over the 0xFF counts of MTGS_JPEG_CHUNK_BYTES-byte chunks; each chunk is written behind the header at
 *            its offset; the last one writes EOI and meta
 * meta[0] = the bytes of the whole file, whether they fit or not; meta[1] = 1 if they did not fit in `capacity` (overflow), else
 * 0.  No byte at or beyond data + capacity is ever written.
 *
 * mtgs_jpeg_sizes: *ws_bytes of workspace (16-byte aligned) and the *capacity that cannot overflow: the header, every block at
 *   MTGS_JPEG_BLOCK_BITS (the longest DC code, 11 bits, and 11 more; 63 AC coefficients each with the longest code, 16 bits, and
 *   10 more: no EOB then, and a ZRL only replaces coefficients that cost more), every byte of that followed by a stuffed 0x00,
 *   and EOI: MTGS_JPEG_HEADER_BYTES + 2 * ceil(blocks * MTGS_JPEG_BLOCK_BITS / 8) + 2.
 * mtgs_jpeg_header: the header for (h, w, quality, subsampling) into HOST header[MTGS_JPEG_HEADER_BYTES]; upload it once.
 * mtgs_jpeg_encode: image[h, w, 3] with strides in ELEMENTS (uint8 for is_float = 0, float32 otherwise), `conversion` one of
 *   MTGS_PRESENT_U8_TRUNCATE / _ROUND (float32 only); `header` the DEVICE copy of mtgs_jpeg_header's bytes for the same h, w and subsampling: the
 *   quantisation tables are read from its two DQT segments, so the quality is the header's.
 * Limits: 1 <= h, w <= 65535 (SOF0's fields); quality in [1, 100]; blocks * MTGS_JPEG_BLOCK_BITS < 2^31.  The host checks name
 * the bad argument. */
#define MTGS_JPEG_HEADER_BYTES 623
#define MTGS_JPEG_BLOCK_BITS 1660
#define MTGS_JPEG_CHUNK_BYTES 16
enum { MTGS_JPEG_420 = 0, MTGS_JPEG_444 = 1 };

int mtgs_jpeg_sizes(int h, int w, int subsampling, size_t *ws_bytes, size_t *capacity);
int mtgs_jpeg_header(int h, int w, int quality, int subsampling, uint8_t *header, size_t header_capacity);
int mtgs_jpeg_encode(const void *image, int is_float, int conversion, int h, int w, int64_t stride_y, int64_t stride_x,
                     int64_t stride_c, int subsampling, const uint8_t *header, uint8_t *data, size_t capacity,
                     int64_t *meta, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MTGS_JPEG_H */
