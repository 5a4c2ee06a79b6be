#ifndef MTGS_PNG_H
#define MTGS_PNG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- lossless depth and label planes on the device: an indexed PNG codec (mtgs_amd/csrc/png.hip; mtgs_amd.png).  Three planes of a
 * training frame arrive as PNG (the pseudo depth, mtgs/dataset/custom_dataset.py:162-173; the panoptic / semantic map, :203-243; the
 * ego mask, :154-160) and two preprocessing stages leave the device only to write such files (nuplan_scripts/generate_dense_depth.py:
 * 236-247 and the semantic-mask stage).  A header of its own, included by mtgs_rast.h; its reviewed record is
 * tests/golden/abi_signatures_png.txt.  Additive: it changed neither MTGS_RAST_ABI_VERSION nor MTGS_RAST_HOT_ABI_VERSION.
 * Conventions (device pointers unless marked HOST, `stream`, return codes, mtgs_rast_last_error) are mtgs_rast.h's.
 *
 * A pair: a WRITER whose files every PNG reader accepts, and a READER that decodes the writer's files in parallel, guided by a
 * private index chunk.  A PNG without that chunk is refused by name (mtgs_amd.png.parse_png): decode it on the host, encode it here.
 *
 * The file:
 *   chunks    the PNG signature | IHDR | mtIX | ONE IDAT | IEND
 *   IHDR      width, height, 8 bits, colour type 0 (gray, 1 channel) or 2 (RGB, 3 channels), compression 0, filter method 0, no interlace
 *   rows      the row stream is h rows of L = 1 + w * channels bytes: the filter byte, then the filtered bytes.  ONE filter per
 *             image: 0 None x; 1 Sub x - (the same channel of the pixel to the left, 0 for the first pixel); 2 Up x - (the byte above,
 *             0 in the first row); all mod 256.  Average and Paeth serialise a row: never written, refused on read
 *   segments  every row's L bytes are cut into ceil(L / segment_bytes) segments of segment_bytes bytes, the last one of a row
 *             shorter; segment s = row * ceil(L / segment_bytes) + k.  The unit of parallel decoding: no run crosses a segment start
 *   tokens    of a segment, left to right: the byte that starts a maximal run of 1 + r equal bytes INSIDE the segment is a literal;
 *             while r >= 3 a match of length min(r, 258) at distance 1 follows and r drops by that length; the remaining 0..2 bytes
 *             are literals.  Per position p of its run: p = 0 is a literal; otherwise q = (p - 1) / 258, rem = r - 258 q; if
 *             rem >= 3 a match of min(rem, 258) stands at the positions with (p - 1) % 258 = 0 and covers the others, otherwise the
 *             position is a literal.  Every position decides alone
 *   IDAT      78 01 | ONE deflate block, BFINAL = 1, BTYPE = 10 (dynamic Huffman) | padding to a byte | the big-endian Adler-32 of the
 *             row stream.  RFC 1951: bits LSB first, Huffman codes from their most significant bit; lengths 3..258 are symbols
 *             257..285 with 0..5 extra bits (258 is symbol 285); distance 1 is distance symbol 0, no extra bits
 *   lit/len   counts over the whole image plus one end-of-block (256).  Lengths by a two-queue Huffman over the used symbols sorted
 *             by (count, symbol) ascending: the two smallest heads are joined, the leaf queue first on ties.  bits[l] = the leaves at
 *             depth l, limited to 15 by JPEG Annex K.2's adjustment: from the longest length i down to 16, while bits[i] > 0: j = the
 *             nearest l <= i - 2 with bits[l] > 0; bits[i] -= 2, bits[i - 1] += 1, bits[j + 1] += 2, bits[j] -= 1.  Lengths go to
 *             the symbols in order of (count descending, symbol ascending), shortest first; then RFC 1951's canonical codes
 *   distance  HDIST = 1: one code of ONE bit (the bit 0) for distance 1 if the image has a match, otherwise a single length 0
 *   lengths   the sequence is the HLIT lit/len lengths (HLIT = max(257, the last used symbol + 1)) followed by the distance length.
 *             A non-zero length is its own symbol.  A run of z zeros: while z >= 11, symbol 18 with min(z, 138); then symbol 17
 *             if z >= 3; otherwise z plain zeros.  Symbol 16 is never used.  The 19 symbols get their code from the same builder,
 *             limited to 7 bits; HCLEN counts them in RFC 1951's order with the trailing zeros dropped, at least 4
 *   mtIX      ancillary, private, not safe to copy.  Little-endian uint32: MTGS_PNG_INDEX_VERSION | filter | segment_bytes | the
 *             segment count n | n bit offsets, each of a segment's first token from the first byte of the IDAT payload (the 78) |
 *             the bit offset of the end-of-block code
 *   CRC-32    IHDR's and IEND's are written; the fields of mtIX and IDAT are written as ZERO: they depend on the bytes, and the host
 *             fills them when the file leaves the device (mtgs_amd.png.PngStream.tobytes).  The device reader never consults them
 *
 * The encoder's launches (all on `stream`, no host read, capturable in a HIP graph, bitwise reproducible; the only atomics are
 * integer adds into the symbol histogram and the order-independent OR that merges shared words):
 *   tokens    one workgroup per segment: the filtered bytes into LDS, run starts and ends by a max / min scan, each position's token
 *             (uint16: a literal, 256 + a match length, or covered), the histogram in LDS and one add per used symbol per
 *             workgroup, the segment's two Adler-32 sums
 *   codes     ONE workgroup: both codes, the canonical table (bit-reversed) and the bits of the block header
 *   offsets   a prefix sum (scan.hpp) over the tokens' bit lengths: each position's bit offset, the segment table, the total
 *   clear     zeroes the words the total covers
 *   pack      2048 positions per workgroup, assembled in LDS; whole words are stored, the first and last word of a workgroup are
 *             merged by a vector atomic OR
 *   finish    ONE workgroup: 78 01 and the block header, the end-of-block code, a = 1 + sum s_i, b = n + sum (n - i) s_i (mod
 *             65521, 64-bit integers) behind the last bits
 *   emit      the only launch that writes `data`: the chunks, every store checked against `capacity`; meta
 * meta[0] = the bytes of the whole file, whether they fit or not; meta[1] = 1 if they did not (overflow), else 0.  No byte at or
 * beyond data + capacity is ever written.
 *
 * The decoder's launches (no host read, no allocation, capturable):
 *   inflate   ONE LANE per segment decodes from its bit offset until its byte count is produced, tables in LDS, into the row stream
 *             in the workspace; it keeps the segment's Adler-32 sums.  Whatever the bytes are: every token produces at least one
 *             byte or ends the segment, a segment writes only its own bytes, reads beyond the payload give zeros, table indices are
 *             masked.  A segment counts as decoded if it ended without an error exactly at the next segment's bit offset
 *   unfilter  Sub: a per-row, per-channel prefix sum mod 256; Up: a per-column prefix sum; then the store: uint8 at strides in
 *             ELEMENTS in file order or reversed (bgr), or as_depth: float32 (float(b0) + float(b1) * 256.0f) * 0.01f with b0 / b1
 *             the file's blue / green (OpenCV's channels 0 / 1): custom_dataset.py:166-168, no byte image is stored
 *   status    ONE workgroup sums the segments' Adler-32 sums and compares with the stored value
 * status, int32[MTGS_PNG_STATUS_WORDS]: [0] an error word (MTGS_PNG_ERR_SEGMENT: a segment did not decode; MTGS_PNG_ERR_ADLER: the
 * recomputed Adler-32 differs), [1] segments decoded, [2] segments expected, [3] 1 if the Adler-32 is the stored one.
 *
 * `tables`, MTGS_PNG_TABLE_WORDS int32 words, built by the host from the block header: FAST_AT [1 << MTGS_PNG_FAST_BITS] by the
 * next bits of the stream (LSB first): (code length << 9) | symbol, 0 if no code that short; COUNT_AT [16] the codes of each length;
 * SYMS_AT [288] the symbols by (length, symbol); DIST_AT [1] 1 if the distance code exists.
 * `segment_bits`: uint32 [segments + 1], mtIX's offsets and the end-of-block offset behind them.
 *
 * The depth rule of the writer (is_depth: `image` is float32 depth[roi_h, roi_w], the file is [h, w, 3]), generate_dense_depth.py:
 * 236-247 in float32, every operation rounded once: d outside [min_depth, max_range] or NaN -> 0; t = d * 100; file blue =
 * (uint8) fmod(t, 256), file green = (uint8) floor(t / 256), red 0, inside the window (roi_x, roi_y, roi_w, roi_h); zero elsewhere.
 *
 * mtgs_png_sizes: *ws_bytes of workspace (16-byte aligned) and the *capacity that cannot overflow: the chunks around the payload,
 *   and a payload of 2 + ceil((MTGS_PNG_HEADER_BITS + 15 * (h * L + 1)) / 8) + 4 bytes: no position costs more than 15 bits (a
 *   match of at most 21 covers at least 3).
 * MTGS_PNG_SEGMENT_BYTES is the measured default (profiles/png.txt): the inflate launch is one serial bit chain per lane, so its time
 *   falls with the segment's length; below 256 bytes the ratio of a label plane and the encoder's time give more than that returns.
 * Limits: 1 <= h, w <= 65535; channels 1 or 3; segment_bytes in [MTGS_PNG_MIN_SEGMENT_BYTES, MTGS_PNG_MAX_SEGMENT_BYTES]; the worst
 * case of the stream below 2^32 bits.  The host checks name the bad argument. */
#define MTGS_PNG_INDEX_VERSION 1
#define MTGS_PNG_MIN_SEGMENT_BYTES 16
#define MTGS_PNG_MAX_SEGMENT_BYTES 8192
#define MTGS_PNG_SEGMENT_BYTES 256
#define MTGS_PNG_HEADER_BITS 4096
#define MTGS_PNG_FAST_BITS 10
#define MTGS_PNG_FAST_AT 0
#define MTGS_PNG_COUNT_AT 1024
#define MTGS_PNG_SYMS_AT 1040
#define MTGS_PNG_DIST_AT 1328
#define MTGS_PNG_TABLE_WORDS 1332
#define MTGS_PNG_STATUS_WORDS 4
enum { MTGS_PNG_FILTER_NONE = 0, MTGS_PNG_FILTER_SUB = 1, MTGS_PNG_FILTER_UP = 2 };
enum { MTGS_PNG_ORDER_RGB = 0, MTGS_PNG_ORDER_BGR = 1 };
enum { MTGS_PNG_ERR_SEGMENT = 1, MTGS_PNG_ERR_ADLER = 2 };

int mtgs_png_sizes(int h, int w, int channels, int segment_bytes, size_t *ws_bytes, size_t *capacity);
int mtgs_png_encode(const void *image, int is_depth, int h, int w, int channels, int64_t stride_y, int64_t stride_x,
                    int64_t stride_c, int order, int filter, int segment_bytes, int roi_x, int roi_y, int roi_w, int roi_h,
                    float max_range, float min_depth, uint8_t *data, size_t capacity, int64_t *meta, void *ws, size_t ws_bytes,
                    void *stream);
int mtgs_png_decode_sizes(int h, int w, int channels, int segment_bytes, size_t *ws_bytes);
int mtgs_png_decode(const uint8_t *payload, int64_t payload_bytes, const uint32_t *segment_bits, const int32_t *tables, int h,
                    int w, int channels, int filter, int segment_bytes, void *out, int as_depth, int64_t stride_y,
                    int64_t stride_x, int64_t stride_c, int order, int32_t *status, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MTGS_PNG_H */
