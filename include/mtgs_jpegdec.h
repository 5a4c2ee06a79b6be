#ifndef MTGS_JPEGDEC_H
#define MTGS_JPEGDEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- decoding baseline JPEG frames on the device (mtgs_amd/csrc/jpegdec.hip; mtgs_amd.jpegdec): the first thing the reference does
 * with a training frame, Image.open(...) followed by np.array(...) (mtgs/dataset/custom_dataset.py:78-97), and the read side of
 * mtgs_jpeg.h.  A header of its own, included by mtgs_rast.h; its reviewed record is tests/golden/abi_signatures_jpegdec.txt.
 * Additive: it changed neither MTGS_RAST_ABI_VERSION nor MTGS_RAST_HOT_ABI_VERSION.  Conventions (device pointers unless marked
 * HOST, `stream`, return codes, mtgs_rast_last_error) are mtgs_rast.h's.
 *
 * The file is parsed on the host (mtgs_amd.jpegdec.parse_jpeg); what reaches this entry is the entropy-coded segment (`scan`, the
 * bytes between the SOS header and EOI, stuffed zeros and restart markers included) and one table of int32 words.  The pixels are
 * byte for byte what Pillow 12.2.0 (libjpeg-turbo: the integer "islow" IDCT, "fancy" upsampling, 16-bit fixed-point colour) gives
 * for the same file: 8-bit baseline sequential DCT, three components read as YCbCr, ONE interleaved scan, luma sampled 1x1
 * (MTGS_JPEGDEC_444), 2x1 (_422) or 2x2 (_420) with chroma 1x1.  Exactness is claimed for files whose IDCT stays inside the
 * library's sample range, which every file an encoder writes does; hand-made quantisation tables that drive it out are out of scope.
 *
 * `tables`, MTGS_JPEGDEC_TABLE_WORDS int32 words.  A Huffman slot is 0 / 1 for the DC tables 0 / 1 and 2 / 3 for the AC tables 0 / 1:
 *   QUANT_AT    [3][64]   the quantisation table of each component, NATURAL order
 *   FAST_AT     [4][1024] by the next MTGS_JPEGDEC_FAST_BITS bits of the stream: (code length << 8) | symbol, 0 if no code that short
 *   MAXCODE_AT  [4][18]   the largest code of length l at [l], -1 if there is none (Annex F.2.2.3)
 *   VALOFF_AT   [4][18]   index into HUFFVAL of the first code of length l, minus that code
 *   HUFFVAL_AT  [4][256]  the symbols
 *   SLOT_AT     [3][2]    each component's DC slot and AC slot
 *
 * The entropy stage (one serial bit stream, no restart markers unless the writer asked for them):
 *   clean     a prefix sum (scan.hpp) drops the stuffed zeros (FF 00) and the restart markers (FF D0..D7) and counts the markers in
 *             its high half: a clean byte stream, padded with 0xFF, and the clean byte at which each restart interval starts
 *   cut       every interval is cut into subsequences of `subsequence_bits` bits (a multiple of 32), counted by a second prefix sum
 *   sync      a decoder state is (bit position, block within the MCU, zigzag index; index 0: a DC code comes next).  The state at an
 *             interval's start is (start, 0, 0), exactly.  Every other subsequence starts from the guess (its first bit, 0, 0).  One
 *             step decodes subsequence i from entry[i] until the position reaches the subsequence's end and stores that state as
 *             entry[i + 1].  When a step changes no entry, the entries are the sequential decoder's own: entry[0] is exact, an exact
 *             entry gives an exact exit, and equality carries exactness forward -- whether or not any guess ever synchronised.  A
 *             workgroup iterates over its MTGS_JPEGDEC_RUN subsequences inside one launch (at most RUN times, leaving early when
 *             nothing changed); the launches are repeated once per workgroup of the stream (a count that depends on the scan's length
 *             only), and a device flag turns a launch into a no-op once the one before it changed nothing.  No host read, no
 *             grid-wide barrier, no loop without a constant bound.
 *   count     the blocks each subsequence completes from its exact entry, through one exclusive prefix sum
 *   write     every lane decodes its subsequence once more and writes int16 coefficients into a zeroed [block][64] buffer (natural
 *             order); a block that straddles two subsequences is written by both lanes at disjoint indices; the DC is written as
 *             the difference; blocks beyond an interval's count (decoded from the padding) are dropped
 *   DC        per-component prefix sums over the blocks in stream order; the prefix at the interval's first block (an index that is
 *             arithmetic, the intervals having a fixed block count) is subtracted
 * Speculative decoding cannot leave bounds, whatever the bytes are:
 *   - every step of a decode consumes at least one bit (a code has at least one; a prefix that is no code skips one), and the loop
 *     over a subsequence is bounded by its bit count, so it ends;
 *   - every table index is masked to its table's size (the fast index is a 10-bit field, HUFFVAL's & 255, a slot & 3, a category
 *     & 15, the block within the MCU is reduced below the MCU's block count);
 *   - every stream read is clamped to the last word of the padded clean stream;
 *   - every coefficient write is guarded by the interval's block count and by index 63;
 *   - interval starts are clamped to the clean length, subsequence indices to the capacity the host derived from the scan's length;
 *   - the DC prefix sums run over the whole image, not per interval, in int64 and are kept as int32 (Cb and Cr as the two signed
 *     halves of one sum).  A file of very many restart intervals with extreme DC values can make them wrap; a DC is the DIFFERENCE
 *     of two of them, which is right modulo 2^32 whatever wrapped, and no index is ever derived from one;
 *   - the host queues one synchronisation launch per workgroup of the stream, each of that many workgroups: W launches of W
 *     workgroups for W = ceil(subsequences / MTGS_JPEGDEC_RUN), W <= 2^27 * 8 / 32 / 256 + 256.  A launch that finds the flag of the
 *     one before it clear returns at its first instruction; what those cost is in profiles/jpegdec.txt.
 *
 * The pixel stages:
 *   IDCT      dequantise, jidctint's islow butterfly at 13 bits (2446 3196 4433 6270 7373 9633 12299 15137 16069 16819 20995 25172),
 *             columns with DESCALE(x, 11), then rows with DESCALE(x, 18), DESCALE(x, n) = (x + (1 << (n - 1))) >> n; output
 *             clamp(v + 128, 0, 255) into planes at component resolution
 *   upsample  chroma edges are the component's TRUE size, ceil(W / 2) (x ceil(H / 2)).  h2v1: even output (3 c + left + 1) >> 2, odd
 *             (3 c + right + 2) >> 2, the outermost outputs the sample itself.  h2v2: s = 3 c + (the row above for an even output
 *             row, below for an odd one, replicated at top and bottom); even columns (3 s + s_left + 8) >> 4, odd (3 s + s_right +
 *             7) >> 4, the outermost (4 s + 8) >> 4 and (4 s + 7) >> 4.  A chroma component of one or two samples' width is
 *             replicated instead, as jdsample.c chooses its fancy routines only for components wider than two samples
 *   colour    R = Y + ((91881 (Cr - 128) + 32768) >> 16), B = Y + ((116130 (Cb - 128) + 32768) >> 16),
 *             G = Y + ((-22554 (Cb - 128) - 46802 (Cr - 128) + 32768) >> 16), each clamped to 0..255
 *   store     uint8, or float32 byte / 255 as ONE correctly rounded division, at strides in ELEMENTS
 *
 * status, int32[MTGS_JPEGDEC_STATUS_WORDS]: [0] an error word (0 for a well-formed file; MTGS_JPEGDEC_ERR_MARKERS: the restart
 * markers found are not the intervals - 1; MTGS_JPEGDEC_ERR_BLOCKS: an interval held fewer blocks than it must), [1] the stream
 * blocks decoded (per interval at most its count), [2] the blocks expected, [3] the synchronisation launches that changed an entry.
 *
 * mtgs_jpegdec_sizes: the workspace bytes (16-byte aligned) for a scan of `scan_bytes` bytes.
 * mtgs_jpegdec_decode: subsequence_bits 0 = MTGS_JPEGDEC_SUBSEQUENCE_BITS; restart_interval in MCUs, 0 = none.
 * Limits: 1 <= h, w <= 65535; 1 <= scan_bytes < 2^27; subsequence_bits a multiple of 32 in [32, 65536]. */
#define MTGS_JPEGDEC_QUANT_AT 0
#define MTGS_JPEGDEC_FAST_AT 192
#define MTGS_JPEGDEC_MAXCODE_AT 4288
#define MTGS_JPEGDEC_VALOFF_AT 4360
#define MTGS_JPEGDEC_HUFFVAL_AT 4432
#define MTGS_JPEGDEC_SLOT_AT 5456
#define MTGS_JPEGDEC_TABLE_WORDS 5464
#define MTGS_JPEGDEC_FAST_BITS 10
#define MTGS_JPEGDEC_RUN 256
#define MTGS_JPEGDEC_SUBSEQUENCE_BITS 512
#define MTGS_JPEGDEC_STATUS_WORDS 4
enum { MTGS_JPEGDEC_444 = 0, MTGS_JPEGDEC_422 = 1, MTGS_JPEGDEC_420 = 2 };
enum { MTGS_JPEGDEC_ERR_MARKERS = 1, MTGS_JPEGDEC_ERR_BLOCKS = 2 };

int mtgs_jpegdec_sizes(int h, int w, int subsampling, int restart_interval, int64_t scan_bytes, int subsequence_bits,
                       size_t *ws_bytes);
int mtgs_jpegdec_decode(const uint8_t *scan, int64_t scan_bytes, const int32_t *tables, int h, int w, int subsampling,
                        int restart_interval, int subsequence_bits, void *out, int is_float, int64_t stride_y, int64_t stride_x,
                        int64_t stride_c, int32_t *status, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MTGS_JPEGDEC_H */
