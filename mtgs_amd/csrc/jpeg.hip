// jpeg.hip -- presented frames as baseline JPEG on the device (include/mtgs_jpeg.h states the arithmetic; gfx950).
//
//   blocks_kernel<SUB>   ONE workgroup per MCU (256 threads for the 16 x 16 pixels of 4:2:0, 64 for the 8 x 8 of 4:4:4): every thread
//                        loads one pixel (edges repeated by clamping the coordinates; float32 converted as mtgs_present.h's uint8
//                        formats), the colour transform, at 4:2:0 the h2v2 average from LDS; 8 threads per block run the row
//                        pass of the butterfly, then the column pass; one thread per coefficient quantises into zigzag order;
//                        then a WAVE per block writes its 64 int16 (a dummy block: the DC of the block before it, zeros) and sums
//                        the lengths of its AC codes (lane = zigzag position, the run before a coefficient from a ballot).
//   mtgs_scan::run       value(i) = AC bits + the DC code of the difference to the previous block of the component (its index is
//                        arithmetic on i); the sink keeps each block's bit offset, the spine the total.
//   clear_kernel         zeroes the packed words the total covers (a kernel, not a memset node: common.hpp) and copies the header.
//   pack_kernel          a wave per block: lane k builds the code of coefficient k, a wave prefix sum places it, LDS atomic ORs
//                        assemble the block's words at its bit offset (word-aligned with the global buffer).  Whole words are plain
//                        stores; the first and the last word of a block, which neighbours may share, are vector atomic ORs into the
//                        zeroed buffer: order-independent, so the stream is bitwise reproducible.  Words hold the stream MSB first.
//   mtgs_scan::run       value(c) = the 0xFF bytes of 16-byte chunk c of the packed stream (the last byte padded with 1-bits);
//                        the sink writes chunk c behind the header at 16 c + (0xFF before it), 0x00 after every 0xFF, every store
//                        checked against the capacity; the sink of the last chunk writes EOI, the length and the overflow flag.
// Only the last stage writes to the caller's buffer.  The packed stream lives in the workspace, whose size is the worst case
// of the block count, so no kernel's addresses depend on the pixels beyond that bound: MTGS_JPEG_BLOCK_BITS per block holds because
// the categories are clamped to what 8-bit samples can reach (11 for a DC difference, 10 for an AC coefficient).
#include "common.hpp"
#include "jpeg_zigzag.hpp"
#include "sample_u8.hpp"
#include "scan.hpp"

namespace {

constexpr int HEADER = MTGS_JPEG_HEADER_BYTES;
constexpr int BLOCK_BITS = MTGS_JPEG_BLOCK_BITS;
constexpr int CHUNK = MTGS_JPEG_CHUNK_BYTES;
static_assert(CHUNK == 16, "a chunk is one 16-byte load");
constexpr int BLOCK_WORDS = (31 + BLOCK_BITS + 31) / 32 + 2;   // a block's words at any bit offset inside its first word, + slack
constexpr int PACK_WAVES = 4;
constexpr int DQT0_AT = 2 + 18 + 5, DQT1_AT = DQT0_AT + 69;   // the 64 entries of table 0 and of table 1 inside the header

// ---- tables: ITU-T T.81 Annex K ------------------------------------------------------------------------------------------------------
constexpr uint8_t ZIGZAG[64] = {MTGS_JPEG_ZIGZAG};
__constant__ uint8_t c_zigzag[64] = {MTGS_JPEG_ZIGZAG};

constexpr uint8_t BASE_Q[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

struct HuffSpec {
    uint8_t bits[16];
    uint8_t n_vals;
    uint8_t vals[162];
};
constexpr HuffSpec DC_LUMA = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr HuffSpec DC_CHROMA = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr HuffSpec AC_LUMA = {
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, 162,
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa}};
constexpr HuffSpec AC_CHROMA = {
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}, 162,
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa}};

// code and length by symbol: Annex C's canonical assignment, done by the compiler
struct Huff {
    uint16_t code[256];
    uint8_t len[256];
};
constexpr Huff make_huff(const HuffSpec &s) {
    Huff h{};
    unsigned code = 0;
    int k = 0;
    for (int length = 1; length <= 16; ++length) {
        for (int j = 0; j < s.bits[length - 1]; ++j, ++k, ++code) {
            h.code[s.vals[k]] = (uint16_t)code;
            h.len[s.vals[k]] = (uint8_t)length;
        }
        code <<= 1;
    }
    return h;
}
constexpr Huff H_DC_LUMA = make_huff(DC_LUMA), H_AC_LUMA = make_huff(AC_LUMA), H_DC_CHROMA = make_huff(DC_CHROMA),
               H_AC_CHROMA = make_huff(AC_CHROMA);
__constant__ Huff c_dc[2] = {H_DC_LUMA, H_DC_CHROMA};     // [0] Y, [1] Cb and Cr
__constant__ Huff c_ac[2] = {H_AC_LUMA, H_AC_CHROMA};

struct QuantTables {
    uint8_t q[2][64];   // zigzag order, as DQT holds them
};

QuantTables quant_tables(int quality) {
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    QuantTables t;
    for (int c = 0; c < 2; ++c)
        for (int k = 0; k < 64; ++k) {
            const int v = (BASE_Q[c][ZIGZAG[k]] * scale + 50) / 100;
            t.q[c][k] = (uint8_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
        }
    return t;
}

// ---- geometry --------------------------------------------------------------------------------------------------------------------
struct Geometry {
    int side, per_mcu, mcus_x, mcus_y;
    int64_t n_blocks, max_bytes, n_chunks;
};

Geometry geometry(int h, int w, int subsampling) {
    Geometry g;
    g.side = subsampling == MTGS_JPEG_420 ? 16 : 8;
    g.per_mcu = subsampling == MTGS_JPEG_420 ? 6 : 3;
    g.mcus_x = (w + g.side - 1) / g.side;
    g.mcus_y = (h + g.side - 1) / g.side;
    g.n_blocks = (int64_t)g.mcus_x * g.mcus_y * g.per_mcu;
    g.max_bytes = ceil_div64(g.n_blocks * BLOCK_BITS, 8);
    g.n_chunks = ceil_div64(g.max_bytes, CHUNK) + 1;   // the last chunk lies beyond any stream: its sink finishes the file
    return g;
}

size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

struct Workspace {
    int16_t *coef;        // [n_blocks][64]
    int32_t *ac_bits;     // [n_blocks]
    int64_t *bit_offset;  // [n_blocks]
    int64_t *totals;      // [0] bits of the scan, [1] its 0xFF bytes
    int64_t *spine_a, *spine_b;
    uint32_t *words;      // [n_chunks][4]
    size_t bytes;
};

Workspace carve(const Geometry &g, void *base) {
    Workspace w;
    size_t at = 0;
    auto take = [&](size_t n) {
        char *p = (char *)base + at;
        at += align16(n);
        return p;
    };
    w.words = (uint32_t *)take((size_t)g.n_chunks * CHUNK);
    w.coef = (int16_t *)take((size_t)g.n_blocks * 64 * sizeof(int16_t));
    w.bit_offset = (int64_t *)take((size_t)g.n_blocks * sizeof(int64_t));
    w.totals = (int64_t *)take(2 * sizeof(int64_t));
    w.spine_a = (int64_t *)take(mtgs_scan::workspace_bytes(g.n_blocks));
    w.spine_b = (int64_t *)take(mtgs_scan::workspace_bytes(g.n_chunks));
    w.ac_bits = (int32_t *)take((size_t)g.n_blocks * sizeof(int32_t));
    w.bytes = at;
    return w;
}

// ---- device pieces ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// jfdctint's butterfly on d[0..7]: FIRST = the row pass (results scaled up by PASS1_BITS), otherwise the column pass
template <bool FIRST>
__device__ __forceinline__ void dct8(int *d) {
    constexpr int LOW = FIRST ? 13 - 2 : 13 + 2;
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    d[0] = FIRST ? (t10 + t11) * 4 : descale(t10 + t11, 2);
    d[4] = FIRST ? (t10 - t11) * 4 : descale(t10 - t11, 2);
    int z1 = (t12 + t13) * 4433;
    d[2] = descale(z1 + t13 * 6270, LOW);
    d[6] = descale(z1 - t12 * 15137, LOW);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
    z1 *= -7373, z2 *= -20995, z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
    d[7] = descale(a4 + z1 + z3, LOW);
    d[5] = descale(a5 + z2 + z4, LOW);
    d[3] = descale(a6 + z2 + z3, LOW);
    d[1] = descale(a7 + z1 + z4, LOW);
}

constexpr int fix16(double x) { return (int)(x * 65536 + 0.5); }

// The code of one lane of a block: lane k holds v, coefficient k in zigzag order (k = 0: the DC DIFFERENCE).  `nonzero` has bit k
// set for every k >= 1 with a non-zero coefficient.  Returns the bits of the code proper (`code`, `len` <= 26, the Huffman code
// followed by the magnitude bits) and the number of ZRL codes before it.  Lane 63 of a block that ends in zeros holds EOB.
struct LaneCode {
    uint32_t code;
    int len, n_zrl;
};

__device__ __forceinline__ LaneCode lane_code(int k, int v, uint64_t nonzero, int table) {
    LaneCode c{0, 0, 0};
    const int a = v < 0 ? -v : v;
    int cat = 32 - __clz(a);                  // the bit length; 0 for 0
    const int low = v < 0 ? v - 1 : v;
    if (k == 0) {
        cat = cat > 11 ? 11 : cat;            // 8-bit samples cannot exceed it; the clamp makes the bound on a block's bits unconditional
        c.code = ((uint32_t)c_dc[table].code[cat] << cat) | ((uint32_t)low & ((1u << cat) - 1));
        c.len = c_dc[table].len[cat] + cat;
    } else if (v != 0) {
        cat = cat > 10 ? 10 : cat;
        const uint64_t below = (nonzero | 1) & ((1ull << k) - 1);   // bit 0 stands for the DC: never empty
        const int run = k - (63 - __clzll((long long)below)) - 1;
        const int sym = ((run & 15) << 4) | cat;
        c.n_zrl = run >> 4;
        c.code = ((uint32_t)c_ac[table].code[sym] << cat) | ((uint32_t)low & ((1u << cat) - 1));
        c.len = c_ac[table].len[sym] + cat;
    } else if (k == 63) {                     // zeros remain at the end: EOB
        c.code = c_ac[table].code[0];
        c.len = c_ac[table].len[0];
    }
    return c;
}

__device__ __forceinline__ int code_bits(const LaneCode &c, int table) { return c.len + c.n_zrl * c_ac[table].len[0xF0]; }

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the block before block i of the same component in scan order, -1 for the first
template <int NB>
__device__ __forceinline__ int64_t predecessor(int64_t i) {
    const int64_t mcu = i / NB;
    const int j = (int)(i - mcu * NB);
    if (NB == 6 && j >= 1 && j <= 3) return i - 1;
    if (mcu == 0) return -1;
    return NB == 6 && j == 0 ? i - 3 : i - NB;
}

__device__ __forceinline__ int component_table(int per_mcu, int64_t i) { return (int)(i % per_mcu) < per_mcu - 2 ? 0 : 1; }

// ---- 1. blocks -------------------------------------------------------------------------------------------------------------------
template <int SUB>
__global__ __launch_bounds__(SUB == MTGS_JPEG_420 ? 256 : 64) void jpeg_blocks_kernel(
    const void *__restrict__ image, bool is_float, bool round, int H, int W, int64_t sy, int64_t sx, int64_t sc,
    const uint8_t *__restrict__ header, int mcus_x, int16_t *__restrict__ coef, int32_t *__restrict__ ac_bits) {
    constexpr bool S420 = SUB == MTGS_JPEG_420;
    constexpr int SIDE = S420 ? 16 : 8, NT = SIDE * SIDE, NB = S420 ? 6 : 3, NY = NB - 2;
    __shared__ int s_blk[NB][64];                      // samples - 128, then the transform in place; natural order
    __shared__ int16_t s_chroma[S420 ? 2 : 1][16][16];   // 4:2:0: Cb and Cr at full resolution
    __shared__ int16_t s_q[NB][64];                    // quantised, zigzag order
    const int t = threadIdx.x;
    const int mx = blockIdx.x % mcus_x, my = blockIdx.x / mcus_x;
    {
        const int px = t % SIDE, py = t / SIDE;
        const int x = min(mx * SIDE + px, W - 1), y = min(my * SIDE + py, H - 1);   // the last column and row repeated
        const int64_t at = y * sy + x * sx;
        const int r = load_sample(image, is_float, round, at), g = load_sample(image, is_float, round, at + sc),
                  b = load_sample(image, is_float, round, at + 2 * sc);
        const int Y = (fix16(.299) * r + fix16(.587) * g + fix16(.114) * b + 32768) >> 16;
        const int Cb = (-fix16(.16874) * r - fix16(.33126) * g + fix16(.5) * b + (128 << 16) + 32767) >> 16;
        const int Cr = (fix16(.5) * r - fix16(.41869) * g - fix16(.08131) * b + (128 << 16) + 32767) >> 16;
        const int at8 = (py & 7) * 8 + (px & 7);
        if (S420) {
            s_blk[(py >> 3) * 2 + (px >> 3)][at8] = Y - 128;
            s_chroma[0][py][px] = (int16_t)Cb;
            s_chroma[1][py][px] = (int16_t)Cr;
        } else {
            s_blk[0][at8] = Y - 128;
            s_blk[1][at8] = Cb - 128;
            s_blk[2][at8] = Cr - 128;
        }
    }
    __syncthreads();
    if constexpr (S420) {
        if (t < 128) {
            // rows were repeated at full resolution up to an even height only (the clamp above does that for row H of an odd H);
            // below the last chroma row it is the DOWNSAMPLED row that repeats
            const int c = t >> 6, i = t & 7;
            const int last = (H + 1) / 2 - 1 - my * 8;     // >= 0: the MCU holds a pixel row
            const int j = min((t >> 3) & 7, last);
            const int16_t(*p)[16] = s_chroma[c];
            s_blk[4 + c][((t >> 3) & 7) * 8 + i] =
                ((p[2 * j][2 * i] + p[2 * j][2 * i + 1] + p[2 * j + 1][2 * i] + p[2 * j + 1][2 * i + 1] + 1 + (i & 1)) >> 2) - 128;
        }
        __syncthreads();
    }
    if (t < NB * 8) {                                  // rows
        int *row = s_blk[t >> 3] + (t & 7) * 8;
        int d[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = row[k];
        dct8<true>(d);
#pragma unroll
        for (int k = 0; k < 8; ++k) row[k] = d[k];
    }
    __syncthreads();
    if (t < NB * 8) {                                  // columns
        int *col = s_blk[t >> 3] + (t & 7);
        int d[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = col[8 * k];
        dct8<false>(d);
#pragma unroll
        for (int k = 0; k < 8; ++k) col[8 * k] = d[k];
    }
    __syncthreads();
    for (int e = t; e < NB * 64; e += NT) {
        const int b = e >> 6, k = e & 63;
        const int c = s_blk[b][c_zigzag[k]];
        const int entry = header[(b < NY ? DQT0_AT : DQT1_AT) + k];   // zigzag order, as DQT holds it
        const int d = (entry < 1 ? 1 : entry) << 3;
        const int q = ((c < 0 ? -c : c) + (d >> 1)) / d;
        s_q[b][k] = (int16_t)(c < 0 ? -q : q);
    }
    __syncthreads();
    const int lane = t & 63;
    const int64_t first = (int64_t)blockIdx.x * NB;
    for (int b = t >> 6; b < NB; b += NT / 64) {       // a wave per block
        int src = b;
        if (S420 && b < 4) {
            // a luma block beyond the component's real blocks takes the DC of the block before it in this MCU; block 0 is real
            const int real_x = (W + 7) / 8 - 2 * mx, real_y = (H + 7) / 8 - 2 * my;
            while (src > 0 && ((src & 1) >= real_x || (src >> 1) >= real_y)) --src;
        }
        const int v = src == b ? s_q[b][lane] : (lane == 0 ? s_q[src][0] : 0);
        coef[(first + b) * 64 + lane] = (int16_t)v;
        const uint64_t nonzero = __ballot(lane > 0 && v != 0);
        const int table = b < NY ? 0 : 1;
        const int bits = wave_sum_i32(lane == 0 ? 0 : code_bits(lane_code(lane, v, nonzero, table), table));
        if (lane == 0) ac_bits[first + b] = bits;
    }
}

// ---- 2. offsets ------------------------------------------------------------------------------------------------------------------
template <int NB>
__device__ __forceinline__ int dc_difference(const int16_t *coef, int64_t i) {
    const int64_t p = predecessor<NB>(i);
    return (int)coef[i * 64] - (p < 0 ? 0 : (int)coef[p * 64]);
}

template <int NB>
struct BitsValue {
    const int16_t *coef;
    const int32_t *ac_bits;
    __device__ int64_t operator()(int64_t i) const {
        return ac_bits[i] + lane_code(0, dc_difference<NB>(coef, i), 0, component_table(NB, i)).len;
    }
};

struct OffsetSink {
    int64_t *bit_offset;
    __device__ void operator()(int64_t i, int64_t excl, int64_t) const { bit_offset[i] = excl; }
};

// ---- 3. clear and pack -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void jpeg_clear_kernel(const int64_t *__restrict__ totals, uint32_t *__restrict__ words,
                                                         const uint8_t *__restrict__ header, uint8_t *__restrict__ data, int64_t capacity) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t used = (totals[0] + 31) >> 5;        // <= the words of the workspace: the total is at most BLOCK_BITS per block
    if (4 * i < used) ((uint4 *)words)[i] = make_uint4(0, 0, 0, 0);   // whole 16-byte groups: the buffer is a whole number of chunks
    if (i < HEADER && i < capacity) data[i] = header[i];
}

__device__ __forceinline__ void put_bits(uint32_t *words, int at, uint32_t value, int len) {
    // value < 2^len, 1 <= len <= 32, bit `at` counted MSB first from words[0]
    const uint64_t x = (uint64_t)value << (64 - (at & 31) - len);
    atomicOr(words + (at >> 5), (uint32_t)(x >> 32));
    if ((uint32_t)x) atomicOr(words + (at >> 5) + 1, (uint32_t)x);
}

template <int NB>
__global__ __launch_bounds__(64 * PACK_WAVES) void jpeg_pack_kernel(int64_t n_blocks, const int16_t *__restrict__ coef,
                                                                    const int64_t *__restrict__ bit_offset, uint32_t *__restrict__ words) {
    __shared__ uint32_t s_words[PACK_WAVES][BLOCK_WORDS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * PACK_WAVES + wave;
    const bool active = i < n_blocks;
    uint32_t *mine = s_words[wave];
    if (lane < BLOCK_WORDS) mine[lane] = 0;
    static_assert(BLOCK_WORDS <= 64, "a lane per word");
    __syncthreads();
    int64_t offset = 0;
    int total = 0;
    if (active) {
        offset = bit_offset[i];
        const int table = component_table(NB, i);
        const int v = lane == 0 ? dc_difference<NB>(coef, i) : (int)coef[i * 64 + lane];
        const uint64_t nonzero = __ballot(lane > 0 && v != 0);
        const LaneCode c = lane_code(lane, v, nonzero, table);
        const int bits = code_bits(c, table);
        int incl = bits;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        total = __shfl(incl, 63, 64);                  // <= BLOCK_BITS: lane_code clamps the categories
        int at = (int)(offset & 31) + incl - bits;
        for (int z = 0; z < c.n_zrl; ++z) {
            put_bits(mine, at, c_ac[table].code[0xF0], c_ac[table].len[0xF0]);
            at += c_ac[table].len[0xF0];
        }
        if (c.len) put_bits(mine, at, c.code, c.len);
    }
    __syncthreads();
    if (active) {
        const int n = ((int)(offset & 31) + total + 31) >> 5;   // <= BLOCK_WORDS - 2
        if (lane < n) {
            const uint32_t w = mine[lane];
            uint32_t *out = words + (offset >> 5) + lane;
            if (lane == 0 || lane == n - 1) {
                if (w) atomicOr(out, w);               // a word that the neighbouring block may share
            } else {
                *out = w;
            }
        }
    }
}

// ---- 4. stuffing -----------------------------------------------------------------------------------------------------------------
// the bytes of chunk c of the packed stream that belong to it (the last byte of the stream padded with 1-bits)
struct Chunk {
    uint32_t w[4];
    int count;
    __device__ __forceinline__ uint32_t byte(int j) const { return (w[j >> 2] >> (24 - 8 * (j & 3))) & 0xFF; }
};

__device__ __forceinline__ Chunk load_chunk(const uint32_t *words, int64_t c, int64_t bits) {
    Chunk k{};
    const int64_t n_bytes = (bits + 7) >> 3, first = c * CHUNK;
    k.count = (int)(n_bytes - first < 0 ? 0 : (n_bytes - first > CHUNK ? CHUNK : n_bytes - first));
    if (k.count == 0) return k;
    const uint4 q = ((const uint4 *)words)[c];
    k.w[0] = q.x, k.w[1] = q.y, k.w[2] = q.z, k.w[3] = q.w;
    if ((bits & 7) && first + k.count == n_bytes) {
        const uint32_t pad = (1u << (8 - (int)(bits & 7))) - 1;
#pragma unroll
        for (int j = 0; j < CHUNK; ++j)       // unrolled: the words stay in registers
            if (j == k.count - 1) k.w[j >> 2] |= pad << (24 - 8 * (j & 3));
    }
    return k;
}

struct StuffValue {
    const uint32_t *words;
    const int64_t *totals;
    __device__ int64_t operator()(int64_t c) const {
        const Chunk k = load_chunk(words, c, totals[0]);
        int n = 0;
#pragma unroll
        for (int j = 0; j < CHUNK; ++j) n += j < k.count && k.byte(j) == 0xFF;
        return n;
    }
};

struct StuffSink {
    const uint32_t *words;
    const int64_t *totals;
    uint8_t *data;
    int64_t capacity, n_chunks;
    int64_t *meta;
    __device__ void operator()(int64_t c, int64_t excl, int64_t incl) const {
        const int64_t bits = totals[0];
        const Chunk k = load_chunk(words, c, bits);
        int64_t at = HEADER + c * CHUNK + excl;
#pragma unroll
        for (int j = 0; j < CHUNK; ++j) {
            if (j >= k.count) break;
            const uint32_t b = k.byte(j);
            if (at < capacity) data[at] = (uint8_t)b;
            ++at;
            if (b == 0xFF) {
                if (at < capacity) data[at] = 0;
                ++at;
            }
        }
        if (c == n_chunks - 1) {                       // beyond the stream: `incl` is the count of all its 0xFF bytes
            const int64_t end = HEADER + ((bits + 7) >> 3) + incl;
            if (end < capacity) data[end] = 0xFF;
            if (end + 1 < capacity) data[end + 1] = 0xD9;
            meta[0] = end + 2;
            meta[1] = end + 2 > capacity ? 1 : 0;
        }
    }
};

// ---- host ------------------------------------------------------------------------------------------------------------------------
int check_shape(const char *fn, int h, int w, int subsampling) {
    MTGS_REQUIRE(subsampling == MTGS_JPEG_420 || subsampling == MTGS_JPEG_444, MTGS_EUNSUPPORTED,
                 "%s: subsampling %d is not implemented (MTGS_JPEG_420 or MTGS_JPEG_444)", fn, subsampling);
    MTGS_REQUIRE(h >= 1 && h <= 65535 && w >= 1 && w <= 65535, MTGS_EINVAL, "%s: h and w outside [1, 65535] (%d, %d)", fn, h, w);
    MTGS_REQUIRE(geometry(h, w, subsampling).n_blocks * BLOCK_BITS < ((int64_t)1 << 31), MTGS_EINVAL,
                 "%s: %d x %d has too many blocks: their bits must stay below 2^31", fn, h, w);
    return MTGS_OK;
}

void put_segment(uint8_t *&p, int marker, const uint8_t *payload, int n) {
    *p++ = 0xFF, *p++ = (uint8_t)marker, *p++ = (uint8_t)((n + 2) >> 8), *p++ = (uint8_t)((n + 2) & 0xFF);
    for (int i = 0; i < n; ++i) *p++ = payload[i];
}

}  // namespace

extern "C" int mtgs_jpeg_sizes(int h, int w, int subsampling, size_t *ws_bytes, size_t *capacity) {
    const char *fn = "mtgs_jpeg_sizes";
    if (int rc = check_shape(fn, h, w, subsampling)) return rc;
    const Geometry g = geometry(h, w, subsampling);
    if (ws_bytes) *ws_bytes = carve(g, nullptr).bytes;
    if (capacity) *capacity = (size_t)(HEADER + 2 * g.max_bytes + 2);
    return MTGS_OK;
}

extern "C" int mtgs_jpeg_header(int h, int w, int quality, int subsampling, uint8_t *header, size_t header_capacity) {
    const char *fn = "mtgs_jpeg_header";
    if (int rc = check_shape(fn, h, w, subsampling)) return rc;
    MTGS_REQUIRE(quality >= 1 && quality <= 100, MTGS_EINVAL, "%s: quality outside [1, 100] (%d)", fn, quality);
    MTGS_REQUIRE(header != nullptr, MTGS_EINVAL, "%s: null pointer: header", fn);
    MTGS_REQUIRE(header_capacity >= (size_t)HEADER, MTGS_EINVAL, "%s: header_capacity %zu < %d bytes", fn, header_capacity, HEADER);
    uint8_t *p = header;
    *p++ = 0xFF, *p++ = 0xD8;
    const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    put_segment(p, 0xE0, jfif, 14);
    const QuantTables qt = quant_tables(quality);
    for (int c = 0; c < 2; ++c) {
        uint8_t dqt[65] = {(uint8_t)c};
        for (int k = 0; k < 64; ++k) dqt[1 + k] = qt.q[c][k];
        put_segment(p, 0xDB, dqt, 65);
    }
    const uint8_t sof[15] = {8, (uint8_t)(h >> 8), (uint8_t)(h & 0xFF), (uint8_t)(w >> 8), (uint8_t)(w & 0xFF), 3,
                             1, (uint8_t)(subsampling == MTGS_JPEG_420 ? 0x22 : 0x11), 0, 2, 0x11, 1, 3, 0x11, 1};
    put_segment(p, 0xC0, sof, 15);
    const HuffSpec *specs[4] = {&DC_LUMA, &AC_LUMA, &DC_CHROMA, &AC_CHROMA};
    const uint8_t ids[4] = {0x00, 0x10, 0x01, 0x11};
    for (int s = 0; s < 4; ++s) {
        uint8_t dht[1 + 16 + 162] = {ids[s]};
        for (int k = 0; k < 16; ++k) dht[1 + k] = specs[s]->bits[k];
        for (int k = 0; k < specs[s]->n_vals; ++k) dht[17 + k] = specs[s]->vals[k];
        put_segment(p, 0xC4, dht, 17 + specs[s]->n_vals);
    }
    const uint8_t sos[10] = {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
    put_segment(p, 0xDA, sos, 10);
    MTGS_REQUIRE(p - header == HEADER, MTGS_EINVAL, "%s: the header came to %d bytes, not %d", fn, (int)(p - header), HEADER);
    return MTGS_OK;
}

extern "C" int mtgs_jpeg_encode(const void *image, int is_float, int conversion, int h, int w, int64_t stride_y, int64_t stride_x,
                                int64_t stride_c, int subsampling, const uint8_t *header, uint8_t *data, size_t capacity,
                                int64_t *meta, void *ws, size_t ws_bytes, void *stream) {
    const char *fn = "mtgs_jpeg_encode";
    if (int rc = check_shape(fn, h, w, subsampling)) return rc;
    MTGS_REQUIRE(conversion == MTGS_PRESENT_U8_TRUNCATE || conversion == MTGS_PRESENT_U8_ROUND, MTGS_EINVAL,
                 "%s: conversion must be MTGS_PRESENT_U8_TRUNCATE or MTGS_PRESENT_U8_ROUND (%d)", fn, conversion);
    MTGS_REQUIRE(stride_y >= 0 && stride_x >= 0 && stride_c >= 0, MTGS_EINVAL, "%s: negative stride (%lld, %lld, %lld)", fn,
                 (long long)stride_y, (long long)stride_x, (long long)stride_c);
    MTGS_REQUIRE(image != nullptr, MTGS_EINVAL, "%s: null pointer: image", fn);
    MTGS_REQUIRE(!is_float || ((uintptr_t)image & 3) == 0, MTGS_EINVAL, "%s: a float32 image must be 4-byte aligned", fn);
    MTGS_REQUIRE(header != nullptr, MTGS_EINVAL, "%s: null pointer: header", fn);
    MTGS_REQUIRE(data != nullptr || capacity == 0, MTGS_EINVAL, "%s: null pointer: data", fn);
    MTGS_REQUIRE(capacity < ((size_t)1 << 62), MTGS_EINVAL, "%s: capacity %zu is no size", fn, capacity);
    MTGS_REQUIRE(meta != nullptr && ((uintptr_t)meta & 7) == 0, MTGS_EINVAL, "%s: meta must be a non-null, 8-byte aligned int64[2]", fn);
    const Geometry g = geometry(h, w, subsampling);
    MTGS_REQUIRE(ws != nullptr, MTGS_EINVAL, "%s: null pointer: ws", fn);
    MTGS_REQUIRE(((uintptr_t)ws & 15) == 0, MTGS_EINVAL, "%s: workspace must be 16-byte aligned", fn);
    const Workspace k = carve(g, ws);
    MTGS_REQUIRE(ws_bytes >= k.bytes, MTGS_EWORKSPACE, "%s: workspace %zu < %zu bytes", fn, ws_bytes, k.bytes);
    hipStream_t st = (hipStream_t)stream;
    const unsigned mcus = (unsigned)(g.mcus_x * g.mcus_y);
    const bool round = conversion == MTGS_PRESENT_U8_ROUND;
    const unsigned clear_blocks = (unsigned)ceil_div64(g.n_chunks > HEADER ? g.n_chunks : HEADER, 256);
    const unsigned pack_blocks = (unsigned)ceil_div64(g.n_blocks, PACK_WAVES);
    if (subsampling == MTGS_JPEG_420) {
        jpeg_blocks_kernel<MTGS_JPEG_420><<<mcus, 256, 0, st>>>(image, is_float != 0, round, h, w, stride_y, stride_x, stride_c, header,
                                                                g.mcus_x, k.coef, k.ac_bits);
        mtgs_scan::run(g.n_blocks, BitsValue<6>{k.coef, k.ac_bits}, OffsetSink{k.bit_offset}, k.spine_a, k.totals, st);
        jpeg_clear_kernel<<<clear_blocks, 256, 0, st>>>(k.totals, k.words, header, data, (int64_t)capacity);
        jpeg_pack_kernel<6><<<pack_blocks, 64 * PACK_WAVES, 0, st>>>(g.n_blocks, k.coef, k.bit_offset, k.words);
    } else {
        jpeg_blocks_kernel<MTGS_JPEG_444><<<mcus, 64, 0, st>>>(image, is_float != 0, round, h, w, stride_y, stride_x, stride_c, header,
                                                               g.mcus_x, k.coef, k.ac_bits);
        mtgs_scan::run(g.n_blocks, BitsValue<3>{k.coef, k.ac_bits}, OffsetSink{k.bit_offset}, k.spine_a, k.totals, st);
        jpeg_clear_kernel<<<clear_blocks, 256, 0, st>>>(k.totals, k.words, header, data, (int64_t)capacity);
        jpeg_pack_kernel<3><<<pack_blocks, 64 * PACK_WAVES, 0, st>>>(g.n_blocks, k.coef, k.bit_offset, k.words);
    }
    mtgs_scan::run(g.n_chunks, StuffValue{k.words, k.totals}, StuffSink{k.words, k.totals, data, (int64_t)capacity, g.n_chunks, meta},
                   k.spine_b, k.totals + 1, st);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}
