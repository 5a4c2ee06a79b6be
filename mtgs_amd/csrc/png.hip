// png.hip -- depth and label planes as indexed PNG on the device (include/mtgs_png.h states the file and the rules; gfx950).
//
// The writer:
//   tokens_kernel   ONE workgroup per segment: the filtered bytes of the segment into LDS (the filter reads the image twice, the
//                   depth rule converts on load), run starts by a max scan and run ends by a min scan over LDS (log2 passes,
//                   ping-pong), the token of every position, the symbol histogram in LDS (one global add per used symbol) and the
//                   segment's two Adler-32 sums.
//   codes_kernel    ONE workgroup: rank sorts (a thread per symbol), the two-queue Huffman and Annex K.2's adjustment by thread 0,
//                   depths by a walk to the root per leaf, canonical codes per symbol; then thread 0 writes the code-length sequence
//                   and the block header's bits.
//   mtgs_scan::run  value(i) = the bits of position i's token; the sink keeps every position's bit offset and the segment table.
//   clear_kernel    zeroes the words the total covers (a kernel, not a memset node: common.hpp).
//   pack_kernel     2048 positions per workgroup: LDS atomic ORs assemble the tokens LSB first at their offsets; whole words are
//                   plain stores, the first and the last word, which a neighbour may share, vector atomic ORs into the zeroed buffer.
//   finish_kernel   ONE workgroup: the header's words, the end-of-block code and the Adler-32 bytes by atomic OR; the payload length.
//   emit_kernel     the file: the only launch that writes the caller's buffer, every store checked against the capacity.
// The reader:
//   inflate_kernel  one LANE per segment, the tables in LDS.  unfilter kernels: a workgroup per row (None, Sub: block prefix sums per
//                   channel) or a thread per pixel column (Up).  status_kernel: the Adler-32 of the decoded row stream.
// No address depends on the pixels beyond the worst-case sizes the host derives from (h, w, channels, segment_bytes).
#include "common.hpp"
#include "scan.hpp"

namespace {

constexpr int NSYM = 288;                       // lit/len symbols 0..285, padded
constexpr int MAX_SEG = MTGS_PNG_MAX_SEGMENT_BYTES;
constexpr int HDR_WORDS = (16 + MTGS_PNG_HEADER_BITS + 31) / 32 + 4;
constexpr uint32_t ADLER = 65521;
constexpr int PACK_TILE = 2048, TOKEN_BITS = 21; // a match: 15 + 5 extra + the distance bit
constexpr int PACK_WORDS = (31 + PACK_TILE * TOKEN_BITS + 31) / 32 + 2;
constexpr uint16_t COVERED = 0xFFFF;
constexpr int FAST_BITS = MTGS_PNG_FAST_BITS;

// ---- RFC 1951's length symbols -----------------------------------------------------------------------------------------------------
struct LengthTable {
    uint8_t sym[259];        // by length 3..258: symbol - 257
    uint16_t base[29];
    uint8_t extra[29];
};
constexpr LengthTable make_lengths() {
    LengthTable t{};
    const int extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    int base = 3;
    for (int s = 0; s < 29; ++s) {
        if (s == 28) base = 258;
        t.base[s] = (uint16_t)base;
        t.extra[s] = (uint8_t)extra[s];
        for (int k = 0; k < (1 << extra[s]) && base + k <= 258; ++k) t.sym[base + k] = (uint8_t)s;
        base += 1 << extra[s];
    }
    return t;
}
constexpr LengthTable LENGTHS = make_lengths();
static_assert(LENGTHS.base[27] == 227 && LENGTHS.sym[257] == 27 && LENGTHS.sym[258] == 28 && LENGTHS.sym[3] == 0, "RFC 1951 3.2.5");
__constant__ LengthTable c_lengths = LENGTHS;

// ---- geometry ----------------------------------------------------------------------------------------------------------------------
struct Geometry {
    int h, w, C, S;
    int64_t L, spr, nseg, N;
    int64_t max_payload, max_words, prefix;   // prefix: the file's bytes before the segment table
};

Geometry geometry(int h, int w, int C, int S) {
    Geometry g;
    g.h = h, g.w = w, g.C = C, g.S = S;
    g.L = 1 + (int64_t)w * C;
    g.spr = ceil_div64(g.L, S);
    g.nseg = g.spr * h;
    g.N = g.L * h;
    g.max_payload = 2 + ceil_div64(MTGS_PNG_HEADER_BITS + 15 * (g.N + 1), 8) + 4;
    g.max_words = ceil_div64(g.max_payload, 4) + 4;
    g.prefix = 8 + 25 + 8 + 16;
    return g;
}

struct Workspace {
    uint32_t *hist, *codes, *hdr, *seg_bits, *part_a, *part_b, *bit_off, *words;
    int64_t *info, *spine, *totals;
    uint16_t *tok;
    size_t bytes;
};

Workspace carve(const Geometry &g, void *base) {
    Workspace k;
    size_t at = 0;
    auto take = [&](size_t n) {
        char *p = (char *)base + at;
        at += (n + 15) & ~(size_t)15;
        return p;
    };
    k.hist = (uint32_t *)take(NSYM * 4);
    k.codes = (uint32_t *)take(NSYM * 4);
    k.hdr = (uint32_t *)take(HDR_WORDS * 4);
    k.info = (int64_t *)take(4 * 8);              // [0] header bits (78 01 included), [1] payload bytes, [2] end-of-block offset
    k.totals = (int64_t *)take(2 * 8);
    k.spine = (int64_t *)take(mtgs_scan::workspace_bytes(g.N));
    k.seg_bits = (uint32_t *)take((size_t)(g.nseg + 1) * 4);
    k.part_a = (uint32_t *)take((size_t)g.nseg * 4);
    k.part_b = (uint32_t *)take((size_t)g.nseg * 4);
    k.bit_off = (uint32_t *)take((size_t)g.N * 4);
    k.tok = (uint16_t *)take((size_t)g.N * 2);
    k.words = (uint32_t *)take((size_t)g.max_words * 4);
    k.bytes = at;
    return k;
}

// ---- the image as file bytes -------------------------------------------------------------------------------------------------------
struct Source {
    const void *image;
    int is_depth, C, order;
    int64_t sy, sx, sc;
    int rx, ry, rw, rh;
    float max_range, min_depth;
};

__device__ __forceinline__ uint32_t source_byte(const Source &s, int y, int x, int c) {   // c: the FILE's channel
    if (s.is_depth) {
        const int yy = y - s.ry, xx = x - s.rx;
        if (c == 0 || yy < 0 || yy >= s.rh || xx < 0 || xx >= s.rw) return 0;
        float d = ((const float *)s.image)[yy * s.sy + xx * s.sx];
        if (!(d <= s.max_range) || d < s.min_depth) d = 0.0f;            // NaN too
        const float t = __fmul_rn(d, 100.0f);
        return c == 2 ? (uint32_t)(uint8_t)fmodf(t, 256.0f) : (uint32_t)(uint8_t)floorf(__fdiv_rn(t, 256.0f));
    }
    return ((const uint8_t *)s.image)[y * s.sy + x * s.sx + (s.order ? s.C - 1 - c : c) * s.sc];
}

__device__ __forceinline__ uint32_t stream_byte(const Source &s, int filter, int y, int64_t j) {   // byte j of row y's stream
    if (j == 0) return (uint32_t)filter;
    const int x = (int)((j - 1) / s.C), c = (int)((j - 1) % s.C);
    const uint32_t cur = source_byte(s, y, x, c);
    uint32_t pred = 0;
    if (filter == MTGS_PNG_FILTER_SUB && x > 0) pred = source_byte(s, y, x - 1, c);
    if (filter == MTGS_PNG_FILTER_UP && y > 0) pred = source_byte(s, y - 1, x, c);
    return (cur - pred) & 255;
}

__device__ __forceinline__ int64_t block_sum_i64(int64_t v, int64_t *lds) {   // every thread receives the total; blockDim.x = 256
    v = wave_sum_all(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    return lds[0] + lds[1] + lds[2] + lds[3];
}

// ---- 1. tokens ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void png_tokens_kernel(Source src, int filter, int S, int64_t L, int64_t spr, int64_t N,
                                                         uint16_t *__restrict__ tok, uint32_t *__restrict__ hist,
                                                         uint32_t *__restrict__ part_a, uint32_t *__restrict__ part_b) {
    __shared__ uint8_t s_b[MAX_SEG];
    __shared__ uint16_t s_p[2][MAX_SEG], s_start[MAX_SEG];
    __shared__ uint32_t s_hist[NSYM];
    __shared__ int64_t s_red[4];
    const int t = threadIdx.x;
    const int64_t seg = blockIdx.x;
    const int y = (int)(seg / spr);
    const int64_t seg_off = (seg % spr) * S;
    const int len = (int)(L - seg_off < S ? L - seg_off : S);
    const int64_t g0 = (int64_t)y * L + seg_off;
    for (int i = t; i < NSYM; i += 256) s_hist[i] = 0;
    int64_t sum_a = 0, sum_b = 0;
    for (int i = t; i < len; i += 256) {
        const uint32_t b = stream_byte(src, filter, y, seg_off + i);
        s_b[i] = (uint8_t)b;
        sum_a += b;
        sum_b += (int64_t)((N - (g0 + i)) % ADLER) * b;      // < 2^24 each, at most 8192 of them
    }
    __syncthreads();
    // run starts: the largest head at or before i
    for (int i = t; i < len; i += 256) s_p[0][i] = (uint16_t)((i == 0 || s_b[i] != s_b[i - 1]) ? i : 0);
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < len; d <<= 1) {
        for (int i = t; i < len; i += 256) {
            const uint16_t a = s_p[cur][i], b = i >= d ? s_p[cur][i - d] : (uint16_t)0;
            s_p[cur ^ 1][i] = a > b ? a : b;
        }
        cur ^= 1;
        __syncthreads();
    }
    for (int i = t; i < len; i += 256) s_start[i] = s_p[cur][i];
    __syncthreads();
    // run ends: the smallest tail at or after i
    for (int i = t; i < len; i += 256) s_p[0][i] = (uint16_t)((i == len - 1 || s_b[i] != s_b[i + 1]) ? i : 0xFFFF);
    __syncthreads();
    cur = 0;
    for (int d = 1; d < len; d <<= 1) {
        for (int i = t; i < len; i += 256) {
            const uint16_t a = s_p[cur][i], b = i + d < len ? s_p[cur][i + d] : (uint16_t)0xFFFF;
            s_p[cur ^ 1][i] = a < b ? a : b;
        }
        cur ^= 1;
        __syncthreads();
    }
    for (int i = t; i < len; i += 256) {
        const int start = s_start[i], p = i - start, r = (int)s_p[cur][i] - start;
        uint16_t token = s_b[i];
        int sym = s_b[i];
        if (p > 0) {
            const int rem = r - 258 * ((p - 1) / 258);
            if (rem >= 3) {
                if ((p - 1) % 258 == 0) {
                    const int m = rem < 258 ? rem : 258;
                    token = (uint16_t)(256 + m);
                    sym = 257 + c_lengths.sym[m];
                } else {
                    token = COVERED;
                    sym = -1;
                }
            }
        }
        tok[g0 + i] = token;
        if (sym >= 0) atomicAdd(&s_hist[sym], 1u);
    }
    __syncthreads();
    for (int i = t; i < NSYM; i += 256)
        if (s_hist[i]) atomicAdd(hist + i, s_hist[i]);
    sum_a = block_sum_i64(sum_a, s_red);
    sum_b = block_sum_i64(sum_b, s_red);
    if (t == 0) {
        part_a[seg] = (uint32_t)(sum_a % ADLER);
        part_b[seg] = (uint32_t)(sum_b % ADLER);
    }
}

// ---- 2. codes ----------------------------------------------------------------------------------------------------------------------
constexpr int CODE_THREADS = 320;
struct Build {
    uint32_t cnt[NSYM], w_leaf[NSYM], w_int[NSYM];
    uint16_t par_leaf[NSYM], par_int[NSYM], code[NSYM];
    int bits[NSYM + 32], next_code[17];
    uint8_t len[NSYM];
};

// the whole workgroup: B.cnt[0, n) -> B.len, B.code (bit-reversed), by mtgs_png.h's rule
__device__ void build_code(Build &B, int n, int limit) {
    const int t = threadIdx.x;
    for (int i = t; i < NSYM + 32; i += CODE_THREADS) B.bits[i] = 0;
    if (t < NSYM) B.len[t] = 0, B.code[t] = 0;
    __syncthreads();
    const uint32_t mine = t < n ? B.cnt[t] : 0;
    const bool used = mine > 0;
    int m = 0, rank = 0, rank2 = 0;
    for (int u = 0; u < n; ++u) {
        const uint32_t c = B.cnt[u];
        if (!c) continue;
        ++m;
        rank += c < mine || (c == mine && u < t);
        rank2 += c > mine || (c == mine && u < t);
    }
    if (used) B.w_leaf[rank] = mine;
    __syncthreads();
    if (t == 0) {
        int li = 0, ii = 0, made = 0;
        for (int k = 0; k + 1 < m; ++k) {
            uint32_t sum = 0;
            for (int e = 0; e < 2; ++e) {
                if (li < m && (ii >= made || B.w_leaf[li] <= B.w_int[ii])) {
                    sum += B.w_leaf[li];
                    B.par_leaf[li++] = (uint16_t)made;
                } else {
                    sum += B.w_int[ii];
                    B.par_int[ii++] = (uint16_t)made;
                }
            }
            B.w_int[made++] = sum;
        }
    }
    __syncthreads();
    if (used) {
        int d = 1;
        if (m > 1)
            for (int node = B.par_leaf[rank]; node != m - 2 && d < NSYM; node = B.par_int[node]) ++d;
        atomicAdd(&B.bits[d], 1);
    }
    __syncthreads();
    if (t == 0) {
        for (int i = m - 1; i > limit; --i)
            while (B.bits[i] > 0) {
                int j = i - 2;
                while (j > 0 && B.bits[j] == 0) --j;
                if (j <= 0) break;                     // cannot happen: n <= 2^limit
                B.bits[i] -= 2, B.bits[i - 1] += 1, B.bits[j + 1] += 2, B.bits[j] -= 1;
            }
        int code = 0;
        for (int l = 1; l <= limit; ++l) {
            code = (code + B.bits[l - 1]) << 1;        // bits[0] is 0
            B.next_code[l] = code;
        }
    }
    __syncthreads();
    int length = 0;
    if (used) {
        int cum = 0;
        for (int l = 1; l <= limit && !length; ++l) {
            cum += B.bits[l];
            if (rank2 < cum) length = l;
        }
        B.len[t] = (uint8_t)length;
    }
    __syncthreads();
    if (used && length) {
        int k = 0;
        for (int u = 0; u < t; ++u) k += B.len[u] == length;
        B.code[t] = (uint16_t)(__brev((uint32_t)(B.next_code[length] + k)) >> (32 - length));
    }
    __syncthreads();
}

__device__ __forceinline__ void put_lds(uint32_t *words, int &at, uint32_t value, int n) {   // thread 0 alone: LSB first
    const uint64_t x = (uint64_t)value << (at & 31);
    words[at >> 5] |= (uint32_t)x;
    if ((uint32_t)(x >> 32)) words[(at >> 5) + 1] |= (uint32_t)(x >> 32);
    at += n;
}

__global__ __launch_bounds__(CODE_THREADS) void png_codes_kernel(const uint32_t *__restrict__ hist, uint32_t *__restrict__ codes,
                                                                uint32_t *__restrict__ hdr, int64_t *__restrict__ info) {
    __shared__ Build B;
    __shared__ uint8_t s_len[NSYM], s_seq[NSYM], s_ext[NSYM];
    __shared__ uint32_t s_hdr[HDR_WORDS];
    __shared__ int s_n;
    const int t = threadIdx.x;
    if (t < NSYM) B.cnt[t] = t < 286 ? hist[t] + (t == 256) : 0;
    for (int i = t; i < HDR_WORDS; i += CODE_THREADS) s_hdr[i] = 0;
    __syncthreads();
    build_code(B, 286, 15);
    if (t < NSYM) {
        s_len[t] = B.len[t];
        codes[t] = ((uint32_t)B.code[t] << 4) | B.len[t];
    }
    __syncthreads();
    if (t < 19) B.cnt[t] = 0;
    __syncthreads();
    int hlit = 257;
    if (t == 0) {
        for (int s = 285; s >= 257; --s)
            if (s_len[s]) {
                hlit = s + 1;
                break;
            }
        const int n_seq = hlit + 1;                     // the distance length behind the lit/len lengths
        auto at = [&](int i) { return i < hlit ? (int)s_len[i] : (hlit > 257 ? 1 : 0); };
        int n = 0;
        auto emit = [&](int sym, int extra) {
            s_seq[n] = (uint8_t)sym, s_ext[n] = (uint8_t)extra, ++n;
            B.cnt[sym] += 1;
        };
        for (int i = 0; i < n_seq;) {
            if (at(i)) {
                emit(at(i), 0);
                ++i;
                continue;
            }
            int z = 0;
            while (i + z < n_seq && at(i + z) == 0) ++z;
            i += z;
            while (z >= 11) {
                const int k = z < 138 ? z : 138;
                emit(18, k - 11);
                z -= k;
            }
            if (z >= 3) emit(17, z - 3), z = 0;
            while (z-- > 0) emit(0, 0);
        }
        s_n = n;
    }
    __syncthreads();
    build_code(B, 19, 7);
    if (t == 0) {
        const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        int hclen = 19;
        while (hclen > 4 && B.len[order[hclen - 1]] == 0) --hclen;
        int at = 0;
        put_lds(s_hdr, at, 0x78, 8);
        put_lds(s_hdr, at, 0x01, 8);
        put_lds(s_hdr, at, 1, 1);
        put_lds(s_hdr, at, 2, 2);
        put_lds(s_hdr, at, (uint32_t)(hlit - 257), 5);
        put_lds(s_hdr, at, 0, 5);
        put_lds(s_hdr, at, (uint32_t)(hclen - 4), 4);
        for (int k = 0; k < hclen; ++k) put_lds(s_hdr, at, B.len[order[k]], 3);
        for (int e = 0; e < s_n; ++e) {
            const int sym = s_seq[e];
            put_lds(s_hdr, at, B.code[sym], B.len[sym]);
            if (sym == 17) put_lds(s_hdr, at, s_ext[e], 3);
            if (sym == 18) put_lds(s_hdr, at, s_ext[e], 7);
        }
        info[0] = at;
    }
    __syncthreads();
    for (int i = t; i < HDR_WORDS; i += CODE_THREADS) hdr[i] = s_hdr[i];
}

// ---- 3. offsets --------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int match_length(uint32_t token) {        // of a token >= 256, kept inside the table whatever it holds
    const int m = (int)token - 256;
    return m < 3 ? 3 : (m > 258 ? 258 : m);
}

__device__ __forceinline__ int token_bits(uint32_t token, const uint32_t *codes) {
    if (token == COVERED) return 0;
    if (token < 256) return (int)(codes[token] & 15);
    const int s = c_lengths.sym[match_length(token)];
    return (int)(codes[257 + s] & 15) + c_lengths.extra[s] + 1;
}

struct BitsValue {
    const uint16_t *tok;
    const uint32_t *codes;
    __device__ int64_t operator()(int64_t i) const { return token_bits(tok[i], codes); }
};

struct OffsetSink {
    uint32_t *bit_off, *seg_bits;
    const int64_t *info;
    int64_t L, spr;
    int S;
    __device__ void operator()(int64_t i, int64_t excl, int64_t) const {
        const uint32_t off = (uint32_t)(info[0] + excl);
        bit_off[i] = off;
        const int64_t j = i % L;
        if (j % S == 0) seg_bits[(i / L) * spr + j / S] = off;
    }
};

// ---- 4. clear, pack, finish --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t payload_bytes_of(const int64_t *info, const int64_t *totals, const uint32_t *codes) {
    return ((info[0] + totals[0] + (int64_t)(codes[256] & 15) + 7) >> 3) + 4;
}

__global__ __launch_bounds__(256) void png_clear_kernel(const int64_t *__restrict__ info, const int64_t *__restrict__ totals,
                                                        const uint32_t *__restrict__ codes, uint32_t *__restrict__ words,
                                                        int64_t max_words) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t used = (payload_bytes_of(info, totals, codes) + 3) >> 2;
    if (i < used && i < max_words) words[i] = 0;
}

__global__ __launch_bounds__(256) void png_pack_kernel(int64_t N, const uint16_t *__restrict__ tok, const uint32_t *__restrict__ bit_off,
                                                       const uint32_t *__restrict__ codes, uint32_t *__restrict__ words,
                                                       int64_t max_words) {
    __shared__ uint32_t s_words[PACK_WORDS];
    __shared__ uint32_t s_end;
    const int t = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * PACK_TILE;
    const int64_t last = (base + PACK_TILE < N ? base + PACK_TILE : N) - 1;
    for (int i = t; i < PACK_WORDS; i += 256) s_words[i] = 0;
    const uint32_t first_bit = bit_off[base];
    if (t == 0) s_end = bit_off[last] + (uint32_t)token_bits(tok[last], codes);
    __syncthreads();
    const uint32_t word0 = first_bit >> 5;
    for (int k = 0; k < PACK_TILE / 256; ++k) {
        const int64_t i = base + k * 256 + t;
        if (i > last) break;
        const uint32_t token = tok[i];
        if (token == COVERED) continue;
        uint32_t value;
        if (token < 256) {
            value = codes[token] >> 4;
        } else {
            const int m = match_length(token);
            const int s = c_lengths.sym[m];
            const uint32_t c = codes[257 + s];
            value = (c >> 4) | ((uint32_t)(m - c_lengths.base[s]) << (c & 15));   // the distance code is the bit 0 behind them
        }
        if (!value) continue;
        const uint32_t off = bit_off[i];
        const uint32_t w = (off >> 5) - word0;         // < PACK_WORDS - 1: offsets grow by at most TOKEN_BITS per position
        if (w + 1 >= (uint32_t)PACK_WORDS) continue;
        const uint64_t x = (uint64_t)value << (off & 31);
        atomicOr(&s_words[w], (uint32_t)x);
        if ((uint32_t)(x >> 32)) atomicOr(&s_words[w + 1], (uint32_t)(x >> 32));
    }
    __syncthreads();
    const uint32_t end_bit = s_end;
    if (end_bit == first_bit) return;
    const int n = (int)(((first_bit & 31) + (end_bit - first_bit) + 31) >> 5);   // <= PACK_WORDS
    for (int i = t; i < n && i < PACK_WORDS; i += 256) {
        const uint32_t w = s_words[i];
        if ((int64_t)word0 + i >= max_words) break;
        if (i == 0 || i == n - 1) {
            if (w) atomicOr(words + word0 + i, w);
        } else {
            words[word0 + i] = w;
        }
    }
}

__device__ __forceinline__ void or_bits(uint32_t *words, int64_t max_words, int64_t at, uint32_t value) {   // value < 2^16
    const uint64_t x = (uint64_t)value << (at & 31);
    const int64_t w = at >> 5;
    if ((uint32_t)x && w < max_words) atomicOr(words + w, (uint32_t)x);
    if ((uint32_t)(x >> 32) && w + 1 < max_words) atomicOr(words + w + 1, (uint32_t)(x >> 32));
}

__global__ __launch_bounds__(256) void png_finish_kernel(int64_t nseg, int64_t N, const uint32_t *__restrict__ part_a,
                                                         const uint32_t *__restrict__ part_b, const uint32_t *__restrict__ hdr,
                                                         const uint32_t *__restrict__ codes, const int64_t *__restrict__ totals,
                                                         int64_t *__restrict__ info, uint32_t *__restrict__ words, int64_t max_words,
                                                         uint32_t *__restrict__ seg_bits) {
    __shared__ int64_t s_red[4];
    const int t = threadIdx.x;
    int64_t a = 0, b = 0;
    for (int64_t s = t; s < nseg; s += 256) a += part_a[s], b += part_b[s];     // < 2^16 each
    a = block_sum_i64(a, s_red);
    b = block_sum_i64(b, s_red);
    const int64_t hdr_bits = info[0];
    const int hdr_words = (int)((hdr_bits + 31) >> 5);
    for (int i = t; i < hdr_words && i < HDR_WORDS; i += 256)
        if (hdr[i] && i < max_words) atomicOr(words + i, hdr[i]);
    if (t == 0) {
        const uint32_t adler = (uint32_t)(((N + b) % ADLER) << 16) | (uint32_t)((1 + a) % ADLER);
        const int64_t eob = hdr_bits + totals[0];
        or_bits(words, max_words, eob, codes[256] >> 4);
        const int64_t at = (eob + (int64_t)(codes[256] & 15) + 7) >> 3;
        for (int k = 0; k < 4; ++k) or_bits(words, max_words, 8 * (at + k), (adler >> (24 - 8 * k)) & 255);
        info[1] = at + 4;
        info[2] = eob;
        seg_bits[nseg] = (uint32_t)eob;
    }
}

// ---- 5. emit -----------------------------------------------------------------------------------------------------------------------
struct Prefix {
    uint8_t b[57];        // the signature, IHDR with its CRC, mtIX's length and name, version, filter, segment_bytes, segment count
};
constexpr int EMIT_BYTES = 16;

__device__ __forceinline__ uint32_t file_byte(int64_t at, const Prefix &prefix, int64_t nseg, const uint32_t *seg_bits,
                                              const uint32_t *words, int64_t payload) {
    if (at < 57) return prefix.b[at];
    at -= 57;
    if (at < 4 * (nseg + 1)) return (seg_bits[at >> 2] >> (8 * (at & 3))) & 255;      // little-endian
    at -= 4 * (nseg + 1);
    if (at < 4) return 0;                                                             // mtIX's CRC: the host's
    at -= 4;
    if (at < 4) return (uint32_t)(payload >> (24 - 8 * at)) & 255;
    at -= 4;
    if (at < 4) return (uint32_t)"IDAT"[at];
    at -= 4;
    if (at < payload) return (words[at >> 2] >> (8 * (at & 3))) & 255;
    at -= payload;
    if (at < 4) return 0;                                                             // IDAT's CRC: the host's
    at -= 4;
    const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
    return iend[at < 12 ? at : 11];
}

__global__ __launch_bounds__(256) void png_emit_kernel(Prefix prefix, int64_t nseg, const uint32_t *__restrict__ seg_bits,
                                                       const uint32_t *__restrict__ words, const int64_t *__restrict__ info,
                                                       uint8_t *__restrict__ data, int64_t capacity, int64_t *__restrict__ meta) {
    const int64_t payload = info[1];
    const int64_t total = 57 + 4 * (nseg + 1) + 4 + 8 + payload + 4 + 12;
    const int64_t first = ((int64_t)blockIdx.x * 256 + threadIdx.x) * EMIT_BYTES;
    if (first == 0) {
        meta[0] = total;
        meta[1] = total > capacity ? 1 : 0;
    }
    for (int k = 0; k < EMIT_BYTES; ++k) {
        const int64_t at = first + k;
        if (at >= total || at >= capacity) return;
        data[at] = (uint8_t)file_byte(at, prefix, nseg, seg_bits, words, payload);
    }
}

// ---- the reader --------------------------------------------------------------------------------------------------------------------
struct Bits {
    const uint8_t *p;
    int64_t n_bytes, next;      // next: the byte the buffer is filled from
    uint64_t buf;
    int count;
    __device__ __forceinline__ void fill() {              // at least 32 valid bits; zeros beyond the payload
        while (count <= 56) {
            const uint64_t b = next < n_bytes ? p[next] : 0;
            buf |= b << count;
            count += 8;
            ++next;
        }
    }
    __device__ __forceinline__ uint32_t take(int n) {
        const uint32_t v = (uint32_t)(buf & ((1ull << n) - 1));
        buf >>= n;
        count -= n;
        return v;
    }
    __device__ __forceinline__ int64_t position() const { return 8 * next - count; }
};

constexpr int INFLATE_LANES = 64;
__global__ __launch_bounds__(INFLATE_LANES) void png_inflate_kernel(const uint8_t *__restrict__ payload, int64_t payload_bytes,
                                                                     const uint32_t *__restrict__ segment_bits,
                                                                     const int32_t *__restrict__ tables, int S, int64_t L, int64_t spr,
                                                                     int64_t nseg, int64_t N, uint8_t *__restrict__ raw,
                                                                     uint32_t *__restrict__ part_a, uint32_t *__restrict__ part_b,
                                                                     int32_t *__restrict__ status) {
    __shared__ uint16_t s_fast[1 << FAST_BITS], s_syms[NSYM], s_count[16];
    __shared__ int s_dist;
    for (int i = threadIdx.x; i < (1 << FAST_BITS); i += INFLATE_LANES) s_fast[i] = (uint16_t)tables[MTGS_PNG_FAST_AT + i];
    for (int i = threadIdx.x; i < NSYM; i += INFLATE_LANES) s_syms[i] = (uint16_t)(tables[MTGS_PNG_SYMS_AT + i] & 511);
    if (threadIdx.x < 16) s_count[threadIdx.x] = (uint16_t)tables[MTGS_PNG_COUNT_AT + threadIdx.x];
    if (threadIdx.x == 0) s_dist = tables[MTGS_PNG_DIST_AT];
    __syncthreads();
    const int64_t seg = (int64_t)blockIdx.x * INFLATE_LANES + threadIdx.x;
    if (seg >= nseg) return;
    const int64_t seg_off = (seg % spr) * S;
    const int len = (int)(L - seg_off < S ? L - seg_off : S);
    const int64_t g0 = (seg / spr) * L + seg_off;
    const int64_t start = segment_bits[seg];
    Bits in{payload, payload_bytes, start >> 3, 0, 0};
    in.fill();
    in.take((int)(start & 7));
    int produced = 0;
    bool bad = false;
    uint32_t prev = 0;
    uint64_t sum_a = 0, sum_b = 0;
    uint32_t weight = (uint32_t)((N - g0) % ADLER);        // of the next byte: (N - i) mod 65521
    while (produced < len) {
        in.fill();
        int sym = -1;
        const uint32_t e = s_fast[in.buf & ((1u << FAST_BITS) - 1)];
        if (e) {
            in.take((int)(e >> 9));
            sym = (int)(e & 511);
        } else {                                          // a code longer than the fast table: canonical, bit by bit
            int code = 0, first = 0, index = 0;
            for (int l = 1; l <= 15; ++l) {
                code |= (int)in.take(1);
                const int count = s_count[l];
                if (code - count < first) {
                    const unsigned at = (unsigned)(index + (code - first));
                    sym = s_syms[at < (unsigned)NSYM ? at : 0];
                    break;
                }
                index += count, first += count;
                first <<= 1, code <<= 1;
            }
        }
        int n = 1;
        if (sym < 0 || sym == 256 || sym > 285) {
            bad = true;
            break;
        }
        if (sym > 256) {
            const int s = sym - 257;
            n = c_lengths.base[s] + (int)in.take(c_lengths.extra[s]);
            if (produced == 0 || !s_dist || in.take(1) != 0 || n > len - produced) {
                bad = true;
                break;
            }
        } else {
            prev = (uint32_t)sym;
        }
        for (int k = 0; k < n; ++k) {                      // produced + n <= len
            raw[g0 + produced + k] = (uint8_t)prev;
            sum_a += prev;
            sum_b += (uint64_t)weight * prev;
            weight = weight ? weight - 1 : ADLER - 1;
        }
        produced += n;
    }
    for (int k = produced; k < len; ++k) raw[g0 + k] = 0;   // a segment that failed: its own bytes, defined
    if (!bad && in.position() != (int64_t)segment_bits[seg + 1]) bad = true;
    part_a[seg] = (uint32_t)(sum_a % ADLER);
    part_b[seg] = (uint32_t)(sum_b % ADLER);
    if (bad) atomicOr(status, MTGS_PNG_ERR_SEGMENT);
    else atomicAdd(status + 1, 1);
}

struct Sink {
    void *out;
    int as_depth, C, order;
    int64_t sy, sx, sc;
};

__device__ __forceinline__ void store_pixel(const Sink &k, int y, int x, const uint32_t *v) {   // v: the FILE's channels
    if (k.as_depth) {
        const float d = __fadd_rn((float)v[2], __fmul_rn((float)v[1], 256.0f));
        ((float *)k.out)[y * k.sy + x * k.sx] = __fmul_rn(d, 0.01f);
        return;
    }
    for (int c = 0; c < k.C; ++c) ((uint8_t *)k.out)[y * k.sy + x * k.sx + (k.order ? k.C - 1 - c : c) * k.sc] = (uint8_t)v[c];
}

// None and Sub: a workgroup per row, 256 pixels at a time, a block prefix sum per channel with a carry
__global__ __launch_bounds__(256) void png_unfilter_rows_kernel(const uint8_t *__restrict__ raw, int64_t L, int w, int sub, Sink sink) {
    __shared__ uint32_t s_wave[3][4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int y = blockIdx.x;
    const uint8_t *row = raw + (int64_t)y * L + 1;
    uint32_t carry[3] = {0, 0, 0};
    for (int x0 = 0; x0 < w; x0 += 256) {
        const int x = x0 + t;
        uint32_t v[3] = {0, 0, 0};
        if (x < w)
            for (int c = 0; c < sink.C; ++c) v[c] = row[(int64_t)x * sink.C + c];
        if (sub) {
            for (int c = 0; c < sink.C; ++c) {
                uint32_t inc = v[c];
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const uint32_t up = __shfl_up(inc, o, 64);
                    if (lane >= o) inc += up;
                }
                if (lane == 63) s_wave[c][wave] = inc;
                v[c] = inc;
            }
            __syncthreads();
            for (int c = 0; c < sink.C; ++c) {
                uint32_t before = carry[c], all = 0;
                for (int k = 0; k < 4; ++k) {
                    if (k < wave) before += s_wave[c][k];
                    all += s_wave[c][k];
                }
                v[c] = (v[c] + before) & 255;
                carry[c] = (carry[c] + all) & 255;
            }
            __syncthreads();
        }
        if (x < w) store_pixel(sink, y, x, v);
    }
}

// Up: a thread per pixel column walks down the rows, eight rows of loads in flight
__global__ __launch_bounds__(64) void png_unfilter_up_kernel(const uint8_t *__restrict__ raw, int64_t L, int h, int w, Sink sink) {
    const int x = blockIdx.x * 64 + threadIdx.x;
    if (x >= w) return;
    uint32_t acc[3] = {0, 0, 0};
    for (int y0 = 0; y0 < h; y0 += 8) {
        uint32_t v[8][3];
#pragma unroll
        for (int k = 0; k < 8; ++k)
            for (int c = 0; c < 3; ++c) v[k][c] = (y0 + k < h && c < sink.C) ? raw[(int64_t)(y0 + k) * L + 1 + (int64_t)x * sink.C + c] : 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (y0 + k >= h) break;
            for (int c = 0; c < 3; ++c) acc[c] = (acc[c] + v[k][c]) & 255;
            store_pixel(sink, y0 + k, x, acc);
        }
    }
}

__global__ __launch_bounds__(256) void png_status_kernel(int64_t nseg, int64_t N, const uint32_t *__restrict__ part_a,
                                                         const uint32_t *__restrict__ part_b, const uint8_t *__restrict__ payload,
                                                         int64_t payload_bytes, int32_t *__restrict__ status) {
    __shared__ int64_t s_red[4];
    int64_t a = 0, b = 0;
    for (int64_t s = threadIdx.x; s < nseg; s += 256) a += part_a[s], b += part_b[s];
    a = block_sum_i64(a, s_red);
    b = block_sum_i64(b, s_red);
    if (threadIdx.x == 0) {
        const uint32_t adler = (uint32_t)(((N + b) % ADLER) << 16) | (uint32_t)((1 + a) % ADLER);
        const uint8_t *p = payload + payload_bytes - 4;
        const uint32_t stored = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
        status[2] = (int32_t)nseg;
        status[3] = adler == stored ? 1 : 0;
        if (adler != stored) atomicOr(status, MTGS_PNG_ERR_ADLER);
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
int check_shape(const char *fn, int h, int w, int channels, int segment_bytes) {
    MTGS_REQUIRE(channels == 1 || channels == 3, MTGS_EUNSUPPORTED, "%s: %d channels are not implemented (1, gray, or 3, RGB)", fn, channels);
    MTGS_REQUIRE(h >= 1 && h <= 65535 && w >= 1 && w <= 65535, MTGS_EINVAL, "%s: h and w outside [1, 65535] (%d, %d)", fn, h, w);
    MTGS_REQUIRE(segment_bytes >= MTGS_PNG_MIN_SEGMENT_BYTES && segment_bytes <= MTGS_PNG_MAX_SEGMENT_BYTES, MTGS_EINVAL,
                 "%s: segment_bytes outside [%d, %d] (%d)", fn, MTGS_PNG_MIN_SEGMENT_BYTES, MTGS_PNG_MAX_SEGMENT_BYTES, segment_bytes);
    const Geometry g = geometry(h, w, channels, segment_bytes);
    MTGS_REQUIRE(8 * g.max_payload < ((int64_t)1 << 32), MTGS_EINVAL, "%s: %d x %d x %d is too large: its stream could exceed 2^32 bits", fn,
                 h, w, channels);
    MTGS_REQUIRE(g.nseg < ((int64_t)1 << 31), MTGS_EINVAL, "%s: too many segments (%lld)", fn, (long long)g.nseg);
    return MTGS_OK;
}

int check_filter_order(const char *fn, int filter, int order) {
    MTGS_REQUIRE(filter == MTGS_PNG_FILTER_NONE || filter == MTGS_PNG_FILTER_SUB || filter == MTGS_PNG_FILTER_UP, MTGS_EUNSUPPORTED,
                 "%s: filter %d is not implemented (0 None, 1 Sub, 2 Up; Average and Paeth serialise a row)", fn, filter);
    MTGS_REQUIRE(order == MTGS_PNG_ORDER_RGB || order == MTGS_PNG_ORDER_BGR, MTGS_EINVAL, "%s: order must be MTGS_PNG_ORDER_RGB or _BGR (%d)",
                 fn, order);
    return MTGS_OK;
}

uint32_t crc32_of(const uint8_t *p, int n) {
    uint32_t c = 0xFFFFFFFFu;
    for (int i = 0; i < n; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1)));
    }
    return ~c;
}

void put_be32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)(v >> 24), p[1] = (uint8_t)(v >> 16), p[2] = (uint8_t)(v >> 8), p[3] = (uint8_t)v; }
void put_le32(uint8_t *p, uint32_t v) { p[3] = (uint8_t)(v >> 24), p[2] = (uint8_t)(v >> 16), p[1] = (uint8_t)(v >> 8), p[0] = (uint8_t)v; }

struct DecodeWorkspace {
    int32_t *status;
    uint32_t *part_a, *part_b;
    uint8_t *raw;
    size_t bytes;
};

DecodeWorkspace carve_decode(const Geometry &g, void *base) {
    DecodeWorkspace k;
    size_t at = 0;
    auto take = [&](size_t n) {
        char *p = (char *)base + at;
        at += (n + 15) & ~(size_t)15;
        return p;
    };
    k.status = (int32_t *)take(MTGS_PNG_STATUS_WORDS * 4);
    k.part_a = (uint32_t *)take((size_t)g.nseg * 4);
    k.part_b = (uint32_t *)take((size_t)g.nseg * 4);
    k.raw = (uint8_t *)take((size_t)g.N);
    k.bytes = at;
    return k;
}

}  // namespace

extern "C" int mtgs_png_sizes(int h, int w, int channels, int segment_bytes, size_t *ws_bytes, size_t *capacity) {
    const char *fn = "mtgs_png_sizes";
    if (int rc = check_shape(fn, h, w, channels, segment_bytes)) return rc;
    const Geometry g = geometry(h, w, channels, segment_bytes);
    if (ws_bytes) *ws_bytes = carve(g, nullptr).bytes;
    if (capacity) *capacity = (size_t)(g.prefix + 4 * (g.nseg + 1) + 4 + 8 + g.max_payload + 4 + 12);
    return MTGS_OK;
}

extern "C" int mtgs_png_encode(const void *image, int is_depth, int h, int w, int channels, int64_t stride_y, int64_t stride_x,
                               int64_t stride_c, int order, int filter, int segment_bytes, int roi_x, int roi_y, int roi_w, int roi_h,
                               float max_range, float min_depth, uint8_t *data, size_t capacity, int64_t *meta, void *ws,
                               size_t ws_bytes, void *stream) {
    const char *fn = "mtgs_png_encode";
    if (int rc = check_shape(fn, h, w, channels, segment_bytes)) return rc;
    if (int rc = check_filter_order(fn, filter, order)) return rc;
    MTGS_REQUIRE(image != nullptr, MTGS_EINVAL, "%s: null pointer: image", fn);
    if (is_depth) {
        MTGS_REQUIRE(channels == 3, MTGS_EINVAL, "%s: a depth file has 3 channels (%d)", fn, channels);
        MTGS_REQUIRE(((uintptr_t)image & 3) == 0, MTGS_EINVAL, "%s: a float32 depth must be 4-byte aligned", fn);
        MTGS_REQUIRE(roi_w >= 1 && roi_h >= 1 && roi_x >= 0 && roi_y >= 0 && (int64_t)roi_x + roi_w <= w && (int64_t)roi_y + roi_h <= h,
                     MTGS_EINVAL, "%s: roi (%d, %d, %d, %d) is empty or leaves the %d x %d image", fn, roi_x, roi_y, roi_w, roi_h, w, h);
        MTGS_REQUIRE(max_range * 100.0f < 65536.0f, MTGS_EUNSUPPORTED,
                     "%s: max_range %g is not implemented: max_range * 100 must stay below 65536 (two bytes of centimetres)", fn, (double)max_range);
        MTGS_REQUIRE(min_depth >= 0.0f, MTGS_EINVAL, "%s: min_depth must not be negative (%g)", fn, (double)min_depth);
    }
    MTGS_REQUIRE(data != nullptr || capacity == 0, MTGS_EINVAL, "%s: null pointer: data", fn);
    MTGS_REQUIRE(capacity < ((size_t)1 << 62), MTGS_EINVAL, "%s: capacity %zu is no size", fn, capacity);
    MTGS_REQUIRE(meta != nullptr && ((uintptr_t)meta & 7) == 0, MTGS_EINVAL, "%s: meta must be a non-null, 8-byte aligned int64[2]", fn);
    MTGS_REQUIRE(ws != nullptr, MTGS_EINVAL, "%s: null pointer: ws", fn);
    MTGS_REQUIRE(((uintptr_t)ws & 15) == 0, MTGS_EINVAL, "%s: workspace must be 16-byte aligned", fn);
    const Geometry g = geometry(h, w, channels, segment_bytes);
    const Workspace k = carve(g, ws);
    MTGS_REQUIRE(ws_bytes >= k.bytes, MTGS_EWORKSPACE, "%s: workspace %zu < %zu bytes", fn, ws_bytes, k.bytes);
    hipStream_t st = (hipStream_t)stream;
    Prefix prefix;
    const uint8_t signature[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    for (int i = 0; i < 8; ++i) prefix.b[i] = signature[i];
    uint8_t *p = prefix.b + 8;
    put_be32(p, 13);
    p[4] = 'I', p[5] = 'H', p[6] = 'D', p[7] = 'R';
    put_be32(p + 8, (uint32_t)w);
    put_be32(p + 12, (uint32_t)h);
    p[16] = 8, p[17] = (uint8_t)(channels == 3 ? 2 : 0), p[18] = 0, p[19] = 0, p[20] = 0;
    put_be32(p + 21, crc32_of(p + 4, 17));
    p += 25;
    put_be32(p, (uint32_t)(4 * (5 + g.nseg)));
    p[4] = 'm', p[5] = 't', p[6] = 'I', p[7] = 'X';
    put_le32(p + 8, MTGS_PNG_INDEX_VERSION);
    put_le32(p + 12, (uint32_t)filter);
    put_le32(p + 16, (uint32_t)segment_bytes);
    put_le32(p + 20, (uint32_t)g.nseg);
    const Source src{image, is_depth, channels, order, stride_y, stride_x, stride_c, roi_x, roi_y, roi_w, roi_h, max_range, min_depth};
    if (int rc = mtgs_zero_async(k.hist, NSYM * 4, st)) return rc;
    png_tokens_kernel<<<(unsigned)g.nseg, 256, 0, st>>>(src, filter, segment_bytes, g.L, g.spr, g.N, k.tok, k.hist, k.part_a, k.part_b);
    png_codes_kernel<<<1, CODE_THREADS, 0, st>>>(k.hist, k.codes, k.hdr, k.info);
    mtgs_scan::run(g.N, BitsValue{k.tok, k.codes}, OffsetSink{k.bit_off, k.seg_bits, k.info, g.L, g.spr, segment_bytes}, k.spine, k.totals, st);
    png_clear_kernel<<<(unsigned)ceil_div64(g.max_words, 256), 256, 0, st>>>(k.info, k.totals, k.codes, k.words, g.max_words);
    png_pack_kernel<<<(unsigned)ceil_div64(g.N, PACK_TILE), 256, 0, st>>>(g.N, k.tok, k.bit_off, k.codes, k.words, g.max_words);
    png_finish_kernel<<<1, 256, 0, st>>>(g.nseg, g.N, k.part_a, k.part_b, k.hdr, k.codes, k.totals, k.info, k.words, g.max_words, k.seg_bits);
    const int64_t max_file = g.prefix + 4 * (g.nseg + 1) + 4 + 8 + g.max_payload + 4 + 12;
    png_emit_kernel<<<(unsigned)ceil_div64(max_file, 256 * EMIT_BYTES), 256, 0, st>>>(prefix, g.nseg, k.seg_bits, k.words, k.info, data,
                                                                                     (int64_t)capacity, meta);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}

extern "C" int mtgs_png_decode_sizes(int h, int w, int channels, int segment_bytes, size_t *ws_bytes) {
    const char *fn = "mtgs_png_decode_sizes";
    if (int rc = check_shape(fn, h, w, channels, segment_bytes)) return rc;
    if (ws_bytes) *ws_bytes = carve_decode(geometry(h, w, channels, segment_bytes), nullptr).bytes;
    return MTGS_OK;
}

extern "C" int mtgs_png_decode(const uint8_t *payload, int64_t payload_bytes, const uint32_t *segment_bits, const int32_t *tables, int h,
                               int w, int channels, int filter, int segment_bytes, void *out, int as_depth, int64_t stride_y,
                               int64_t stride_x, int64_t stride_c, int order, int32_t *status, void *ws, size_t ws_bytes, void *stream) {
    const char *fn = "mtgs_png_decode";
    if (int rc = check_shape(fn, h, w, channels, segment_bytes)) return rc;
    if (int rc = check_filter_order(fn, filter, order)) return rc;
    const Geometry g = geometry(h, w, channels, segment_bytes);
    MTGS_REQUIRE(payload != nullptr, MTGS_EINVAL, "%s: null pointer: payload", fn);
    MTGS_REQUIRE(payload_bytes >= 8 && payload_bytes <= g.max_payload, MTGS_EINVAL,
                 "%s: payload_bytes %lld outside [8, %lld], the most this shape can take", fn, (long long)payload_bytes, (long long)g.max_payload);
    MTGS_REQUIRE(segment_bits != nullptr && ((uintptr_t)segment_bits & 3) == 0, MTGS_EINVAL, "%s: segment_bits must be a non-null, aligned uint32 array", fn);
    MTGS_REQUIRE(tables != nullptr && ((uintptr_t)tables & 3) == 0, MTGS_EINVAL, "%s: tables must be a non-null, aligned int32 array", fn);
    MTGS_REQUIRE(out != nullptr, MTGS_EINVAL, "%s: null pointer: out", fn);
    MTGS_REQUIRE(stride_y >= 0 && stride_x >= 0 && stride_c >= 0, MTGS_EINVAL, "%s: negative stride (%lld, %lld, %lld)", fn,
                 (long long)stride_y, (long long)stride_x, (long long)stride_c);
    if (as_depth) {
        MTGS_REQUIRE(channels == 3, MTGS_EINVAL, "%s: a depth file has 3 channels (%d)", fn, channels);
        MTGS_REQUIRE(((uintptr_t)out & 3) == 0, MTGS_EINVAL, "%s: a float32 out must be 4-byte aligned", fn);
    }
    MTGS_REQUIRE(ws != nullptr, MTGS_EINVAL, "%s: null pointer: ws", fn);
    MTGS_REQUIRE(((uintptr_t)ws & 15) == 0, MTGS_EINVAL, "%s: workspace must be 16-byte aligned", fn);
    const DecodeWorkspace k = carve_decode(g, ws);
    MTGS_REQUIRE(ws_bytes >= k.bytes, MTGS_EWORKSPACE, "%s: workspace %zu < %zu bytes", fn, ws_bytes, k.bytes);
    MTGS_REQUIRE(status == nullptr || ((uintptr_t)status & 3) == 0, MTGS_EINVAL, "%s: status must be 4-byte aligned", fn);
    int32_t *state = status ? status : k.status;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = mtgs_zero_async(state, MTGS_PNG_STATUS_WORDS * 4, st)) return rc;
    png_inflate_kernel<<<(unsigned)ceil_div64(g.nseg, INFLATE_LANES), INFLATE_LANES, 0, st>>>(payload, payload_bytes, segment_bits, tables,
                                                                                             segment_bytes, g.L, g.spr, g.nseg, g.N, k.raw,
                                                                                             k.part_a, k.part_b, state);
    const Sink sink{out, as_depth, channels, order, stride_y, stride_x, stride_c};
    if (filter == MTGS_PNG_FILTER_UP)
        png_unfilter_up_kernel<<<(unsigned)ceil_div64(w, 64), 64, 0, st>>>(k.raw, g.L, h, w, sink);
    else
        png_unfilter_rows_kernel<<<(unsigned)h, 256, 0, st>>>(k.raw, g.L, w, filter == MTGS_PNG_FILTER_SUB, sink);
    png_status_kernel<<<1, 256, 0, st>>>(g.nseg, g.N, k.part_a, k.part_b, payload, payload_bytes, state);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}
