// jpegdec.hip -- baseline JPEG frames decoded on the device (include/mtgs_jpegdec.h states the arithmetic and the argument why no
// speculative decode can leave bounds; gfx950).  Integer arithmetic throughout; the one float conversion is __fdiv_rn.
//
//   mtgs_zero_async      the control words (status, flags, interval starts, totals) and the coefficient buffer
//   mtgs_scan::run       value(i) = (byte i of the scan is kept) + (it closes a restart marker) << 32; the sink compacts the kept bytes
//                        into the clean stream, records the clean offset behind marker r as the start of interval r + 1 and pads the
//                        stream's tail with 0xFF
//   mtgs_scan::run       value(k) = the subsequences of interval k; the sink keeps each interval's first subsequence
//   setup_kernel         a thread per subsequence: its interval (a bounded binary search), its first and last bit, the guess
//   sync_kernel x L      the fixed point of the header: a workgroup per MTGS_JPEGDEC_RUN subsequences, a lane per subsequence;
//                        inside a launch the lanes pass exits to their successors through LDS until nothing changes; between
//                        launches the last lane's exit reaches the next workgroup through a double-buffered array of heads, so a
//                        launch reads only what the launch before it wrote.  L = the workgroups of the stream.
//   mtgs_scan::run       value(s) = the blocks subsequence s completed in its last decode (from its final, exact entry)
//   write_kernel         a lane per subsequence decodes it again and writes the coefficients
//   mtgs_scan::run x 2   the DC differences of Y, and of Cb and Cr packed as two signed 32-bit halves
//   idct_kernel          8 lanes per block: columns, LDS, rows; planes at component resolution (padded to whole MCUs)
//   colour_kernel        a lane per pixel: fancy upsampling, the colour transform, the store in any strides
//   status_kernel        the error word and the counts
#include "common.hpp"
#include "jpeg_zigzag.hpp"
#include "scan.hpp"

namespace {

typedef unsigned long long u64;
constexpr int RUN = MTGS_JPEGDEC_RUN;
constexpr int QUANT_AT = MTGS_JPEGDEC_QUANT_AT, FAST_AT = MTGS_JPEGDEC_FAST_AT, MAXCODE_AT = MTGS_JPEGDEC_MAXCODE_AT,
              VALOFF_AT = MTGS_JPEGDEC_VALOFF_AT, HUFFVAL_AT = MTGS_JPEGDEC_HUFFVAL_AT, SLOT_AT = MTGS_JPEGDEC_SLOT_AT;
constexpr int FAST_BITS = MTGS_JPEGDEC_FAST_BITS;
static_assert((1 << FAST_BITS) == (MAXCODE_AT - FAST_AT) / 4, "the fast tables are indexed by FAST_BITS bits");
constexpr u64 NONE = ~0ull;
constexpr int64_t LOW32 = 0xffffffffll;

__constant__ uint8_t c_natural[64] = {MTGS_JPEG_ZIGZAG};

// ---- geometry and workspace ------------------------------------------------------------------------------------------------------
struct Dec {
    // host-known
    int H, W, hs, vs, nb, mcus_x, ri, n_int, bits, n_sub_max, n_wg;
    int64_t n_blocks, scan_bytes, cap_bytes;
    int plane_w[3], plane_h[3];
    // device
    const uint8_t *scan;
    const int32_t *tab;
    int32_t *status;         // [4]                      } zeroed
    int32_t *flags;          // [n_wg + 1]               }
    int32_t *istart;         // [n_int + 1]              }
    int64_t *totals;         // [0] kept bytes | markers << 32, [1] subsequences, [2] blocks, [3] DC   }
    int16_t *coef;           // [n_blocks][64] natural   }
    uint8_t *clean;          // [cap_bytes]
    int32_t *sub_offset;     // [n_int + 1]
    int4 *sub_info;          // [n_sub_max] first bit, last bit, interval, 1 if it starts the interval
    u64 *entry;              // [n_sub_max]
    u64 *head;               // [2][n_wg + 1]
    int32_t *count;          // [n_sub_max + 1]
    int32_t *before;         // [n_sub_max + 1]
    int32_t *dcsum;          // [n_blocks]
    int64_t *spine;
    uint8_t *plane[3];
    size_t zero_bytes, bytes;
};

size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

Dec geometry(int h, int w, int subsampling, int restart_interval, int64_t scan_bytes, int bits, void *base) {
    Dec d{};
    d.H = h, d.W = w;
    d.hs = subsampling == MTGS_JPEGDEC_444 ? 1 : 2;
    d.vs = subsampling == MTGS_JPEGDEC_420 ? 2 : 1;
    d.nb = d.hs * d.vs + 2;
    d.mcus_x = (w + 8 * d.hs - 1) / (8 * d.hs);
    const int mcus_y = (h + 8 * d.vs - 1) / (8 * d.vs);
    const int n_mcu = d.mcus_x * mcus_y;
    d.ri = restart_interval > 0 && restart_interval < n_mcu ? restart_interval : n_mcu;
    d.n_int = (n_mcu + d.ri - 1) / d.ri;
    d.bits = bits;
    d.n_blocks = (int64_t)n_mcu * d.nb;
    d.scan_bytes = scan_bytes;
    d.cap_bytes = (scan_bytes + 3) / 4 * 4 + 8;          // whole words, and two more that every read may touch
    d.n_sub_max = (int)(ceil_div64(8 * scan_bytes, bits) + d.n_int);
    d.n_wg = (d.n_sub_max + RUN - 1) / RUN;
    for (int c = 0; c < 3; ++c) {
        d.plane_w[c] = d.mcus_x * 8 * (c == 0 ? d.hs : 1);
        d.plane_h[c] = mcus_y * 8 * (c == 0 ? d.vs : 1);
    }
    size_t at = 0;
    auto take = [&](size_t n) {
        char *p = (char *)base + at;
        at += align16(n);
        return p;
    };
    d.status = (int32_t *)take(MTGS_JPEGDEC_STATUS_WORDS * sizeof(int32_t));
    d.flags = (int32_t *)take((size_t)(d.n_wg + 1) * sizeof(int32_t));
    d.istart = (int32_t *)take((size_t)(d.n_int + 1) * sizeof(int32_t));
    d.totals = (int64_t *)take(4 * sizeof(int64_t));
    d.coef = (int16_t *)take((size_t)d.n_blocks * 64 * sizeof(int16_t));
    d.zero_bytes = at;
    d.clean = (uint8_t *)take((size_t)d.cap_bytes);
    d.sub_offset = (int32_t *)take((size_t)(d.n_int + 1) * sizeof(int32_t));
    d.sub_info = (int4 *)take((size_t)d.n_sub_max * sizeof(int4));
    d.entry = (u64 *)take((size_t)d.n_sub_max * sizeof(u64));
    d.head = (u64 *)take((size_t)2 * (d.n_wg + 1) * sizeof(u64));
    d.count = (int32_t *)take((size_t)(d.n_sub_max + 1) * sizeof(int32_t));
    d.before = (int32_t *)take((size_t)(d.n_sub_max + 1) * sizeof(int32_t));
    d.dcsum = (int32_t *)take((size_t)d.n_blocks * sizeof(int32_t));
    int64_t longest = d.cap_bytes;
    if (d.n_blocks > longest) longest = d.n_blocks;
    if (d.n_sub_max + 1 > longest) longest = d.n_sub_max + 1;
    if (d.n_int > longest) longest = d.n_int;
    d.spine = (int64_t *)take(mtgs_scan::workspace_bytes(longest));
    for (int c = 0; c < 3; ++c) d.plane[c] = (uint8_t *)take((size_t)d.plane_w[c] * d.plane_h[c]);
    d.bytes = at;
    return d;
}

// ---- device pieces ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int clean_bytes(const Dec &d) {
    const int64_t n = d.totals[0] & LOW32;
    return (int)(n > d.scan_bytes ? d.scan_bytes : n);
}

// the clean byte at which interval k starts; k = n_int: the end of the stream.  A start that no marker recorded is the end.
__device__ __forceinline__ int interval_start(const Dec &d, int k, int n_clean) {
    if (k <= 0) return 0;
    if (k >= d.n_int) return n_clean;
    const int v = d.istart[k];
    return v <= 0 || v > n_clean ? n_clean : v;
}

__device__ __forceinline__ int blocks_of_interval(const Dec &d, int k) {
    const int64_t first = (int64_t)k * d.ri * d.nb, all = (int64_t)d.ri * d.nb;
    const int64_t left = d.n_blocks - first;
    return (int)(left < 0 ? 0 : (left < all ? left : all));
}

__device__ __forceinline__ int component_of(const Dec &d, int blk) { return blk < d.nb - 2 ? 0 : blk - (d.nb - 2) + 1; }

// the next 32 bits at bit p of the clean stream, MSB first; the word index is clamped, and the stream holds two words beyond it.
// The two words stay in registers until p leaves the first of them.
struct Window {
    uint32_t at = ~0u;
    u64 x = 0;
};

__device__ __forceinline__ uint32_t peek(const Dec &d, Window &win, int p) {
    const uint32_t last = (uint32_t)(d.cap_bytes / 4 - 2);
    uint32_t w = (uint32_t)p >> 5;
    w = w > last ? last : w;
    if (w != win.at) {
        const uint32_t *words = (const uint32_t *)d.clean;
        win.x = ((u64)__builtin_bswap32(words[w]) << 32) | __builtin_bswap32(words[w + 1]);
        win.at = w;
    }
    return (uint32_t)(win.x >> (32 - (p & 31)));
}

// the tables in LDS: every lane of a workgroup walks them symbol by symbol
__device__ __forceinline__ void stage_tables(const Dec &d, int32_t *s_tab) {
    for (int k = threadIdx.x; k < MTGS_JPEGDEC_TABLE_WORDS; k += blockDim.x) s_tab[k] = d.tab[k];
    __syncthreads();
}

// the code at the head of `window`: its length (0: no code starts here) and its symbol
__device__ __forceinline__ int lookup(const int32_t *tab, int slot, uint32_t window, int &symbol) {
    slot &= 3;
    const int fast = tab[FAST_AT + (slot << FAST_BITS) + (int)(window >> (32 - FAST_BITS))];
    if (fast) {
        symbol = fast & 255;
        return (fast >> 8) & 31;
    }
#pragma unroll
    for (int l = FAST_BITS + 1; l <= 16; ++l) {
        const int code = (int)(window >> (32 - l));
        if (code <= tab[MAXCODE_AT + slot * 18 + l]) {
            symbol = tab[HUFFVAL_AT + slot * 256 + ((code + tab[VALOFF_AT + slot * 18 + l]) & 255)] & 255;
            return l;
        }
    }
    symbol = 0;
    return 0;
}

__device__ __forceinline__ int extend(uint32_t window, int len, int cat) {
    if (cat == 0) return 0;
    const int v = (int)((window << len) >> (32 - cat));        // len <= 16, 1 <= cat <= 15
    return v < (1 << (cat - 1)) ? v - (1 << cat) + 1 : v;
}

__device__ __forceinline__ u64 pack_state(int p, int blk, int zz) { return ((u64)(uint32_t)p << 16) | (u64)(blk << 6) | (u64)zz; }

// Decodes from `state` until the position reaches `end`; returns the state there and adds the blocks completed to `done`.
// WRITE: coefficients go to block first_block + (blocks completed so far) while that count is below `limit`.
template <bool WRITE>
__device__ __forceinline__ u64 decode(const Dec &d, const int32_t *tab, u64 state, int end, int &done, int64_t first_block, int limit) {
    Window win;
    int slots = 0;                                             // each component's DC and AC slot, two bits each
#pragma unroll
    for (int k = 0; k < 6; ++k) slots |= (tab[SLOT_AT + k] & 3) << (2 * k);
    int p = (int)(uint32_t)(state >> 16);
    int blk = (int)(state >> 6) & 7, zz = (int)state & 63;
    blk = blk < d.nb ? blk : 0;
    for (int step = 0; step < d.bits && p < end; ++step) {     // every step consumes a bit or more: at most `bits` steps to the end
        const uint32_t window = peek(d, win, p);
        const int comp = component_of(d, blk);
        int symbol;
        if (zz == 0) {
            const int len = lookup(tab, slots >> (4 * comp), window, symbol);
            if (len == 0) {
                p += 1;
                continue;
            }
            const int cat = symbol & 15;
            if (WRITE && done < limit) d.coef[(first_block + done) * 64] = (int16_t)extend(window, len, cat);
            p += len + cat;
            zz = 1;
        } else {
            const int len = lookup(tab, slots >> (4 * comp + 2), window, symbol);
            if (len == 0) {
                p += 1;
                continue;
            }
            const int run = symbol >> 4, cat = symbol & 15;
            p += len + cat;
            if (cat) {
                const int k = zz + run;
                if (WRITE && k <= 63 && done < limit) d.coef[(first_block + done) * 64 + c_natural[k]] = (int16_t)extend(window, len, cat);
                zz = k + 1;
            } else {
                zz = run == 15 ? zz + 16 : 64;                  // ZRL | EOB
            }
        }
        if (zz > 63) {
            zz = 0;
            blk = blk + 1 < d.nb ? blk + 1 : 0;
            ++done;
        }
    }
    return pack_state(p, blk, zz);
}

// ---- 1. the clean stream -----------------------------------------------------------------------------------------------------------
struct CleanValue {
    const uint8_t *scan;
    int64_t n;
    __device__ int64_t operator()(int64_t i) const {
        if (i >= n) return 0;
        const int b = scan[i], prev = i > 0 ? scan[i - 1] : 0, next = i + 1 < n ? scan[i + 1] : 0;
        const bool closes = prev == 0xFF && (b & 0xF8) == 0xD0;              // the D0..D7 of a restart marker
        const bool opens = b == 0xFF && (next & 0xF8) == 0xD0;               // its FF
        const bool stuffed = prev == 0xFF && b == 0x00;
        return (int64_t)(!(closes || opens || stuffed)) + ((int64_t)closes << 32);
    }
};

struct CleanSink {
    Dec d;
    __device__ void operator()(int64_t i, int64_t excl, int64_t incl) const {
        const int64_t kept = excl & LOW32;                                   // <= i < cap_bytes
        if (i < d.scan_bytes) {
            if ((incl & LOW32) != kept) d.clean[kept] = d.scan[i];
            if ((incl >> 32) != (excl >> 32)) {
                const int64_t k = (excl >> 32) + 1;                          // the marker closes interval k - 1
                if (k < d.n_int) d.istart[k] = (int32_t)kept;
            }
        }
        const int64_t pad = (d.totals[0] & LOW32) + i;                       // the spine wrote the total before this launch
        if (pad < d.cap_bytes) d.clean[pad] = 0xFF;
    }
};

// ---- 2. subsequences ---------------------------------------------------------------------------------------------------------------
struct CutValue {
    Dec d;
    __device__ int64_t operator()(int64_t k) const {
        const int n_clean = clean_bytes(d);
        const int64_t bits = 8 * (int64_t)(interval_start(d, (int)k + 1, n_clean) - interval_start(d, (int)k, n_clean));
        const int64_t n = bits <= 0 ? 1 : (bits + d.bits - 1) / d.bits;
        return n;
    }
};

struct CutSink {
    Dec d;
    __device__ void operator()(int64_t k, int64_t excl, int64_t) const {
        d.sub_offset[k] = (int32_t)(excl < d.n_sub_max ? excl : d.n_sub_max);
    }
};

__device__ __forceinline__ int n_subsequences(const Dec &d) {
    const int64_t n = d.totals[1];
    return (int)(n < 0 ? 0 : (n > d.n_sub_max ? d.n_sub_max : n));
}

__global__ __launch_bounds__(256) void jpegdec_setup_kernel(Dec d) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    const int n_sub = n_subsequences(d);
    if (s == 0) d.sub_offset[d.n_int] = n_sub;
    if (s >= d.n_sub_max) return;
    int4 info = make_int4(0, 0, 0, 1);
    if (s < n_sub) {
        int lo = 0, hi = d.n_int - 1;                          // the last interval whose first subsequence is <= s
        for (int it = 0; it < 32 && lo < hi; ++it) {
            const int mid = (lo + hi + 1) >> 1;
            if (d.sub_offset[mid] <= s) lo = mid;
            else hi = mid - 1;
        }
        const int n_clean = clean_bytes(d);
        const int off = d.sub_offset[lo];
        const int64_t stop = 8 * (int64_t)interval_start(d, lo + 1, n_clean);
        int64_t begin = 8 * (int64_t)interval_start(d, lo, n_clean) + (int64_t)(s - off) * d.bits;
        begin = begin > stop ? stop : begin;
        const int64_t end = begin + d.bits < stop ? begin + d.bits : stop;
        info = make_int4((int)begin, (int)end, lo, s == off ? 1 : 0);
    }
    d.sub_info[s] = info;
    if (s % RUN == 0) d.head[s / RUN] = pack_state(info.x, 0, 0);
}

// ---- 3. synchronisation ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RUN) void jpegdec_sync_kernel(Dec d, int launch) {
    __shared__ u64 s_exit[RUN];
    __shared__ int32_t s_tab[MTGS_JPEGDEC_TABLE_WORDS];
    if (launch > 0 && d.flags[launch - 1] == 0) return;       // the launch before this one changed nothing: the fixed point
    stage_tables(d, s_tab);
    const int tid = threadIdx.x, wg = blockIdx.x;
    const int s = wg * RUN + tid;
    const bool active = s < n_subsequences(d);
    const int4 info = active ? d.sub_info[s] : make_int4(0, 0, 0, 1);
    const bool first = info.w != 0;
    const u64 *head_in = d.head + (size_t)(launch & 1) * (d.n_wg + 1);
    u64 *head_out = d.head + (size_t)((launch + 1) & 1) * (d.n_wg + 1);
    u64 e = pack_state(info.x, 0, 0);
    if (launch > 0 && active) e = d.entry[s];
    bool dirty = active && launch == 0, changed = false, decoded = false;
    if (tid == 0 && active && !first) {
        const u64 h = head_in[wg];
        if (h != e) e = h, dirty = changed = true;
    }
    u64 exit_state = NONE;
    int done = 0;
    for (int it = 0; it < RUN; ++it) {
        u64 x = NONE;
        if (dirty) {
            done = 0;
            x = exit_state = decode<false>(d, s_tab, e, info.y, done, 0, 0);
            decoded = true;
            dirty = false;
        }
        s_exit[tid] = x;
        __syncthreads();
        if (tid > 0 && active && !first) {
            const u64 y = s_exit[tid - 1];
            if (y != NONE && y != e) e = y, dirty = changed = true;
        }
        if (!__syncthreads_or(dirty)) break;
    }
    if (active) {
        d.entry[s] = e;
        if (decoded) d.count[s] = done;
    }
    if (tid == RUN - 1) head_out[wg + 1] = decoded ? exit_state : head_in[wg + 1];
    if (__syncthreads_or(changed) && tid == 0) atomicOr(d.flags + launch, 1);
}

// ---- 4. counts, coefficients -------------------------------------------------------------------------------------------------------
struct CountValue {
    Dec d;
    __device__ int64_t operator()(int64_t s) const { return s < n_subsequences(d) ? d.count[s] : 0; }
};

struct CountSink {
    Dec d;
    __device__ void operator()(int64_t s, int64_t excl, int64_t) const { d.before[s] = (int32_t)excl; }
};

__global__ __launch_bounds__(256) void jpegdec_write_kernel(Dec d) {
    __shared__ int32_t s_tab[MTGS_JPEGDEC_TABLE_WORDS];
    stage_tables(d, s_tab);
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n_subsequences(d)) return;
    const int4 info = d.sub_info[s];
    const int k = info.z;
    const int local = d.before[s] - d.before[d.sub_offset[k]];          // blocks of this interval completed before s
    const int limit = blocks_of_interval(d, k) - local;
    int done = 0;
    const u64 e = info.w ? pack_state(info.x, 0, 0) : d.entry[s];
    if (limit > 0 && local >= 0) decode<true>(d, s_tab, e, info.y, done, (int64_t)k * d.ri * d.nb + local, limit);
}

// ---- 5. DC prediction --------------------------------------------------------------------------------------------------------------
template <bool LUMA>
struct DcValue {
    Dec d;
    __device__ int64_t operator()(int64_t i) const {
        const int comp = component_of(d, (int)(i % d.nb));
        const int64_t v = d.coef[i * 64];
        if (LUMA) return comp == 0 ? v : 0;
        return comp == 1 ? v * ((int64_t)1 << 32) : (comp == 2 ? v : 0);
    }
};

template <bool LUMA>
struct DcSink {
    Dec d;
    __device__ void operator()(int64_t i, int64_t, int64_t incl) const {
        const int comp = component_of(d, (int)(i % d.nb));
        if (LUMA) {
            if (comp == 0) d.dcsum[i] = (int32_t)incl;
            return;
        }
        const int64_t low = (int64_t)(int32_t)(incl & LOW32);             // Cr: the signed low half; Cb: what is left above it
        if (comp == 1) d.dcsum[i] = (int32_t)((incl - low) >> 32);
        if (comp == 2) d.dcsum[i] = (int32_t)low;
    }
};

// ---- 6. IDCT -----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// jidctint's butterfly on in[0..7]; out[k] before the descale
__device__ __forceinline__ void idct8(const int *in, int *out) {
    int z1 = (in[2] + in[6]) * 4433;
    const int e2 = z1 - in[6] * 15137, e3 = z1 + in[2] * 6270;
    const int e0 = (in[0] + in[4]) * 8192, e1 = (in[0] - in[4]) * 8192;
    const int t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
    int t0 = in[7], t1 = in[5], t2 = in[3], t3 = in[1];
    z1 = t0 + t3;
    int z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const int z5 = (z3 + z4) * 9633;
    t0 *= 2446, t1 *= 16819, t2 *= 25172, t3 *= 12299;
    z1 *= -7373, z2 *= -20995, z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
    t0 += z1 + z3, t1 += z2 + z4, t2 += z2 + z3, t3 += z1 + z4;
    out[0] = t10 + t3, out[7] = t10 - t3, out[1] = t11 + t2, out[6] = t11 - t2;
    out[2] = t12 + t1, out[5] = t12 - t1, out[3] = t13 + t0, out[4] = t13 - t0;
}

__global__ __launch_bounds__(256) void jpegdec_idct_kernel(Dec d) {
    __shared__ int s_ws[32][65];
    const int b = threadIdx.x >> 3, j = threadIdx.x & 7;
    const int64_t i = (int64_t)blockIdx.x * 32 + b;
    const bool valid = i < d.n_blocks;
    int comp = 0, blk = 0;
    int64_t mcu = 0;
    if (valid) {
        mcu = i / d.nb;
        blk = (int)(i - mcu * d.nb);
        comp = component_of(d, blk);
        const int16_t *c = d.coef + i * 64;
        const int32_t *q = d.tab + QUANT_AT + comp * 64;
        int in[8], out[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) in[r] = (int)c[8 * r + j] * q[8 * r + j];
        if (j == 0) {
            // the DC: the prefix of the differences, less the prefix before the interval's first block of this component
            const int64_t i0 = (mcu / d.ri) * d.ri * d.nb + (comp == 0 ? 0 : blk);
            in[0] = (d.dcsum[i] - (d.dcsum[i0] - (int)d.coef[i0 * 64])) * q[0];
        }
        idct8(in, out);
#pragma unroll
        for (int r = 0; r < 8; ++r) s_ws[b][8 * r + j] = descale(out[r], 11);
    }
    __syncthreads();
    if (valid) {
        int in[8], out[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) in[k] = s_ws[b][8 * j + k];
        idct8(in, out);
        const int my = (int)(mcu / d.mcus_x), mx = (int)(mcu - (int64_t)my * d.mcus_x);
        int bx = mx, by = my;
        if (comp == 0) bx = mx * d.hs + blk % d.hs, by = my * d.vs + blk / d.hs;
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            int v = descale(out[k], 18) + 128;
            v = v < 0 ? 0 : (v > 255 ? 255 : v);
            if (k < 4) lo |= (uint32_t)v << (8 * k);
            else hi |= (uint32_t)v << (8 * (k - 4));
        }
        uint8_t *row = d.plane[comp] + ((size_t)by * 8 + j) * d.plane_w[comp] + (size_t)bx * 8;   // 8-byte aligned
        *(uint2 *)row = make_uint2(lo, hi);
    }
}

// ---- 7. upsampling, colour, store --------------------------------------------------------------------------------------------------
__device__ __forceinline__ int chroma_at(const Dec &d, int c, int x, int y) {
    const uint8_t *p = d.plane[c];
    const int pw = d.plane_w[c];
    if (d.hs == 1) return p[(size_t)y * pw + x];
    const int cw = (d.W + 1) >> 1, cx = x >> 1;
    if (cw <= 2) return p[(size_t)(y >> (d.vs - 1)) * pw + cx];      // jdsample.c: fancy only for components wider than two samples
    if (d.vs == 1) {
        const uint8_t *row = p + (size_t)y * pw;
        const int v = row[cx];
        if (x & 1) return cx == cw - 1 ? v : (3 * v + row[cx + 1] + 2) >> 2;
        return cx == 0 ? v : (3 * v + row[cx - 1] + 1) >> 2;
    }
    const int ch = (d.H + 1) >> 1, cy = y >> 1;
    const int other = (y & 1) ? (cy + 1 < ch ? cy + 1 : ch - 1) : (cy > 0 ? cy - 1 : 0);
    const uint8_t *near = p + (size_t)cy * pw, *far = p + (size_t)other * pw;
    const int s = 3 * near[cx] + far[cx];
    if (x & 1) return cx == cw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * near[cx + 1] + far[cx + 1] + 7) >> 4;
    return cx == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * near[cx - 1] + far[cx - 1] + 8) >> 4;
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

template <bool FLOAT>
__global__ __launch_bounds__(256) void jpegdec_colour_kernel(Dec d, void *__restrict__ out, int64_t sy, int64_t sx, int64_t sc) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)d.H * d.W) return;
    const int y = (int)(i / d.W), x = (int)(i - (int64_t)y * d.W);
    const int Y = d.plane[0][(size_t)y * d.plane_w[0] + x];
    const int cb = chroma_at(d, 1, x, y) - 128, cr = chroma_at(d, 2, x, y) - 128;
    const int rgb[3] = {clamp255(Y + ((91881 * cr + 32768) >> 16)), clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16)),
                        clamp255(Y + ((116130 * cb + 32768) >> 16))};
    const int64_t at = y * sy + x * sx;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (FLOAT) ((float *)out)[at + c * sc] = __fdiv_rn((float)rgb[c], 255.0f);
        else ((uint8_t *)out)[at + c * sc] = (uint8_t)rgb[c];
    }
}

// ---- 8. status ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void jpegdec_status_kernel(Dec d, int32_t *__restrict__ status) {
    const int lane = threadIdx.x;
    int blocks = 0, short_of = 0, launches = 0;
    for (int k = lane; k < d.n_int; k += 64) {
        const int want = blocks_of_interval(d, k);
        const int got = d.before[d.sub_offset[k + 1]] - d.before[d.sub_offset[k]];
        blocks += got < want ? (got < 0 ? 0 : got) : want;
        short_of |= got < want;
    }
    for (int l = lane; l < d.n_wg; l += 64) launches += d.flags[l] != 0;
    blocks = wave_sum_all(blocks), short_of = wave_sum_all(short_of), launches = wave_sum_all(launches);
    if (lane == 0) {
        const int markers = (int)(d.totals[0] >> 32);
        status[0] = (markers != d.n_int - 1 ? MTGS_JPEGDEC_ERR_MARKERS : 0) | (short_of ? MTGS_JPEGDEC_ERR_BLOCKS : 0);
        status[1] = blocks;
        status[2] = (int32_t)d.n_blocks;
        status[3] = launches;
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
int check_shape(const char *fn, int h, int w, int subsampling, int restart_interval, int64_t scan_bytes, int &bits) {
    MTGS_REQUIRE(subsampling == MTGS_JPEGDEC_444 || subsampling == MTGS_JPEGDEC_422 || subsampling == MTGS_JPEGDEC_420, MTGS_EUNSUPPORTED,
                 "%s: subsampling %d is not implemented (MTGS_JPEGDEC_444, _422 or _420)", fn, subsampling);
    MTGS_REQUIRE(h >= 1 && h <= 65535 && w >= 1 && w <= 65535, MTGS_EINVAL, "%s: h and w outside [1, 65535] (%d, %d)", fn, h, w);
    MTGS_REQUIRE(restart_interval >= 0 && restart_interval <= 65535, MTGS_EINVAL, "%s: restart_interval outside [0, 65535] (%d)", fn,
                 restart_interval);
    MTGS_REQUIRE(scan_bytes >= 1 && scan_bytes < ((int64_t)1 << 27), MTGS_EINVAL, "%s: scan_bytes outside [1, 2^27) (%lld)", fn,
                 (long long)scan_bytes);
    if (bits == 0) bits = MTGS_JPEGDEC_SUBSEQUENCE_BITS;
    MTGS_REQUIRE(bits >= 32 && bits <= 65536 && bits % 32 == 0, MTGS_EINVAL,
                 "%s: subsequence_bits must be a multiple of 32 in [32, 65536] (%d)", fn, bits);
    return MTGS_OK;
}

}  // namespace

extern "C" int mtgs_jpegdec_sizes(int h, int w, int subsampling, int restart_interval, int64_t scan_bytes, int subsequence_bits,
                                  size_t *ws_bytes) {
    const char *fn = "mtgs_jpegdec_sizes";
    if (int rc = check_shape(fn, h, w, subsampling, restart_interval, scan_bytes, subsequence_bits)) return rc;
    MTGS_REQUIRE(ws_bytes != nullptr, MTGS_EINVAL, "%s: null pointer: ws_bytes", fn);
    *ws_bytes = geometry(h, w, subsampling, restart_interval, scan_bytes, subsequence_bits, nullptr).bytes;
    return MTGS_OK;
}

extern "C" int mtgs_jpegdec_decode(const uint8_t *scan, int64_t scan_bytes, const int32_t *tables, int h, int w, int subsampling,
                                   int restart_interval, int subsequence_bits, void *out, int is_float, int64_t stride_y,
                                   int64_t stride_x, int64_t stride_c, int32_t *status, void *ws, size_t ws_bytes, void *stream) {
    const char *fn = "mtgs_jpegdec_decode";
    if (int rc = check_shape(fn, h, w, subsampling, restart_interval, scan_bytes, subsequence_bits)) return rc;
    MTGS_REQUIRE(scan != nullptr, MTGS_EINVAL, "%s: null pointer: scan", fn);
    MTGS_REQUIRE(tables != nullptr && ((uintptr_t)tables & 3) == 0, MTGS_EINVAL, "%s: tables must be a non-null, 4-byte aligned int32 array", fn);
    MTGS_REQUIRE(out != nullptr, MTGS_EINVAL, "%s: null pointer: out", fn);
    MTGS_REQUIRE(!is_float || ((uintptr_t)out & 3) == 0, MTGS_EINVAL, "%s: a float32 out must be 4-byte aligned", fn);
    MTGS_REQUIRE(stride_y >= 0 && stride_x >= 0 && stride_c >= 0, MTGS_EINVAL, "%s: negative stride (%lld, %lld, %lld)", fn,
                 (long long)stride_y, (long long)stride_x, (long long)stride_c);
    MTGS_REQUIRE(status != nullptr && ((uintptr_t)status & 3) == 0, MTGS_EINVAL, "%s: status must be a non-null, 4-byte aligned int32[4]", fn);
    MTGS_REQUIRE(ws != nullptr, MTGS_EINVAL, "%s: null pointer: ws", fn);
    MTGS_REQUIRE(((uintptr_t)ws & 15) == 0, MTGS_EINVAL, "%s: workspace must be 16-byte aligned", fn);
    Dec d = geometry(h, w, subsampling, restart_interval, scan_bytes, subsequence_bits, ws);
    MTGS_REQUIRE(ws_bytes >= d.bytes, MTGS_EWORKSPACE, "%s: workspace %zu < %zu bytes", fn, ws_bytes, d.bytes);
    d.scan = scan;
    d.tab = tables;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = mtgs_zero_async(ws, d.zero_bytes, st)) return rc;
    mtgs_scan::run(d.cap_bytes, CleanValue{scan, scan_bytes}, CleanSink{d}, d.spine, d.totals, st);
    mtgs_scan::run(d.n_int, CutValue{d}, CutSink{d}, d.spine, d.totals + 1, st);
    jpegdec_setup_kernel<<<(unsigned)ceil_div64(d.n_sub_max, 256), 256, 0, st>>>(d);
    for (int launch = 0; launch < d.n_wg; ++launch) jpegdec_sync_kernel<<<(unsigned)d.n_wg, RUN, 0, st>>>(d, launch);
    mtgs_scan::run((int64_t)d.n_sub_max + 1, CountValue{d}, CountSink{d}, d.spine, d.totals + 2, st);
    jpegdec_write_kernel<<<(unsigned)ceil_div64(d.n_sub_max, 256), 256, 0, st>>>(d);
    mtgs_scan::run(d.n_blocks, DcValue<true>{d}, DcSink<true>{d}, d.spine, d.totals + 3, st);
    mtgs_scan::run(d.n_blocks, DcValue<false>{d}, DcSink<false>{d}, d.spine, d.totals + 3, st);
    jpegdec_idct_kernel<<<(unsigned)ceil_div64(d.n_blocks, 32), 256, 0, st>>>(d);
    const unsigned pixel_blocks = (unsigned)ceil_div64((int64_t)h * w, 256);
    if (is_float) jpegdec_colour_kernel<true><<<pixel_blocks, 256, 0, st>>>(d, out, stride_y, stride_x, stride_c);
    else jpegdec_colour_kernel<false><<<pixel_blocks, 256, 0, st>>>(d, out, stride_y, stride_x, stride_c);
    jpegdec_status_kernel<<<1, 64, 0, st>>>(d, status);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}
