// frame.hip -- a training frame at its stage's resolution (CustomInputDataset._resize_data, mtgs/dataset/custom_dataset.py:279-304,
// and the mask preparation of :203-274): Pillow's BILINEAR resampling of 8-bit and float32 images and its NEAREST resampling of
// the label planes, byte for byte, from host-built tables.  include/mtgs_frame.h states the arithmetic; this file is compiled with
// -ffp-contract=off because the float32 path rounds every product and every sum of (double)float * double once.
//
// frame_resize_kernel<T>, one launch per image: a workgroup owns TW x TH output pixels (all channels).  The source rows the tile
// needs, [first row of its top output, last row of its bottom output], are walked in chunks of RCH rows:
//   (contiguous pixels)        stage the chunk's row spans into LDS with aligned dword loads, five in flight per thread -- a
//                              3-byte pixel read byte by byte from global memory costs one request per byte, and a tap loop
//                              that reads global memory pays a round trip per tap; the dwords of a row are coalesced
//   horizontal                 every (row, column, channel) of the chunk: Pillow's filter, ROUNDED to T, into LDS
//   vertical                   every thread adds the chunk's taps to the accumulators of its 6 outputs, rows ascending
// so the order of every sum is Pillow's whatever the chunking, the horizontal result is rounded before the vertical pass reads it,
// and neither tap count is bounded.  An identity pass (size unchanged) copies.  Vertically adjacent tiles recompute the rows they
// share (2 of 34 at scale 0.5); in exchange there is no [h, ow] intermediate in global memory and one launch instead of two.
//
// frame_nearest_kernel, one launch for all nearest planes of a frame (the table idea of crop.hip's gather and refine.hip's row
// moves): blockIdx.y names the plane, a thread one output pixel; the panoptic split, the invalid-pixel fills and the label
// membership are applied to the gathered element, which equals applying them at full size first.
#include <type_traits>

#include "common.hpp"

namespace {

constexpr int TW = MTGS_FRAME_TILE_W, TH = MTGS_FRAME_TILE_H, RCH = MTGS_FRAME_CHUNK_ROWS, RAW_ROW = MTGS_FRAME_RAW_ROW_BYTES;
constexpr int NT = 512, MAXC = 3, NW = NT / MTGS_WAVE, KCAP = 8;
constexpr int HROWS = RCH / NW, VROWS = TH / NW, COLS = TW * MAXC / MTGS_WAVE;   // per wave: source rows of a chunk, output rows; per lane: columns
static_assert(RCH % NW == 0 && TH % NW == 0 && TW * MAXC % MTGS_WAVE == 0 && RAW_ROW % 4 == 0, "tile constants");

template <class T> struct Px;
template <> struct Px<uint8_t> {
    using Coef = int32_t;
    using Acc = int32_t;
    static __device__ __forceinline__ Acc zero() { return 1 << 21; }
    static __device__ __forceinline__ Acc mac(Acc a, uint8_t p, Coef k) { return a + (int32_t)p * k; }
    static __device__ __forceinline__ Acc same(uint8_t p) { return ((int32_t)p << 22) + (1 << 21); }
    static __device__ __forceinline__ uint8_t round(Acc a) {
        const int32_t v = a >> 22;
        return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
    }
};
template <> struct Px<float> {
    using Coef = double;
    using Acc = double;
    static __device__ __forceinline__ Acc zero() { return 0.0; }
    static __device__ __forceinline__ Acc mac(Acc a, float p, Coef k) { return a + (double)p * k; }   // two roundings: no fma here
    static __device__ __forceinline__ Acc same(float p) { return (double)p; }                            // exact, and back
    static __device__ __forceinline__ float round(Acc a) { return (float)a; }
};

template <class T>
struct ResizeArgs {
    const T *src;
    int64_t sh, sw, sc;
    int h, w, c, oh, ow;
    const int32_t *hb, *vb;
    const typename Px<T>::Coef *hk, *vk;
    int hks, vks;
    void *dst;
    int out_float;
};

// (first source index, taps) of output j, clamped to the source: a table that is not mtgs_amd.frame's is not followed outside it
__device__ __forceinline__ void bound(const int32_t *__restrict__ b, int j, int in_size, int ksize, bool identity, int &first, int &n) {
    if (identity) {
        first = j;
        n = 1;
        return;
    }
    first = min(max(b[2 * j], 0), in_size - 1);
    n = min(min(max(b[2 * j + 1], 0), ksize), in_size - first);
}

template <class T>
__global__ __launch_bounds__(NT) void frame_resize_kernel(ResizeArgs<T> a) {
    using P = Px<T>;
    using Acc = typename P::Acc;
    constexpr bool U8 = std::is_same<T, uint8_t>::value;
    __shared__ T inter[RCH * TW * MAXC];
    __shared__ uint32_t raw[RCH * RAW_ROW / 4];
    __shared__ typename P::Coef hk_s[TW * KCAP], vk_s[TH * KCAP];
    __shared__ int hb_s[TW * 2], vb_s[TH * 2];

    const int tid = threadIdx.x;
    const int tiles_x = (a.ow + TW - 1) / TW;
    const int x0 = (int)(blockIdx.x % tiles_x) * TW, y0 = (int)(blockIdx.x / tiles_x) * TH;
    const int tw = min(TW, a.ow - x0), th = min(TH, a.oh - y0);
    const int c = a.c, rowlen = tw * c;
    const bool hid = a.w == a.ow, vid = a.h == a.oh;

    int first, n;
    bound(a.vb, y0, a.h, a.vks, vid, first, n);
    const int r_begin = first;
    bound(a.vb, y0 + th - 1, a.h, a.vks, vid, first, n);
    const int r_end = min(first + n, a.h);
    bound(a.hb, x0, a.w, a.hks, hid, first, n);
    const int col_begin = first;
    bound(a.hb, x0 + tw - 1, a.w, a.hks, hid, first, n);
    const int col_end = min(first + n, a.w);
    const int seg = (col_end - col_begin) * c * (int)sizeof(T);     // bytes of a source row this tile reads
    const bool staged = a.sc == 1 && a.sw == c && seg > 0 && seg + 6 <= RAW_ROW;

    // the tile's rows of the tables, once, into LDS: a table read from global memory inside the tap loops is a dependent round trip
    // per tap.  Filters longer than KCAP taps keep their coefficients in global memory (the bounds are staged either way).
    const bool hk_lds = a.hks <= KCAP, vk_lds = a.vks <= KCAP;
    for (int e = tid; e < tw; e += NT) {
        bound(a.hb, x0 + e, a.w, a.hks, hid, first, n);
        hb_s[2 * e] = first;
        hb_s[2 * e + 1] = n;
    }
    for (int e = tid; e < th; e += NT) {
        bound(a.vb, y0 + e, a.h, a.vks, vid, first, n);
        vb_s[2 * e] = first;
        vb_s[2 * e + 1] = n;
    }
    if (!hid && hk_lds)
        for (int e = tid; e < tw * KCAP; e += NT) hk_s[e] = (e % KCAP) < a.hks ? a.hk[(int64_t)(x0 + e / KCAP) * a.hks + e % KCAP] : typename P::Coef(0);
    if (!vid && vk_lds)
        for (int e = tid; e < th * KCAP; e += NT) vk_s[e] = (e % KCAP) < a.vks ? a.vk[(int64_t)(y0 + e / KCAP) * a.vks + e % KCAP] : typename P::Coef(0);
    __syncthreads();

    // a wave owns the source rows wave, wave + NW, .. of a chunk and the output rows wave, wave + NW, .. of the tile; a lane owns the
    // columns lane, lane + 64, .. of either.  So a coefficient is loaded once for HROWS (VROWS x COLS) independent sums, and the
    // vertical pass's bounds and coefficients are wave-uniform.
    const int lane = tid & (MTGS_WAVE - 1), wave = __builtin_amdgcn_readfirstlane(tid / MTGS_WAVE);
    const uint8_t *rawb = (const uint8_t *)raw;
    Acc acc[VROWS][COLS];
#pragma unroll
    for (int q = 0; q < VROWS; ++q)
#pragma unroll
        for (int j = 0; j < COLS; ++j) acc[q][j] = P::zero();

    for (int c0 = r_begin; c0 < r_end; c0 += RCH) {
        const int c1 = min(c0 + RCH, r_end), rows = c1 - c0;
        if (staged) {
            const int ndw = (seg + 6) >> 2;                          // the most dwords a row's span touches, whatever its alignment
            // a wave stages the rows it will filter itself, a lane the dwords lane, lane + 64, .. of each: no division, and the
            // loads of all its rows are issued before the first LDS write waits for one
#pragma unroll
            for (int g = 0; g < RAW_ROW / 4; g += MTGS_WAVE) {
                if (g < ndw) {
                    uint32_t v[HROWS];
                    int to[HROWS];
#pragma unroll
                    for (int q = 0; q < HROWS; ++q) {                // every lane loads, from a clamped address: no branch between the loads
                        const int rr = min(wave + q * NW, rows - 1), k = g + lane;
                        const uintptr_t p = (uintptr_t)(a.src + ((int64_t)(c0 + rr) * a.sh + (int64_t)col_begin * c));
                        const int al = (int)(p & 3), last = ((al + seg + 3) >> 2) - 1;
                        v[q] = ((const uint32_t *)(p - al))[min(k, last)];
                        to[q] = (wave + q * NW < rows && k <= last) ? rr * (RAW_ROW / 4) + k : -1;
                    }
#pragma unroll
                    for (int q = 0; q < HROWS; ++q)
                        if (to[q] >= 0) raw[to[q]] = v[q];
                }
            }
            __syncthreads();
        }
        // horizontal pass of the chunk, rounded to T
        int rawrow[HROWS];                                           // where a staged row's span starts in `raw`: its own alignment
#pragma unroll
        for (int q = 0; q < HROWS; ++q) {
            const int rr = wave + q * NW;
            const uintptr_t p = (uintptr_t)(a.src + ((int64_t)(c0 + rr) * a.sh + (int64_t)col_begin * c));
            rawrow[q] = rr * RAW_ROW + (int)(p & 3);
        }
#pragma unroll
        for (int j = 0; j < COLS; ++j) {
            const int xc = lane + j * MTGS_WAVE;
            if (xc < rowlen) {
                const int x = xc / c, ch = xc - x * c;
                first = hb_s[2 * x];
                n = hb_s[2 * x + 1];
                if (staged) {
                    first = max(first, col_begin);                   // no-ops on a monotone table: the staged span is never left
                    n = min(n, col_end - first);
                }
                const typename P::Coef *__restrict__ kk = a.hk + (int64_t)(x0 + x) * a.hks;
                const int in_raw = ((first - col_begin) * c + ch) * (int)sizeof(T);
                const T *g = a.src + (int64_t)c0 * a.sh + (int64_t)first * a.sw + (int64_t)ch * a.sc;
                Acc s[HROWS];
#pragma unroll
                for (int q = 0; q < HROWS; ++q) s[q] = P::zero();
                for (int i = 0; i < n; ++i) {
                    const typename P::Coef k = hid ? typename P::Coef(0) : (hk_lds ? hk_s[x * KCAP + i] : kk[i]);
#pragma unroll
                    for (int q = 0; q < HROWS; ++q) {
                        const int rr = wave + q * NW;
                        if (rr < rows) {
                            T px;
                            if (staged) px = *(const T *)(rawb + rawrow[q] + in_raw + i * c * (int)sizeof(T));
                            else px = g[(int64_t)rr * a.sh + (int64_t)i * a.sw];
                            s[q] = hid ? P::same(px) : P::mac(s[q], px, k);
                        }
                    }
                }
#pragma unroll
                for (int q = 0; q < HROWS; ++q) {
                    const int rr = wave + q * NW;
                    if (rr < rows) inter[rr * rowlen + xc] = P::round(s[q]);
                }
            }
        }
        __syncthreads();
        // the chunk's share of the vertical pass, rows ascending
#pragma unroll
        for (int q = 0; q < VROWS; ++q) {
            const int y = wave + q * NW;
            if (y < th) {
                first = vb_s[2 * y];
                n = vb_s[2 * y + 1];
                const int lo = max(first, c0), hi = min(first + n, c1);
                const typename P::Coef *__restrict__ kk = a.vk + (int64_t)(y0 + y) * a.vks - first;
                for (int r = lo; r < hi; ++r) {
                    const typename P::Coef k = vid ? typename P::Coef(0) : (vk_lds ? vk_s[y * KCAP + r - first] : kk[r]);
#pragma unroll
                    for (int j = 0; j < COLS; ++j) {
                        const int xc = lane + j * MTGS_WAVE;
                        if (xc < rowlen) {
                            const T px = inter[(r - c0) * rowlen + xc];
                            acc[q][j] = vid ? P::same(px) : P::mac(acc[q][j], px, k);
                        }
                    }
                }
            }
        }
        __syncthreads();
    }

#pragma unroll
    for (int q = 0; q < VROWS; ++q) {
        const int y = wave + q * NW;
#pragma unroll
        for (int j = 0; j < COLS; ++j) {
            const int xc = lane + j * MTGS_WAVE;
            if (y < th && xc < rowlen) {
                const int64_t at = ((int64_t)(y0 + y) * a.ow + x0) * c + xc;
                const T v = P::round(acc[q][j]);
                if (U8 && !a.out_float) ((uint8_t *)a.dst)[at] = (uint8_t)v;
                else if (U8) ((float *)a.dst)[at] = __fdiv_rn((float)v, 255.0f);
                else ((float *)a.dst)[at] = (float)v;
            }
        }
    }
}

struct NearestTable {
    mtgs_frame_plane p[MTGS_FRAME_MAX_PLANES];
    uint32_t labels[8];
};

__global__ __launch_bounds__(NT) void frame_nearest_kernel(NearestTable t, int h, int w, int oh, int ow, const int32_t *__restrict__ sy,
                                                           const int32_t *__restrict__ sx) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= (int64_t)oh * ow) return;
    const mtgs_frame_plane &p = t.p[blockIdx.y];
    const int y = (int)(i / ow), x = (int)(i - (int64_t)y * ow);
    const int64_t ys = min(max(sy[y], 0), h - 1), xs = min(max(sx[x], 0), w - 1);
    const int64_t at = ys * p.src_stride[0] + xs * p.src_stride[1];
    const bool valid = p.valid == nullptr || p.valid[ys * p.valid_stride[0] + xs * p.valid_stride[1]] != 0;
    if (p.op == MTGS_FRAME_COPY) {
        if (p.elem_bytes == 4) {
            for (int k = 0; k < p.channels; ++k) ((uint32_t *)p.dst)[i * p.channels + k] = ((const uint32_t *)p.src)[at + k * p.src_stride[2]];
        } else {
            for (int k = 0; k < p.channels; ++k) ((uint8_t *)p.dst)[i * p.channels + k] = ((const uint8_t *)p.src)[at + k * p.src_stride[2]];
        }
        return;
    }
    const uint8_t *s = (const uint8_t *)p.src + at;
    if (p.op == MTGS_FRAME_INSTANCE) {
        ((int32_t *)p.dst)[i] = valid ? (int32_t)s[0] + 256 * (int32_t)s[p.src_stride[2]] : 0;
    } else if (p.op == MTGS_FRAME_SEMANTIC) {
        ((uint8_t *)p.dst)[i] = valid ? s[0] : (uint8_t)255;
    } else {
        const uint32_t l = s[0];
        ((uint8_t *)p.dst)[i] = (valid && !((t.labels[l >> 5] >> (l & 31)) & 1u)) ? 1 : 0;
    }
}

int check_sizes(const char *fn, int h, int w, int oh, int ow) {
    MTGS_REQUIRE(h >= 1 && h <= MTGS_FRAME_MAX_SIZE, MTGS_EINVAL, "%s: h outside [1, %d] (%d)", fn, MTGS_FRAME_MAX_SIZE, h);
    MTGS_REQUIRE(w >= 1 && w <= MTGS_FRAME_MAX_SIZE, MTGS_EINVAL, "%s: w outside [1, %d] (%d)", fn, MTGS_FRAME_MAX_SIZE, w);
    MTGS_REQUIRE(oh >= 1 && oh <= MTGS_FRAME_MAX_SIZE, MTGS_EINVAL, "%s: oh outside [1, %d] (%d)", fn, MTGS_FRAME_MAX_SIZE, oh);
    MTGS_REQUIRE(ow >= 1 && ow <= MTGS_FRAME_MAX_SIZE, MTGS_EINVAL, "%s: ow outside [1, %d] (%d)", fn, MTGS_FRAME_MAX_SIZE, ow);
    return MTGS_OK;
}

template <class T>
int resize(const char *fn, int h, int w, int c, const T *src, int64_t sh, int64_t sw, int64_t sc, int oh, int ow, const int32_t *hb,
           const typename Px<T>::Coef *hk, int hks, const int32_t *vb, const typename Px<T>::Coef *vk, int vks, int out_float, void *dst,
           void *stream) {
    if (int rc = check_sizes(fn, h, w, oh, ow)) return rc;
    MTGS_REQUIRE(c >= 1 && c <= MAXC, MTGS_EUNSUPPORTED, "%s: c outside [1, %d] (%d)", fn, MAXC, c);
    MTGS_NONNULL(fn, src); MTGS_NONNULL(fn, dst);
    if (w != ow) {
        MTGS_NONNULL(fn, hb); MTGS_NONNULL(fn, hk);
        MTGS_REQUIRE(hks >= 1, MTGS_EINVAL, "%s: hk < 1 (%d)", fn, hks);
    }
    if (h != oh) {
        MTGS_NONNULL(fn, vb); MTGS_NONNULL(fn, vk);
        MTGS_REQUIRE(vks >= 1, MTGS_EINVAL, "%s: vk < 1 (%d)", fn, vks);
    }
    MTGS_REQUIRE(((uintptr_t)dst & (out_float ? 3 : 0)) == 0, MTGS_EINVAL, "%s: dst must be 4-byte aligned", fn);
    const int64_t tiles = ceil_div64(ow, TW) * ceil_div64(oh, TH);
    MTGS_REQUIRE(tiles < ((int64_t)1 << 31), MTGS_EINVAL, "%s: %lld output tiles", fn, (long long)tiles);
    ResizeArgs<T> a{src, sh, sw, sc, h, w, c, oh, ow, hb, vb, hk, vk, hks, vks, dst, out_float};
    frame_resize_kernel<T><<<(unsigned)tiles, NT, 0, (hipStream_t)stream>>>(a);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}

}  // namespace


extern "C" int mtgs_frame_resize_u8(int h, int w, int c, const uint8_t *src, int64_t stride_h, int64_t stride_w, int64_t stride_c,
                                    int oh, int ow, const int32_t *hbounds, const int32_t *hcoef, int hk, const int32_t *vbounds,
                                    const int32_t *vcoef, int vk, int out_float, void *dst, void *stream) {
    return resize<uint8_t>("mtgs_frame_resize_u8", h, w, c, src, stride_h, stride_w, stride_c, oh, ow, hbounds, hcoef, hk, vbounds,
                           vcoef, vk, out_float != 0, dst, stream);
}

extern "C" int mtgs_frame_resize_f32(int h, int w, int c, const float *src, int64_t stride_h, int64_t stride_w, int64_t stride_c,
                                     int oh, int ow, const int32_t *hbounds, const double *hcoef, int hk, const int32_t *vbounds,
                                     const double *vcoef, int vk, float *dst, void *stream) {
    const char *fn = "mtgs_frame_resize_f32";
    MTGS_REQUIRE(((uintptr_t)src & 3) == 0, MTGS_EINVAL, "%s: src must be 4-byte aligned", fn);
    MTGS_REQUIRE((((uintptr_t)hcoef | (uintptr_t)vcoef) & 7) == 0, MTGS_EINVAL, "%s: hcoef and vcoef must be 8-byte aligned", fn);
    return resize<float>(fn, h, w, c, src, stride_h, stride_w, stride_c, oh, ow, hbounds, hcoef, hk, vbounds, vcoef, vk, 1, dst, stream);
}

extern "C" int mtgs_frame_nearest(int h, int w, int oh, int ow, const int32_t *sy, const int32_t *sx, int n_planes,
                                  const mtgs_frame_plane *planes, const uint8_t *labels, void *stream) {
    const char *fn = "mtgs_frame_nearest";
    if (int rc = check_sizes(fn, h, w, oh, ow)) return rc;
    MTGS_REQUIRE(n_planes >= 1 && n_planes <= MTGS_FRAME_MAX_PLANES, MTGS_EINVAL, "%s: n_planes outside [1, %d] (%d)", fn,
                 MTGS_FRAME_MAX_PLANES, n_planes);
    MTGS_NONNULL(fn, sy); MTGS_NONNULL(fn, sx); MTGS_NONNULL(fn, planes);
    NearestTable t{};
    for (int j = 0; j < n_planes; ++j) {
        const mtgs_frame_plane &p = planes[j];
        MTGS_REQUIRE(p.src != nullptr && p.dst != nullptr, MTGS_EINVAL, "%s: null pointer: planes[%d].%s", fn, j, p.src ? "dst" : "src");
        MTGS_REQUIRE(p.op >= MTGS_FRAME_COPY && p.op <= MTGS_FRAME_MASK, MTGS_EINVAL, "%s: planes[%d].op unknown (%d)", fn, j, p.op);
        if (p.op == MTGS_FRAME_COPY) {
            MTGS_REQUIRE(p.elem_bytes == 1 || p.elem_bytes == 4, MTGS_EUNSUPPORTED, "%s: planes[%d].elem_bytes must be 1 or 4 (%d)", fn, j, p.elem_bytes);
            MTGS_REQUIRE(p.channels >= 1 && p.channels <= MAXC, MTGS_EUNSUPPORTED, "%s: planes[%d].channels outside [1, %d] (%d)", fn, j, MAXC, p.channels);
        }
        const bool words = p.op == MTGS_FRAME_INSTANCE || (p.op == MTGS_FRAME_COPY && p.elem_bytes == 4);
        MTGS_REQUIRE(!words || ((uintptr_t)p.dst & 3) == 0, MTGS_EINVAL, "%s: planes[%d].dst must be 4-byte aligned", fn, j);
        MTGS_REQUIRE(!(p.op == MTGS_FRAME_COPY && p.elem_bytes == 4) || ((uintptr_t)p.src & 3) == 0, MTGS_EINVAL,
                     "%s: planes[%d].src must be 4-byte aligned", fn, j);
        t.p[j] = p;
    }
    if (labels)
        for (int l = 0; l < 256; ++l)
            if ((labels[l >> 3] >> (l & 7)) & 1) t.labels[l >> 5] |= 1u << (l & 31);
    const int64_t blocks = ceil_div64((int64_t)oh * ow, NT);
    MTGS_REQUIRE(blocks < ((int64_t)1 << 31), MTGS_EINVAL, "%s: %lld workgroups", fn, (long long)blocks);
    frame_nearest_kernel<<<dim3((unsigned)blocks, (unsigned)n_planes), NT, 0, (hipStream_t)stream>>>(t, h, w, oh, ow, sy, sx);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}
