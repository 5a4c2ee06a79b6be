// present.hip -- the last stage of the viewer thread and of the offline render tool (include/mtgs_present.h): nerfstudio's
// apply_colormap / apply_depth_colormap, the split view, the concatenation of outputs, the uint8 conversion and the padding as
// ONE launch that writes the whole frame, after at most one launch that takes the minima and maxima the colormaps need; and the
// viewer's resized depth as one launch.  Nothing here reads the device from the host.
//
// mtgs_present_stats     workgroup b works for ONE source (its index against the running sum of the sources' workgroup counts,
//                        wave-uniform) and strides over it with the source's other workgroups; its (min, max), NaN if it met one,
//                        go to ws[panel][workgroup].  At most MTGS_PRESENT_STAT_BLOCKS workgroups per source.
// mtgs_present_compose   every workgroup first re-reduces the partials of each source in the same fixed order (<= 256 pairs per
//                        source out of L2: cheaper than a finish launch between the two) and derives the panels' constants into
//                        LDS; then one lane per 4 consecutive pixels of the flat uint8 frame -- 12 bytes, one 12-byte store when
//                        the frame's base is 4-byte aligned, whatever 3 * out_w is, because the groups tile the FLAT frame and not
//                        its rows; a group may span a row end or a panel seam, each of its pixels finds its own panel -- and byte
//                        stores for the last, partial group and for a misaligned base.  A float32 frame: one lane per pixel.
// The 3 KB colour table is read through the vector cache, not staged in LDS.  In LDS entry k would sit on banks 3k .. 3k + 2
// (mod 32; 12-byte stride): neighbouring entries never collide, 3 being coprime to 32, but the indices are data-dependent, so a
// busy image gathers at arbitrary multiples of 32 apart and a smooth one reads the same few entries, which a cache line serves as
// well.  Staging would cost every workgroup 768 loads and a barrier for the 3072 dwords it looks up, once per table -- and up to
// eight panels may each bring their own.  The table stays resident in each CU's cache for the life of the launch.
//
// Every arithmetic step rounds once, in the order the header states: contraction is off for this file (the build passes
// -ffp-contract=off as well), and fp32 division is hipcc's correctly rounded default.
#include <math.h>

#include "common.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int MAXP = MTGS_PRESENT_MAX_PANELS;
constexpr int TB = 256;                       // threads of every workgroup here
constexpr int STAT_MIN_ITEMS = 1024;          // a stats workgroup is worth starting for this many values
constexpr int MAX_STAT_BLOCKS = MTGS_PRESENT_STAT_BLOCKS;
static_assert(MAX_STAT_BLOCKS <= TB, "compose re-reduces one partial per thread");

struct Panel {
    const void *src;
    const float *acc, *lut;
    double near_plane, far_plane;
    float cscale, cmin;                        // (float)(colormap_max - colormap_min), (float)colormap_min
    int32_t kind, normalize, invert;
    int32_t stat_blocks;                       // 0: its extrema are not needed
    int32_t src_h, src_w, src_x0, y0, x0, h, w;
};

struct Table {
    Panel p[MAXP];
    int32_t stat_first[MAXP + 1];              // running sum of stat_blocks
    int32_t n;
};

struct Derived {                               // per panel, in LDS
    float nearf, inv, lo, den;
};

__device__ __forceinline__ float clip01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }   // NaN kept

// (min, max) over the workgroup, NaN if any thread met one; valid in every thread.  Fixed order: bitwise reproducible.
__device__ __forceinline__ void block_minmax(float &mn, float &mx, bool bad, float (*lds)[2]) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    }
    bad = __any(bad);
    const int wave = threadIdx.x >> 6;
    __syncthreads();                           // the previous use of lds is over
    if ((threadIdx.x & 63) == 0) {
        lds[wave][0] = bad ? NAN : mn;
        lds[wave][1] = bad ? NAN : mx;
    }
    __syncthreads();
    mn = lds[0][0], mx = lds[0][1];
    bad = mn != mn;
#pragma unroll
    for (int k = 1; k < TB / 64; ++k) {
        const float a = lds[k][0], b = lds[k][1];
        bad = bad || a != a;
        mn = fminf(mn, a), mx = fmaxf(mx, b);
    }
    if (bad) mn = mx = NAN;
}

__global__ __launch_bounds__(TB) void present_stats_kernel(Table t, float *__restrict__ ws) {
    __shared__ float lds[TB / 64][2];
    const int b = blockIdx.x;
    int j = 0;
#pragma unroll
    for (int k = 1; k < MAXP; ++k)
        if (k < t.n && b >= t.stat_first[k]) j = k;
    const int lb = b - t.stat_first[j], nb = t.p[j].stat_blocks;
    const float *__restrict__ src = (const float *)t.p[j].src;
    const int64_t n = (int64_t)t.p[j].src_h * t.p[j].src_w;
    float mn = INFINITY, mx = -INFINITY;
    bool bad = false;
#pragma unroll 4
    for (int64_t i = (int64_t)lb * TB + threadIdx.x; i < n; i += (int64_t)nb * TB) {
        const float v = src[i];
        bad = bad || v != v;
        mn = fminf(mn, v), mx = fmaxf(mx, v);
    }
    block_minmax(mn, mx, bad, lds);
    if (threadIdx.x == 0) {
        ws[((int64_t)j * MAX_STAT_BLOCKS + lb) * 2] = mn;
        ws[((int64_t)j * MAX_STAT_BLOCKS + lb) * 2 + 1] = mx;
    }
}

// the constants of every panel, into drv[]; all threads of the workgroup call it
__device__ __forceinline__ void derive(const Table &t, const float *__restrict__ ws, Derived *drv, float (*lds)[2], float (*ext)[2]) {
    for (int j = 0; j < t.n; ++j) {            // uniform
        const int nb = t.p[j].stat_blocks;
        if (nb == 0) continue;
        float mn = INFINITY, mx = -INFINITY;
        bool bad = false;
        if ((int)threadIdx.x < nb) {
            mn = ws[((int64_t)j * MAX_STAT_BLOCKS + threadIdx.x) * 2];
            mx = ws[((int64_t)j * MAX_STAT_BLOCKS + threadIdx.x) * 2 + 1];
            bad = mn != mn;
        }
        block_minmax(mn, mx, bad, lds);
        if (threadIdx.x == 0) ext[j][0] = mn, ext[j][1] = mx;
    }
    __syncthreads();
    if ((int)threadIdx.x < t.n) {
        const int j = threadIdx.x;
        const Panel &p = t.p[j];
        const float mn = p.stat_blocks ? ext[j][0] : 0.f, mx = p.stat_blocks ? ext[j][1] : 0.f;
        Derived d{0.f, 1.f, 0.f, 1.f};
        if (p.kind == MTGS_PRESENT_DEPTH) {
            const double nd = p.near_plane != p.near_plane ? (double)mn : p.near_plane;
            const double fd = p.far_plane != p.far_plane ? (double)mx : p.far_plane;
            const double D = (fd - nd) + 1e-10;
            d.nearf = (float)nd;
            d.inv = 1.0f / (float)D;
            if (p.normalize) {                 // every step so far is monotone: the extrema of the clipped values are the
                float a = clip01((mn - d.nearf) * d.inv), b = clip01((mx - d.nearf) * d.inv);   // clipped values of the extrema
                if (b < a) { const float s = a; a = b; b = s; }                                  // a negative scale: far < near
                d.lo = a;
                d.den = (b - a) + 1e-9f;
            }
        } else if (p.kind == MTGS_PRESENT_FLOAT && p.normalize) {
            d.lo = mn;
            d.den = (mx - mn) + 1e-9f;
        }
        drv[j] = d;
    }
    __syncthreads();
}

// the colour of output pixel (y, x): false where no panel covers it
__device__ __forceinline__ bool shade(const Table &t, const Derived *drv, int split_column, float s0, float s1, float s2, int y, int x,
                                      float &r, float &g, float &b) {
    int j = -1;
    for (int k = t.n - 1; k >= 0; --k)         // the FIRST panel of the table that covers the pixel
        if ((unsigned)(y - t.p[k].y0) < (unsigned)t.p[k].h && (unsigned)(x - t.p[k].x0) < (unsigned)t.p[k].w) j = k;
    if (j < 0) return false;
    if (x == split_column) {
        r = s0, g = s1, b = s2;
        return true;
    }
    const Panel &p = t.p[j];
    const int64_t at = (int64_t)(y - p.y0) * p.src_w + (p.src_x0 + (x - p.x0));
    if (p.kind == MTGS_PRESENT_RGB) {
        const float *s = (const float *)p.src + 3 * at;
        r = s[0], g = s[1], b = s[2];
        return true;
    }
    if (p.kind == MTGS_PRESENT_BOOL) {
        r = g = b = ((const uint8_t *)p.src)[at] ? 1.f : 0.f;
        return true;
    }
    const Derived d = drv[j];
    float v = ((const float *)p.src)[at];
    if (p.kind == MTGS_PRESENT_DEPTH) {
        v = v - d.nearf;
        v = v * d.inv;
        v = clip01(v);
    }
    if (p.normalize) {
        v = v - d.lo;
        v = v / d.den;
    }
    v = v * p.cscale;
    v = v + p.cmin;
    v = clip01(v);
    if (p.invert) v = 1.f - v;
    if (v != v) v = 0.f;
    if (p.lut) {
        int k = (int)(v * 255.f);
        k = k < 0 ? 0 : (k > 255 ? 255 : k);   // v is in [0, 1]: never taken, kept so that no value can index outside the table
        const float *c = p.lut + 3 * k;
        r = c[0], g = c[1], b = c[2];
    } else {
        r = g = b = v;
    }
    if (p.kind == MTGS_PRESENT_DEPTH && p.acc) {
        const float a = p.acc[at], oma = 1.f - a;
        r = r * a, g = g * a, b = b * a;
        r = r + oma, g = g + oma, b = b + oma;
    }
    return true;
}

__device__ __forceinline__ uint32_t quantise(float x, bool round) {
    x = x != x ? 0.f : clip01(x);
    x = x * 255.f;
    if (round) x = x + 0.5f;
    return (uint32_t)x;
}

struct alignas(4) Bytes12 {
    uint32_t a, b, c;
};

__global__ __launch_bounds__(TB) void present_compose_u8_kernel(Table t, const float *__restrict__ ws, int out_w, int64_t n_pixels,
                                                                int split_column, float s0, float s1, float s2, int round, int aligned,
                                                                uint8_t *__restrict__ out) {
    __shared__ float lds[TB / 64][2];
    __shared__ float ext[MAXP][2];
    __shared__ Derived drv[MAXP];
    derive(t, ws, drv, lds, ext);
    const int64_t p0 = ((int64_t)blockIdx.x * TB + threadIdx.x) * 4;
    if (p0 >= n_pixels) return;
    int y = (int)(p0 / out_w), x = (int)(p0 - (int64_t)y * out_w);
    const int count = n_pixels - p0 < 4 ? (int)(n_pixels - p0) : 4;
    uint32_t q[12];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float r = 0.f, g = 0.f, b = 0.f;
        if (i < count) shade(t, drv, split_column, s0, s1, s2, y, x, r, g, b);
        q[3 * i] = quantise(r, round), q[3 * i + 1] = quantise(g, round), q[3 * i + 2] = quantise(b, round);
        if (++x == out_w) x = 0, ++y;
    }
    uint8_t *o = out + p0 * 3;
    if (aligned && count == 4) {
        Bytes12 w;
        w.a = q[0] | q[1] << 8 | q[2] << 16 | q[3] << 24;
        w.b = q[4] | q[5] << 8 | q[6] << 16 | q[7] << 24;
        w.c = q[8] | q[9] << 8 | q[10] << 16 | q[11] << 24;
        *(Bytes12 *)o = w;
    } else {
#pragma unroll
        for (int i = 0; i < 12; ++i)
            if (i < 3 * count) o[i] = (uint8_t)q[i];
    }
}

__global__ __launch_bounds__(TB) void present_compose_f32_kernel(Table t, const float *__restrict__ ws, int out_w, int64_t n_pixels,
                                                                 int split_column, float s0, float s1, float s2, float *__restrict__ out) {
    __shared__ float lds[TB / 64][2];
    __shared__ float ext[MAXP][2];
    __shared__ Derived drv[MAXP];
    derive(t, ws, drv, lds, ext);
    const int64_t p0 = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (p0 >= n_pixels) return;
    const int y = (int)(p0 / out_w), x = (int)(p0 - (int64_t)y * out_w);
    float r = 0.f, g = 0.f, b = 0.f;
    shade(t, drv, split_column, s0, s1, s2, y, x, r, g, b);
    float *o = out + p0 * 3;
    o[0] = r, o[1] = g, o[2] = b;
}

__global__ __launch_bounds__(TB) void present_depth_resize_kernel(int in_h, int in_w, const float *__restrict__ src, int out_h, int out_w,
                                                                  float rh, float rw, float scale, float *__restrict__ dst) {
    const int64_t at = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (at >= (int64_t)out_h * out_w) return;
    const int oy = (int)(at / out_w), ox = (int)(at - (int64_t)oy * out_w);
    float sy = rh * ((float)oy + 0.5f) - 0.5f, sx = rw * ((float)ox + 0.5f) - 0.5f;
    sy = sy < 0.f ? 0.f : sy, sx = sx < 0.f ? 0.f : sx;
    int y0 = (int)sy, x0 = (int)sx;
    y0 = y0 > in_h - 1 ? in_h - 1 : y0, x0 = x0 > in_w - 1 ? in_w - 1 : x0;   // never taken for r = in / out; keeps every read inside
    const int y1 = y0 + (y0 < in_h - 1), x1 = x0 + (x0 < in_w - 1);
    const float h1 = sy - (float)y0, h0 = 1.f - h1, w1 = sx - (float)x0, w0 = 1.f - w1;
    const float a = src[(int64_t)y0 * in_w + x0], b = src[(int64_t)y0 * in_w + x1];
    const float c = src[(int64_t)y1 * in_w + x0], d = src[(int64_t)y1 * in_w + x1];
    const float v = h0 * (w0 * a + w1 * b) + h1 * (w0 * c + w1 * d);
    dst[at] = v * scale;
}

int stat_blocks_of(int64_t n) {
    const int64_t b = ceil_div64(n, STAT_MIN_ITEMS);
    return (int)(b < MAX_STAT_BLOCKS ? b : MAX_STAT_BLOCKS);
}

bool is_nan(double v) { return v != v; }

// The host checks of a panel table and its device form.  out_h < 0: the table alone (mtgs_present_stats), no frame to fit.
int make_table(const char *fn, int n_panels, const mtgs_present_panel *panels, int out_h, int out_w, Table &t) {
    MTGS_REQUIRE(n_panels >= 1 && n_panels <= MAXP, MTGS_EINVAL, "%s: n_panels outside [1, %d] (%d)", fn, MAXP, n_panels);
    MTGS_REQUIRE(panels != nullptr, MTGS_EINVAL, "%s: null pointer: panels", fn);
    t.n = n_panels;
    t.stat_first[0] = 0;
    for (int j = 0; j < n_panels; ++j) {
        const mtgs_present_panel &s = panels[j];
        Panel &p = t.p[j];
        MTGS_REQUIRE(s.kind >= MTGS_PRESENT_RGB && s.kind <= MTGS_PRESENT_BOOL, MTGS_EINVAL, "%s: panels[%d].kind outside [0, 3] (%d)", fn, j, s.kind);
        MTGS_REQUIRE(s.src != nullptr, MTGS_EINVAL, "%s: null pointer: panels[%d].src", fn, j);
        MTGS_REQUIRE(s.src_h >= 1 && s.src_w >= 1 && (int64_t)s.src_h * s.src_w < ((int64_t)1 << 31), MTGS_EINVAL,
                     "%s: panels[%d]: src_h, src_w must be >= 1 with src_h * src_w < 2^31 (%d, %d)", fn, j, s.src_h, s.src_w);
        const bool is_float = s.kind != MTGS_PRESENT_BOOL, mapped = s.kind == MTGS_PRESENT_FLOAT || s.kind == MTGS_PRESENT_DEPTH;
        MTGS_REQUIRE(!is_float || ((uintptr_t)s.src & 3) == 0, MTGS_EINVAL, "%s: panels[%d].src must be 4-byte aligned", fn, j);
        MTGS_REQUIRE((((uintptr_t)s.accumulation | (uintptr_t)s.lut) & 3) == 0, MTGS_EINVAL,
                     "%s: panels[%d].accumulation and .lut must be 4-byte aligned", fn, j);
        MTGS_REQUIRE(s.h >= 0 && s.w >= 0 && s.y0 >= 0 && s.x0 >= 0 && s.src_x0 >= 0, MTGS_EINVAL,
                     "%s: panels[%d]: negative rectangle (y0 %d, x0 %d, h %d, w %d, src_x0 %d)", fn, j, s.y0, s.x0, s.h, s.w, s.src_x0);
        MTGS_REQUIRE(s.h <= s.src_h && (int64_t)s.src_x0 + s.w <= s.src_w, MTGS_EINVAL,
                     "%s: panels[%d]: rectangle reads outside its source (h %d of %d rows, columns [%d, %lld) of %d)", fn, j, s.h, s.src_h,
                     s.src_x0, (long long)s.src_x0 + s.w, s.src_w);
        if (out_h >= 0)
            MTGS_REQUIRE((int64_t)s.y0 + s.h <= out_h && (int64_t)s.x0 + s.w <= out_w, MTGS_EINVAL,
                         "%s: panels[%d]: rectangle outside the %d x %d frame (rows [%d, %lld), columns [%d, %lld))", fn, j, out_h, out_w,
                         s.y0, (long long)s.y0 + s.h, s.x0, (long long)s.x0 + s.w);
        p.src = s.src;
        p.acc = s.kind == MTGS_PRESENT_DEPTH ? s.accumulation : nullptr;
        p.lut = mapped ? s.lut : nullptr;
        p.near_plane = s.near_plane, p.far_plane = s.far_plane;
        p.cscale = (float)(s.colormap_max - s.colormap_min), p.cmin = (float)s.colormap_min;
        p.kind = s.kind, p.normalize = mapped && s.normalize, p.invert = mapped && s.invert;
        p.src_h = s.src_h, p.src_w = s.src_w, p.src_x0 = s.src_x0, p.y0 = s.y0, p.x0 = s.x0, p.h = s.h, p.w = s.w;
        const bool needs = (s.kind == MTGS_PRESENT_DEPTH && (is_nan(s.near_plane) || is_nan(s.far_plane))) || p.normalize;
        p.stat_blocks = needs ? stat_blocks_of((int64_t)s.src_h * s.src_w) : 0;
        t.stat_first[j + 1] = t.stat_first[j] + p.stat_blocks;
    }
    return MTGS_OK;
}

constexpr size_t WS_BYTES = (size_t)MAXP * MAX_STAT_BLOCKS * 2 * sizeof(float);

int check_ws(const char *fn, const void *ws, size_t ws_bytes) {
    MTGS_REQUIRE(ws != nullptr, MTGS_EINVAL, "%s: null pointer: ws (a panel takes its extrema from the data)", fn);
    MTGS_REQUIRE(ws_bytes >= WS_BYTES, MTGS_EWORKSPACE, "%s: workspace %zu < %zu bytes", fn, ws_bytes, WS_BYTES);
    MTGS_REQUIRE(((uintptr_t)ws & 7) == 0, MTGS_EINVAL, "%s: workspace must be 8-byte aligned", fn);
    return MTGS_OK;
}

}  // namespace

extern "C" int mtgs_present_workspace_bytes(size_t *bytes, size_t *panel_bytes) {
    const char *fn = "mtgs_present_workspace_bytes";
    MTGS_REQUIRE(bytes != nullptr, MTGS_EINVAL, "%s: null pointer: bytes", fn);
    *bytes = WS_BYTES;
    if (panel_bytes) *panel_bytes = sizeof(mtgs_present_panel);
    return MTGS_OK;
}

extern "C" int mtgs_present_stats(int n_panels, const mtgs_present_panel *panels, void *ws, size_t ws_bytes, void *stream) {
    const char *fn = "mtgs_present_stats";
    Table t{};
    if (int rc = make_table(fn, n_panels, panels, -1, -1, t)) return rc;
    const int blocks = t.stat_first[n_panels];
    if (blocks == 0) return MTGS_OK;
    if (int rc = check_ws(fn, ws, ws_bytes)) return rc;
    present_stats_kernel<<<(unsigned)blocks, TB, 0, (hipStream_t)stream>>>(t, (float *)ws);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}

extern "C" int mtgs_present_compose(int n_panels, const mtgs_present_panel *panels, int out_h, int out_w, int split_column,
                                    const float *split_color, int format, void *out, const void *ws, size_t ws_bytes, void *stream) {
    const char *fn = "mtgs_present_compose";
    MTGS_REQUIRE(out_h >= 0 && out_w >= 0 && (int64_t)out_h * out_w < ((int64_t)1 << 31), MTGS_EINVAL,
                 "%s: out_h, out_w must be >= 0 with out_h * out_w < 2^31 (%d, %d)", fn, out_h, out_w);
    MTGS_REQUIRE(format >= MTGS_PRESENT_U8_TRUNCATE && format <= MTGS_PRESENT_F32, MTGS_EINVAL, "%s: format outside [0, 2] (%d)", fn, format);
    MTGS_REQUIRE(split_column >= -1 && split_column < (out_w > 0 ? out_w : 1), MTGS_EINVAL, "%s: split_column outside [-1, out_w) (%d)", fn, split_column);
    MTGS_REQUIRE(split_column < 0 || split_color != nullptr, MTGS_EINVAL, "%s: null pointer: split_color", fn);
    Table t{};
    if (int rc = make_table(fn, n_panels, panels, out_h, out_w, t)) return rc;
    const int64_t n_pixels = (int64_t)out_h * out_w;
    if (n_pixels == 0) return MTGS_OK;
    MTGS_REQUIRE(out != nullptr, MTGS_EINVAL, "%s: null pointer: out", fn);
    if (t.stat_first[n_panels])
        if (int rc = check_ws(fn, ws, ws_bytes)) return rc;
    const float s0 = split_column >= 0 ? split_color[0] : 0.f, s1 = split_column >= 0 ? split_color[1] : 0.f,
                s2 = split_column >= 0 ? split_color[2] : 0.f;
    hipStream_t st = (hipStream_t)stream;
    if (format == MTGS_PRESENT_F32) {
        MTGS_REQUIRE(((uintptr_t)out & 3) == 0, MTGS_EINVAL, "%s: a float32 out must be 4-byte aligned", fn);
        present_compose_f32_kernel<<<(unsigned)ceil_div64(n_pixels, TB), TB, 0, st>>>(t, (const float *)ws, out_w, n_pixels, split_column, s0,
                                                                                       s1, s2, (float *)out);
    } else {
        present_compose_u8_kernel<<<(unsigned)ceil_div64(n_pixels, 4 * TB), TB, 0, st>>>(
            t, (const float *)ws, out_w, n_pixels, split_column, s0, s1, s2, format == MTGS_PRESENT_U8_ROUND, ((uintptr_t)out & 3) == 0,
            (uint8_t *)out);
    }
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}

extern "C" int mtgs_present_depth_resize(int in_h, int in_w, const float *src, int out_h, int out_w, float scale, float *dst, void *stream) {
    const char *fn = "mtgs_present_depth_resize";
    MTGS_REQUIRE(in_h >= 0 && in_w >= 0 && (int64_t)in_h * in_w < ((int64_t)1 << 31), MTGS_EINVAL,
                 "%s: in_h, in_w must be >= 0 with in_h * in_w < 2^31 (%d, %d)", fn, in_h, in_w);
    MTGS_REQUIRE(out_h >= 0 && out_w >= 0 && (int64_t)out_h * out_w < ((int64_t)1 << 31), MTGS_EINVAL,
                 "%s: out_h, out_w must be >= 0 with out_h * out_w < 2^31 (%d, %d)", fn, out_h, out_w);
    const int64_t n = (int64_t)out_h * out_w;
    if (n == 0) return MTGS_OK;
    MTGS_REQUIRE(in_h >= 1 && in_w >= 1, MTGS_EINVAL, "%s: an empty source cannot fill a %d x %d output", fn, out_h, out_w);
    MTGS_REQUIRE(src != nullptr, MTGS_EINVAL, "%s: null pointer: src", fn);
    MTGS_REQUIRE(dst != nullptr, MTGS_EINVAL, "%s: null pointer: dst", fn);
    const float rh = (float)in_h / (float)out_h, rw = (float)in_w / (float)out_w;
    present_depth_resize_kernel<<<(unsigned)ceil_div64(n, TB), TB, 0, (hipStream_t)stream>>>(in_h, in_w, src, out_h, out_w, rh, rw, scale, dst);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}
