// brightness.hip -- camera brightness equalisation (include/mtgs_brightness.h states both rules in full; mtgs_amd.brightness):
// adjust_brightness and adjust_brightness_single_frame of nuplan_scripts/utils/nuplan_utils_custom.py:334-431.
//
// mtgs_brightness_adjust, one launch for C images: 8-bit RGB -> HSV in integers, V scaled in fp64 by a factor READ FROM DEVICE MEMORY,
// HSV -> RGB in fp32 ([RECALLED]: the project's definition, not a claim about OpenCV's bytes).  A byte-stream kernel: about 60 integer
// and fp32 operations per pixel against 6 bytes of traffic, so what bounds it is how the bytes are moved.  adjust_dword_kernel: a
// thread owns 4 pixels = 12 contiguous bytes = three dwords in, three dwords out (48 bytes = three 16-byte stores with a float32
// result); lane i of a wave touches bytes 12 i .. 12 i + 11, so a wave's three loads cover 768 contiguous bytes and every fetched
// byte is used.  adjust_strided_kernel: one pixel per thread, three byte loads through the four strides, three byte stores; it
// serves every layout the dword path cannot (padded rows, a base off a dword, negative strides) and the tail of an image whose
// pixel count is no multiple of 4.  Both call adjust_pixel, so they give the same bytes.  No LDS, no atomics.
//
// mtgs_brightness_estimate =
//   strips_kernel   grid (2 P, MTGS_BRIGHTNESS_STRIP_SLABS): the sum of max(r, g, b) over one row slab of one fallback strip, into ws;
//                   block (0, 0) also clears n, s1, s2 of every pair -- the strips run first so that no launch is spent on a clear
//   sample_kernel   one thread per point: the cameras in ascending order through lidar_sample.hpp (paint_kernel's body), V per seeing
//                   camera packed 8 to a register; per pair (n, s1, s2) packed into one uint64, summed over the wave by shuffles, over
//                   the workgroup through LDS, then three integer atomicAdds per pair and workgroup.  Integer sums: any order, same bits
//   solve_kernel    one thread: adds the slabs in slab order, runs the chain and NumPy's mean in the order the header states
//
// Compiled with -ffp-contract=off: the fp32 chain of HSV -> RGB and the fp64 projection round once per operation, as the NumPy
// restatement (tests/brightness_refs.py) does.
#include "common.hpp"
#include "lidar_sample.hpp"

namespace {

constexpr int TB = 256, SLABS = MTGS_BRIGHTNESS_STRIP_SLABS, MAXC = MTGS_BRIGHTNESS_MAX_CAMERAS, MAXP = MTGS_BRIGHTNESS_MAX_PAIRS;
static_assert(MAXC <= 16, "V of every camera is packed into two 64-bit registers");

// ---- the tables of RGB -> HSV, built at compile time ----------------------------------------------------------------------------
constexpr int rint_even(double q) {        // q >= 0; ties to even
    const long long fl = (long long)q;
    const double r = q - (double)fl;
    return (int)(r > 0.5 ? fl + 1 : (r < 0.5 ? fl : fl + (fl & 1)));
}
struct HsvTables {
    int sdiv[256], hdiv[256];
    constexpr HsvTables() : sdiv(), hdiv() {
        sdiv[0] = hdiv[0] = 0;
        for (int i = 1; i < 256; ++i) {
            sdiv[i] = rint_even((double)(255 << 12) / (double)i);
            hdiv[i] = rint_even((double)(180 << 12) / (6.0 * (double)i));
        }
    }
};
__device__ const HsvTables TABLES{};

// ---- one pixel: (c0, c1, c2) as stored -> the three result bytes packed c0 | c1 << 8 | c2 << 16 ------------------------------------
__device__ __forceinline__ uint32_t adjust_pixel(int c0, int c1, int c2, double factor, bool bgr) {
    const int r = bgr ? c2 : c0, g = c1, b = bgr ? c0 : c2;
    const int v = max(r, max(g, b)), vmin = min(r, min(g, b)), d = v - vmin;
    const int s = (d * TABLES.sdiv[v] + 2048) >> 12;
    int h = (v == r) ? g - b : (v == g) ? b - r + 2 * d : r - g + 4 * d;
    h = (h * TABLES.hdiv[d] + 2048) >> 12;
    if (h < 0) h += 180;
    // fmax and fmin return the other operand for a NaN: a NaN product becomes 0
    const int v2 = (int)fmin(fmax((double)v * factor, 0.0), 255.0);
    const float vf = (float)v2 * (1.0f / 255.0f);
    float fr = vf, fg = vf, fb = vf;
    if (s != 0) {
        const float hf = (float)h * (float)(6.0 / 180.0), sf = (float)s * (1.0f / 255.0f);
        const float fl = floorf(hf), f = hf - fl;
        const int sector = (int)fl;
        const float p = vf * (1.0f - sf), q = vf * (1.0f - sf * f), t = vf * (1.0f - sf * (1.0f - f));
        fb = sector == 0 || sector == 1 ? p : (sector == 2 ? t : (sector == 5 ? q : vf));
        fg = sector == 0 ? t : (sector == 1 || sector == 2 ? vf : (sector == 3 ? q : p));
        fr = sector == 0 || sector == 5 ? vf : (sector == 1 ? q : (sector == 4 ? t : p));
    }
    const int ob = (int)fminf(fmaxf(rintf(fb * 255.0f), 0.0f), 255.0f);
    const int og = (int)fminf(fmaxf(rintf(fg * 255.0f), 0.0f), 255.0f);
    const int orr = (int)fminf(fmaxf(rintf(fr * 255.0f), 0.0f), 255.0f);
    const int o0 = bgr ? ob : orr, o2 = bgr ? orr : ob;
    return (uint32_t)o0 | ((uint32_t)og << 8) | ((uint32_t)o2 << 16);
}

__device__ __forceinline__ float unit(uint32_t byte) { return __fdiv_rn((float)byte, 255.0f); }

struct AdjustArgs {
    const uint8_t *src;
    int64_t s_img, s_row, s_col, s_ch;      // bytes
    const double *factors;
    int64_t f_stride;
    void *dst;
    int64_t n_pix;                          // h * w
    int w, bgr, out_float;
};

// pixel i of image c through the strides, byte by byte
__device__ __forceinline__ void adjust_one(const AdjustArgs &a, int c, int64_t i, double factor) {
    const uint8_t *s = a.src + c * a.s_img + (i / a.w) * a.s_row + (i % a.w) * a.s_col;
    const uint32_t o = adjust_pixel(s[0], s[a.s_ch], s[2 * a.s_ch], factor, a.bgr != 0);
    const int64_t at = ((int64_t)c * a.n_pix + i) * 3;
    if (a.out_float) {
        float *d = (float *)a.dst + at;
        d[0] = unit(o & 255u); d[1] = unit((o >> 8) & 255u); d[2] = unit(o >> 16);
    } else {
        uint8_t *d = (uint8_t *)a.dst + at;
        d[0] = (uint8_t)(o & 255u); d[1] = (uint8_t)((o >> 8) & 255u); d[2] = (uint8_t)(o >> 16);
    }
}

// every layout: one pixel of image blockIdx.y per thread
__global__ __launch_bounds__(TB) void adjust_strided_kernel(AdjustArgs a) {
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= a.n_pix) return;
    adjust_one(a, (int)blockIdx.y, i, a.factors[(int64_t)blockIdx.y * a.f_stride]);
}

// group gidx = pixels 4 gidx .. 4 gidx + 3 of image blockIdx.y = 3 dwords per thread; the launcher has checked contiguity and
// alignment.  The thread behind the last whole group takes the n_pix % 4 pixels that are left, byte by byte.
template <bool OUT_FLOAT>
__global__ __launch_bounds__(TB) void adjust_dword_kernel(AdjustArgs a) {
    const int64_t gidx = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (gidx > a.n_pix / 4) return;
    const int c = (int)blockIdx.y;
    const double factor = a.factors[c * a.f_stride];
    if (gidx == a.n_pix / 4) {
        for (int64_t i = gidx * 4; i < a.n_pix; ++i) adjust_one(a, c, i, factor);
        return;
    }
    const bool bgr = a.bgr != 0;
    const uint32_t *s = (const uint32_t *)(a.src + c * a.s_img) + gidx * 3;
    const uint32_t d0 = s[0], d1 = s[1], d2 = s[2];
    const uint32_t p0 = adjust_pixel(d0 & 255u, (d0 >> 8) & 255u, (d0 >> 16) & 255u, factor, bgr);
    const uint32_t p1 = adjust_pixel(d0 >> 24, d1 & 255u, (d1 >> 8) & 255u, factor, bgr);
    const uint32_t p2 = adjust_pixel((d1 >> 16) & 255u, d1 >> 24, d2 & 255u, factor, bgr);
    const uint32_t p3 = adjust_pixel((d2 >> 8) & 255u, (d2 >> 16) & 255u, d2 >> 24, factor, bgr);
    const int64_t at = ((int64_t)c * a.n_pix + gidx * 4) * 3;            // a multiple of 4: the launcher's condition
    if (OUT_FLOAT) {
        float4 *d = (float4 *)((float *)a.dst + at);
        d[0] = make_float4(unit(p0 & 255u), unit((p0 >> 8) & 255u), unit(p0 >> 16), unit(p1 & 255u));
        d[1] = make_float4(unit((p1 >> 8) & 255u), unit(p1 >> 16), unit(p2 & 255u), unit((p2 >> 8) & 255u));
        d[2] = make_float4(unit(p2 >> 16), unit(p3 & 255u), unit((p3 >> 8) & 255u), unit(p3 >> 16));
    } else {
        uint32_t *d = (uint32_t *)((uint8_t *)a.dst + at);
        d[0] = p0 | (p1 << 24);
        d[1] = (p1 >> 8) | (p2 << 16);
        d[2] = (p2 >> 16) | (p3 << 8);
    }
}

// ---- the estimate -----------------------------------------------------------------------------------------------------------------
struct Pair {
    int cam1, cam2, side;
    bool ok;
};
// a pair of the device table; one that names a camera outside [0, C) or the same camera twice is skipped everywhere
__device__ __forceinline__ Pair load_pair(const int32_t *__restrict__ pairs, int p, int C) {
    Pair r{pairs[3 * p], pairs[3 * p + 1], pairs[3 * p + 2], false};
    r.ok = r.cam1 >= 0 && r.cam1 < C && r.cam2 >= 0 && r.cam2 < C && r.cam1 != r.cam2 && (r.side == 0 || r.side == 1);
    return r;
}

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, o, 64);
    return v;
}

__global__ __launch_bounds__(TB) void strips_kernel(int C, int h, int w, const uint8_t *__restrict__ images, int P,
                                                    const int32_t *__restrict__ pairs, int strip, uint64_t *__restrict__ partial,
                                                    int64_t *__restrict__ stats) {
    __shared__ uint64_t lds[TB / MTGS_WAVE];
    if (blockIdx.x == 0 && blockIdx.y == 0) {
        for (int i = threadIdx.x; i < 3 * P; i += TB) stats[(i / 3) * 5 + i % 3] = 0;
    }
    const int p = (int)blockIdx.x >> 1, second = (int)blockIdx.x & 1;
    const Pair pr = load_pair(pairs, p, C);
    uint64_t sum = 0;
    if (pr.ok) {
        const int cam = second ? pr.cam2 : pr.cam1;
        const bool left = (pr.side == 0) == (second == 0);
        const int cols = min(strip, w), col0 = left ? 0 : w - cols;
        const int per = (int)ceil_div64(h, SLABS), r0 = min((int)blockIdx.y * per, h), r1 = min(r0 + per, h);
        const uint8_t *img = images + (int64_t)cam * h * w * 3;
        const int64_t n = (int64_t)(r1 - r0) * cols;
        for (int64_t i = threadIdx.x; i < n; i += TB) {
            const uint8_t *t = img + ((int64_t)(r0 + i / cols) * w + col0 + i % cols) * 3;
            sum += (uint64_t)max((int)t[0], max((int)t[1], (int)t[2]));
        }
    }
    sum = wave_sum_u64(sum);
    if (lane_id() == 0) lds[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) partial[(int64_t)blockIdx.x * SLABS + blockIdx.y] = ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

template <class T>
__global__ __launch_bounds__(TB) void sample_kernel(int32_t N, const T *__restrict__ points, int64_t stride, int C,
                                                    const double *__restrict__ mats, int h, int w, const uint8_t *__restrict__ images,
                                                    int P, const int32_t *__restrict__ pairs, int64_t *__restrict__ stats) {
    __shared__ uint64_t lds[TB / MTGS_WAVE][MAXP];
    const int64_t t = (int64_t)blockIdx.x * TB + threadIdx.x;
    uint32_t seen = 0;
    uint64_t vlo = 0, vhi = 0;                                  // V of camera c in byte c of (vlo, vhi)
    if (t < N) {
        double x[3];
        load_point(points, stride, t, x);
        const int64_t plane = (int64_t)h * w;
        for (int c = 0; c < C; ++c) {
            double ix, iy;
            if (!lidar_see(mats + 12 * c, x, h, w, ix, iy)) continue;
            const LidarTaps taps = lidar_taps(images + c * plane * 3, h, w, ix, iy);
            int V = 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) V = max(V, (int)(lidar_tap_value(taps, k) * 255.0) & 255);
            seen |= 1u << c;
            if (c < 8) vlo |= (uint64_t)V << (8 * c);
            else vhi |= (uint64_t)V << (8 * (c - 8));
        }
    }
    const int wave = (int)threadIdx.x >> 6;
    for (int p = 0; p < P; ++p) {                               // wave-uniform trip count and pair
        const Pair pr = load_pair(pairs, p, C);
        uint64_t packed = 0;                                    // n in bits 0 .. 15, s1 in 16 .. 39, s2 in 40 .. 63: sums of <= 256 lanes
        if (pr.ok && ((seen >> pr.cam1) & (seen >> pr.cam2) & 1u)) {
            const uint64_t v1 = ((pr.cam1 < 8 ? vlo : vhi) >> (8 * (pr.cam1 & 7))) & 255u;
            const uint64_t v2 = ((pr.cam2 < 8 ? vlo : vhi) >> (8 * (pr.cam2 & 7))) & 255u;
            packed = 1u | (v1 << 16) | (v2 << 40);
        }
        packed = wave_sum_u64(packed);
        if (lane_id() == 0) lds[wave][p] = packed;
    }
    __syncthreads();
    for (int p = threadIdx.x; p < P; p += TB) {
        const uint64_t n = (lds[0][p] & 0xffffu) + (lds[1][p] & 0xffffu) + (lds[2][p] & 0xffffu) + (lds[3][p] & 0xffffu);
        if (n == 0) continue;
        uint64_t s1 = 0, s2 = 0;
#pragma unroll
        for (int k = 0; k < TB / MTGS_WAVE; ++k) {
            s1 += (lds[k][p] >> 16) & 0xffffffu;
            s2 += lds[k][p] >> 40;
        }
        unsigned long long *row = (unsigned long long *)(stats + 5 * p);
        atomicAdd(row, (unsigned long long)n);
        atomicAdd(row + 1, (unsigned long long)s1);
        atomicAdd(row + 2, (unsigned long long)s2);
    }
}

// np.mean's sum of a contiguous float64 array of n <= 128 values (NumPy's pairwise_sum below its block size)
__device__ double numpy_sum(const double *a, int n) {
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) res = res + a[i];
        return res;
    }
    double r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    int i = 8;
    for (; i + 8 <= n; i += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = r[j] + a[i + j];
    }
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res = res + a[i];
    return res;
}

__global__ void solve_kernel(int C, int h, int w, int P, const int32_t *__restrict__ pairs, int strip, int min_overlap,
                             const uint64_t *__restrict__ partial, int64_t *__restrict__ stats, double *__restrict__ factors) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    for (int c = 0; c < C; ++c) factors[c] = 1.0;
    uint32_t has = 1u;
    const double n_strip = (double)((int64_t)h * min(strip, w));
    for (int p = 0; p < P; ++p) {
        uint64_t strip1 = 0, strip2 = 0;
        for (int k = 0; k < SLABS; ++k) {
            strip1 += partial[(int64_t)(2 * p) * SLABS + k];
            strip2 += partial[(int64_t)(2 * p + 1) * SLABS + k];
        }
        stats[5 * p + 3] = (int64_t)strip1;
        stats[5 * p + 4] = (int64_t)strip2;
        const Pair pr = load_pair(pairs, p, C);
        if (!pr.ok) continue;
        const int64_t n = stats[5 * p];
        const bool overlap = n >= (int64_t)min_overlap;
        const double a = overlap ? (double)stats[5 * p + 1] : (double)strip1, b = overlap ? (double)stats[5 * p + 2] : (double)strip2;
        const double cnt = overlap ? (double)n : n_strip;
        const double v_ratio = (a / cnt) / (b / cnt);
        const double base = ((has >> pr.cam1) & 1u) ? factors[pr.cam1] : 1.0;
        const double ratio = base * v_ratio;
        factors[pr.cam2] = ((has >> pr.cam2) & 1u) ? (factors[pr.cam2] + ratio) / 2.0 : ratio;
        has |= 1u << pr.cam2;
    }
    const double mean = numpy_sum(factors, C) / (double)C;
    for (int c = 0; c < C; ++c) factors[c] = factors[c] / mean;
}

#define BRIGHTNESS_HW(fn, h, w)                                                                                                \
    MTGS_REQUIRE(h >= 1 && w >= 1 && (int64_t)h * w < ((int64_t)1 << 31), MTGS_EINVAL, "%s: h and w must be >= 1 and h * w < 2^31 (%d x %d)", \
                 fn, h, w)

size_t estimate_ws_bytes(int P) { return (size_t)2 * P * SLABS * sizeof(uint64_t); }

}  // namespace


extern "C" int mtgs_brightness_adjust(int C, int h, int w, const uint8_t *src, int64_t image_stride, int64_t row_stride,
                                      int64_t col_stride, int64_t channel_stride, const double *factors, int64_t factor_stride, int bgr,
                                      int out_float, int force_strided, void *dst, void *stream) {
    const char *fn = "mtgs_brightness_adjust";
    MTGS_REQUIRE(C >= 1 && C <= MTGS_BRIGHTNESS_MAX_IMAGES, MTGS_EINVAL, "%s: C outside [1, %d] (%d)", fn, MTGS_BRIGHTNESS_MAX_IMAGES, C);
    BRIGHTNESS_HW(fn, h, w);
    MTGS_NONNULL(fn, src); MTGS_NONNULL(fn, factors); MTGS_NONNULL(fn, dst);
    MTGS_REQUIRE(((uintptr_t)factors & 7) == 0, MTGS_EINVAL, "%s: factors must be 8-byte aligned", fn);
    MTGS_REQUIRE(factor_stride == 0 || factor_stride == 1, MTGS_EINVAL, "%s: factor_stride must be 0 or 1 (%lld)", fn, (long long)factor_stride);
    MTGS_REQUIRE(!out_float || ((uintptr_t)dst & 3) == 0, MTGS_EINVAL, "%s: a float32 dst must be 4-byte aligned", fn);
    hipStream_t st = (hipStream_t)stream;
    AdjustArgs a{src, image_stride, row_stride, col_stride, channel_stride, factors, factor_stride, dst, (int64_t)h * w, w, bgr, out_float};
    const uintptr_t dst_align = out_float ? 15 : 3;
    const bool dword = !force_strided && channel_stride == 1 && col_stride == 3 && (h == 1 || row_stride == (int64_t)3 * w) &&
                       ((uintptr_t)src & 3) == 0 && ((uintptr_t)dst & dst_align) == 0 &&
                       (C == 1 || ((image_stride & 3) == 0 && (a.n_pix & 3) == 0));
    if (dword) {
        const dim3 grid((unsigned)ceil_div64(ceil_div64(a.n_pix, 4), TB), (unsigned)C);
        if (out_float) adjust_dword_kernel<true><<<grid, TB, 0, st>>>(a);
        else adjust_dword_kernel<false><<<grid, TB, 0, st>>>(a);
    } else {
        adjust_strided_kernel<<<dim3((unsigned)ceil_div64(a.n_pix, TB), (unsigned)C), TB, 0, st>>>(a);
    }
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}

extern "C" int mtgs_brightness_estimate_workspace_bytes(int P, size_t *bytes) {
    const char *fn = "mtgs_brightness_estimate_workspace_bytes";
    MTGS_REQUIRE(P >= 1 && P <= MAXP, MTGS_EINVAL, "%s: P outside [1, %d] (%d)", fn, MAXP, P);
    MTGS_NONNULL(fn, bytes);
    *bytes = estimate_ws_bytes(P);
    return MTGS_OK;
}

extern "C" int mtgs_brightness_estimate(int64_t N, const void *points, int points_f64, int64_t row_stride, int C,
                                        const double *lidar2imgs, int h, int w, const uint8_t *images, int P, const int32_t *pairs,
                                        int strip, int min_overlap, double *factors, int64_t *stats, void *ws, size_t ws_bytes,
                                        void *stream) {
    const char *fn = "mtgs_brightness_estimate";
    MTGS_COUNT31(fn, N);
    BRIGHTNESS_HW(fn, h, w);
    MTGS_REQUIRE(C >= 1 && C <= MAXC, MTGS_EINVAL, "%s: C outside [1, %d] (%d)", fn, MAXC, C);
    MTGS_REQUIRE(P >= 1 && P <= MAXP, MTGS_EINVAL, "%s: P outside [1, %d] (%d)", fn, MAXP, P);
    MTGS_REQUIRE(strip >= 1, MTGS_EINVAL, "%s: strip < 1 (%d)", fn, strip);
    MTGS_REQUIRE(min_overlap >= 0, MTGS_EINVAL, "%s: min_overlap < 0 (%d)", fn, min_overlap);
    MTGS_NONNULL(fn, images); MTGS_NONNULL(fn, pairs); MTGS_NONNULL(fn, factors); MTGS_NONNULL(fn, stats); MTGS_NONNULL(fn, ws);
    MTGS_REQUIRE(ws_bytes >= estimate_ws_bytes(P), MTGS_EWORKSPACE, "%s: workspace %zu < %zu bytes", fn, ws_bytes, estimate_ws_bytes(P));
    MTGS_REQUIRE((((uintptr_t)ws | (uintptr_t)stats | (uintptr_t)factors) & 7) == 0, MTGS_EINVAL,
                 "%s: workspace, stats and factors must be 8-byte aligned", fn);
    if (N > 0) {
        MTGS_NONNULL(fn, points); MTGS_NONNULL(fn, lidar2imgs);
        MTGS_REQUIRE(row_stride >= 3, MTGS_EINVAL, "%s: row_stride < 3 (%lld)", fn, (long long)row_stride);
    }
    hipStream_t st = (hipStream_t)stream;
    uint64_t *partial = (uint64_t *)ws;
    strips_kernel<<<dim3((unsigned)(2 * P), SLABS), TB, 0, st>>>(C, h, w, images, P, pairs, strip, partial, stats);
    MTGS_CHECK_LAUNCH(fn);
    if (N > 0) {
        const unsigned blocks = (unsigned)ceil_div64(N, TB);
        if (points_f64)
            sample_kernel<double><<<blocks, TB, 0, st>>>((int32_t)N, (const double *)points, row_stride, C, lidar2imgs, h, w, images, P, pairs, stats);
        else
            sample_kernel<float><<<blocks, TB, 0, st>>>((int32_t)N, (const float *)points, row_stride, C, lidar2imgs, h, w, images, P, pairs, stats);
        MTGS_CHECK_LAUNCH(fn);
    }
    solve_kernel<<<1, MTGS_WAVE, 0, st>>>(C, h, w, P, pairs, strip, min_overlap, partial, stats, factors);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}
