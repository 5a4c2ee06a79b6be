// lpips.hip -- the LPIPS metric with the AlexNet backbone (include/mtgs_lpips.h): five convolutions as implicit GEMMs on exact-f32
// MFMA (v_mfma_f32_32x32x2_f32), two max-pools, and a fused tail (channel norms, weighted squared difference, spatial mean).
//
// Activations are NHWC, both images in one array [2, h, w, C], so a layer is ONE launch with M = 2 * oh * ow rows.
//   lpips_conv      the tile of mfma_f32_tile.hpp, 128 (M) x 64 (N) per workgroup, the chain never restarted; cout is a multiple of 32
//                   only, so the last column tile may be half empty.  The last k-step is zero-filled beyond K (K = 363 for layer 1).
//                   Three loaders for A: VEC (cin % 32 == 0: a K-step lies inside one tap, 16-byte loads), SCALAR (any cin), FIRST
//                   (the two [H, W, 3] images and the mask, input transform applied on load; padding taps stay 0).
//   lpips_maxpool   3x3 stride 2, four channels per thread.
//   lpips_distance  one wave per tap pixel: both feature vectors read once into registers, the two sums of squares and the weighted
//                   squared difference by butterfly sums (every lane the same total), pixels walked in a fixed order, one partial
//                   per workgroup.
//   lpips_finish    one workgroup: the partials of each layer in a fixed tree, / pixel count, summed layer by layer.
#include <math.h>

#include "block_reduce.hpp"
#include "common.hpp"
#include "mfma_f32_tile.hpp"

namespace {

constexpr int DIST_BLOCKS = 256;          // partials per layer
constexpr int DIST_MAX_Q = 8;             // channels per lane held in registers: cout <= 512
constexpr int N_LAYERS = 5;

enum { LOAD_VEC = 0, LOAD_SCALAR = 1, LOAD_FIRST = 2 };

struct Conv {
    const float *in;        // [n, h, w, cin]; FIRST: unused
    const float *img0, *img1;   // FIRST: [h, w, 3] each
    const uint8_t *mask;    // FIRST: [h, w] or NULL
    const float *wt;        // [K][cout]
    const float *bias;      // [cout]
    float *out;             // [n, oh, ow, cout]
    int n, h, w, cin, cout, kh, kw, stride, pad, oh, ow, M, K, relu, normalize;     // n images: M = n * oh * ow
};

__device__ __forceinline__ float first_value(const Conv &c, const float *img, int iy, int ix, int ch) {
    const float shift = ch == 0 ? -.030f : (ch == 1 ? -.088f : -.188f);
    const float scale = ch == 0 ? .458f : (ch == 1 ? .449f : .450f);
    const size_t p = (size_t)iy * c.w + ix;
    float v = img[p * 3 + ch];
    if (c.mask != nullptr && c.mask[p] == 0) v = 0.f;
    if (c.normalize) v = 2.f * v - 1.f;
    return (v - shift) / scale;
}

template <int MODE>
__global__ __launch_bounds__(TB) void lpips_conv_kernel(Conv c) {
    const int kq = tile_a_kq();            // A loader: the window origin of this thread's rows, then one of three fetches
    int oy0[RA], ox0[RA], img[RA];
    bool rowok[RA];
#pragma unroll
    for (int r = 0; r < RA; ++r) {
        const int m = blockIdx.x * BM + tile_a_row(r);
        rowok[r] = m < c.M;
        const int mm = rowok[r] ? m : 0;
        const int per = c.oh * c.ow;
        img[r] = mm / per;
        const int q = mm - img[r] * per;
        const int oy = q / c.ow;
        oy0[r] = oy * c.stride - c.pad;
        ox0[r] = (q - oy * c.ow) * c.stride - c.pad;
    }
    auto fetch_a = [&](int k0, float4 (&ra)[RA]) {
        if (MODE == LOAD_VEC) {
            const int tap = k0 / c.cin, ch = k0 - tap * c.cin + 4 * kq;
            const int ky = tap / c.kw, kx = tap - ky * c.kw;
#pragma unroll
            for (int r = 0; r < RA; ++r) {
                const int iy = oy0[r] + ky, ix = ox0[r] + kx;
                ra[r] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (rowok[r] && iy >= 0 && iy < c.h && ix >= 0 && ix < c.w)
                    ra[r] = *reinterpret_cast<const float4 *>(c.in + (((size_t)img[r] * c.h + iy) * c.w + ix) * c.cin + ch);
            }
        } else {
            float va[RA][4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = k0 + 4 * kq + j;
                const int tap = k / c.cin, ch = k - tap * c.cin;
                const int ky = tap / c.kw, kx = tap - ky * c.kw;
#pragma unroll
                for (int r = 0; r < RA; ++r) {
                    const int iy = oy0[r] + ky, ix = ox0[r] + kx;
                    float v = 0.f;
                    if (k < c.K && rowok[r] && iy >= 0 && iy < c.h && ix >= 0 && ix < c.w) {
                        if (MODE == LOAD_FIRST) v = first_value(c, img[r] ? c.img1 : c.img0, iy, ix, ch);
                        else v = c.in[(((size_t)img[r] * c.h + iy) * c.w + ix) * c.cin + ch];
                    }
                    va[r][j] = v;
                }
            }
#pragma unroll
            for (int r = 0; r < RA; ++r) ra[r] = make_float4(va[r][0], va[r][1], va[r][2], va[r][3]);
        }
    };
    // + bias, ReLU
    mfma_f32_tile<2, 0, true>(c.wt, c.M, c.cout, c.K, fetch_a, [&](int n) {
        const float b = c.bias[n];
        return [&c, n, b](int m, float x) {
            x += b;
            if (c.relu) x = x > 0.f ? x : 0.f;
            c.out[(size_t)m * c.cout + n] = x;
        };
    });
}

__global__ __launch_bounds__(TB) void lpips_repack_kernel(int cout, int cin, int kh, int kw, const float *__restrict__ w,
                                                          float *__restrict__ packed, int n) {
    const int e = blockIdx.x * TB + threadIdx.x;
    if (e >= n) return;
    const int o = e % cout, k = e / cout;
    const int ch = k % cin, tap = k / cin;
    const int kx = tap % kw, ky = tap / kw;
    packed[e] = w[(((size_t)o * cin + ch) * kh + ky) * kw + kx];
}

__global__ __launch_bounds__(TB) void lpips_maxpool_kernel(int h, int w, int c4, int oh, int ow, const float4 *__restrict__ in,
                                                           float4 *__restrict__ out, int n) {
    const int e = blockIdx.x * TB + threadIdx.x;
    if (e >= n) return;
    const int ch = e % c4;
    int q = e / c4;
    const int ox = q % ow;
    q /= ow;
    const int oy = q % oh, img = q / oh;
    float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {      // 2 oy + 2 <= h - 1 and 2 ox + 2 <= w - 1 by the floor in oh, ow
            const float4 v = in[(((size_t)img * h + 2 * oy + dy) * w + 2 * ox + dx) * c4 + ch];
            m.x = v.x > m.x ? v.x : m.x; m.y = v.y > m.y ? v.y : m.y; m.z = v.z > m.z ? v.z : m.z; m.w = v.w > m.w ? v.w : m.w;
        }
    out[e] = m;
}

// feat [2, P, C]; partials[blockIdx.x] = sum over this workgroup's pixels of sum_c lin[c] (u0 - u1)^2
__global__ __launch_bounds__(TB) void lpips_distance_kernel(int P, int C, int norm, const float *__restrict__ feat,
                                                            const float *__restrict__ lin, float *__restrict__ partials) {
    __shared__ float s_part[TB / 64];
    const int wv = threadIdx.x >> 6, l = threadIdx.x & 63;
    float wl[DIST_MAX_Q];
#pragma unroll
    for (int q = 0; q < DIST_MAX_Q; ++q) wl[q] = l + 64 * q < C ? lin[l + 64 * q] : 0.f;
    float total = 0.f;
    for (int p = blockIdx.x * (TB / 64) + wv; p < P; p += gridDim.x * (TB / 64)) {     // p is the same for the whole wave
        const float *f0 = feat + (size_t)p * C, *f1 = feat + ((size_t)P + p) * C;
        float a[DIST_MAX_Q], b[DIST_MAX_Q], s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int q = 0; q < DIST_MAX_Q; ++q) {
            const bool ok = l + 64 * q < C;
            a[q] = ok ? f0[l + 64 * q] : 0.f;
            b[q] = ok ? f1[l + 64 * q] : 0.f;
            s0 += a[q] * a[q];
            s1 += b[q] * b[q];
        }
        s0 = wave_sum_all(s0);
        s1 = wave_sum_all(s1);
        const float na = norm == MTGS_LPIPS_NORM_SQRT_EPS_INSIDE ? sqrtf(s0 + 1e-8f) : sqrtf(s0) + 1e-10f;
        const float nb = norm == MTGS_LPIPS_NORM_SQRT_EPS_INSIDE ? sqrtf(s1 + 1e-8f) : sqrtf(s1) + 1e-10f;
        float d = 0.f;
#pragma unroll
        for (int q = 0; q < DIST_MAX_Q; ++q) {
            const float e = a[q] / na - b[q] / nb;
            d += wl[q] * (e * e);
        }
        total += wave_sum_all(d);
    }
    if (l == 0) s_part[wv] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int k = 0; k < TB / 64; ++k) s += s_part[k];
        partials[blockIdx.x] = s;
    }
}

struct Finish {
    int blocks[N_LAYERS], pixels[N_LAYERS];
};

__global__ __launch_bounds__(DIST_BLOCKS) void lpips_finish_kernel(Finish f, const float *__restrict__ partials, float *__restrict__ out) {
    __shared__ float s[DIST_BLOCKS];
    const int t = threadIdx.x;
    float total = 0.f;
    for (int layer = 0; layer < N_LAYERS; ++layer) {
        const float sum = block_tree_sum_f32<DIST_BLOCKS>(t < f.blocks[layer] ? partials[layer * DIST_BLOCKS + t] : 0.f, s);
        if (t == 0) total += sum / (float)f.pixels[layer];
        __syncthreads();
    }
    if (t == 0) out[0] = total;
}

// ---- host -------------------------------------------------------------------------------------------------------------------
struct Layer {
    int cin, cout, k, stride, pad, pool_before;
};
constexpr Layer LAYERS[N_LAYERS] = {{3, 64, 11, 4, 2, 0}, {64, 192, 5, 1, 2, 1}, {192, 384, 3, 1, 1, 1}, {384, 256, 3, 1, 1, 0}, {256, 256, 3, 1, 1, 0}};

constexpr int64_t LIMIT = (int64_t)1 << 31;

int conv_out(int n, int k, int stride, int pad) { return n + 2 * pad < k ? 0 : (n + 2 * pad - k) / stride + 1; }
int pool_out(int n) { return n < 3 ? 0 : (n - 3) / 2 + 1; }

int launch_conv(const char *fn, int mode, Conv c, hipStream_t st) {
    MTGS_REQUIRE(c.n > 0 && c.h > 0 && c.w > 0 && c.cin > 0 && c.cout > 0 && c.kh > 0 && c.kw > 0 && c.stride > 0 && c.pad >= 0, MTGS_EINVAL,
                 "%s: sizes must be positive (n %d, h %d, w %d, cin %d, cout %d, kernel %d x %d, stride %d, pad %d)", fn, c.n, c.h, c.w, c.cin,
                 c.cout, c.kh, c.kw, c.stride, c.pad);
    MTGS_REQUIRE(c.cout % 32 == 0, MTGS_EUNSUPPORTED, "%s: cout = %d is not a multiple of 32", fn, c.cout);
    MTGS_REQUIRE(c.wt && c.bias && c.out, MTGS_EINVAL, "%s: null pointer: packed, bias or out", fn);
    MTGS_REQUIRE(((uintptr_t)c.wt & 15) == 0, MTGS_EINVAL, "%s: packed weights must be 16-byte aligned", fn);
    c.oh = conv_out(c.h, c.kh, c.stride, c.pad);
    c.ow = conv_out(c.w, c.kw, c.stride, c.pad);
    MTGS_REQUIRE(c.oh > 0 && c.ow > 0, MTGS_EINVAL, "%s: a %d x %d input leaves no output for a %d x %d kernel with pad %d", fn, c.h, c.w,
                 c.kh, c.kw, c.pad);
    const int64_t M = (int64_t)c.n * c.oh * c.ow, K = (int64_t)c.kh * c.kw * c.cin;
    MTGS_REQUIRE(M * c.cout < LIMIT && (int64_t)c.n * c.h * c.w * c.cin < LIMIT && K * c.cout < LIMIT, MTGS_EUNSUPPORTED,
                 "%s: an array of 2^31 elements or more", fn);
    c.M = (int)M;
    c.K = (int)K;
    if (mode == LOAD_SCALAR && c.cin % BK == 0 && ((uintptr_t)c.in & 15) == 0) mode = LOAD_VEC;
    const dim3 grid((unsigned)ceil_div64(M, BM), (unsigned)ceil_div64(c.cout, BN));
    if (mode == LOAD_VEC) lpips_conv_kernel<LOAD_VEC><<<grid, TB, 0, st>>>(c);
    else if (mode == LOAD_SCALAR) lpips_conv_kernel<LOAD_SCALAR><<<grid, TB, 0, st>>>(c);
    else lpips_conv_kernel<LOAD_FIRST><<<grid, TB, 0, st>>>(c);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}

int launch_pool(const char *fn, int n_img, int h, int w, int ch, const float *in, float *out, hipStream_t st) {
    MTGS_REQUIRE(n_img > 0 && h >= 3 && w >= 3 && ch > 0, MTGS_EINVAL, "%s: a %d x %d x %d x %d input leaves no 3 x 3 window", fn, n_img, h, w, ch);
    MTGS_REQUIRE(ch % 4 == 0, MTGS_EUNSUPPORTED, "%s: c = %d is not a multiple of 4", fn, ch);
    MTGS_REQUIRE(in && out, MTGS_EINVAL, "%s: null pointer: in or out", fn);
    MTGS_REQUIRE((((uintptr_t)in | (uintptr_t)out) & 15) == 0, MTGS_EINVAL, "%s: in and out must be 16-byte aligned", fn);
    MTGS_REQUIRE((int64_t)n_img * h * w * ch < LIMIT, MTGS_EUNSUPPORTED, "%s: an array of 2^31 elements or more", fn);
    const int oh = pool_out(h), ow = pool_out(w), n = n_img * oh * ow * (ch / 4);
    lpips_maxpool_kernel<<<(unsigned)ceil_div64(n, TB), TB, 0, st>>>(h, w, ch / 4, oh, ow, (const float4 *)in, (float4 *)out, n);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}

// tap sizes and the workspace: two activation buffers and the partials
struct Plan {
    int h[N_LAYERS], w[N_LAYERS];        // output size of each convolution
    int ph[N_LAYERS], pw[N_LAYERS];      // its input size (after the pool, if any)
    size_t a_floats, b_floats;
};

int make_plan(const char *fn, int H, int W, Plan &p) {
    MTGS_REQUIRE(H >= MTGS_LPIPS_MIN_SIDE && W >= MTGS_LPIPS_MIN_SIDE, MTGS_EINVAL,
                 "%s: a %d x %d image leaves no pixel after the second pool (both sides must be >= %d)", fn, H, W, MTGS_LPIPS_MIN_SIDE);
    MTGS_REQUIRE((int64_t)H * W * 3 < LIMIT, MTGS_EUNSUPPORTED, "%s: an image of 2^31 elements or more", fn);
    int h = H, w = W;
    size_t buf[2] = {0, 0};
    int which = 0;                       // buffer the next convolution writes: conv1 -> A, pools -> B, then alternating
    for (int l = 0; l < N_LAYERS; ++l) {
        const Layer &L = LAYERS[l];
        if (L.pool_before) {
            h = pool_out(h);
            w = pool_out(w);
            const size_t n = (size_t)2 * h * w * L.cin;
            if (n > buf[1]) buf[1] = n;
            which = 0;
        }
        p.ph[l] = h;
        p.pw[l] = w;
        h = conv_out(h, L.k, L.stride, L.pad);
        w = conv_out(w, L.k, L.stride, L.pad);
        p.h[l] = h;
        p.w[l] = w;
        const size_t n = (size_t)2 * h * w * L.cout;
        MTGS_REQUIRE((int64_t)n < LIMIT, MTGS_EUNSUPPORTED, "%s: an activation of 2^31 elements or more", fn);
        if (n > buf[which]) buf[which] = n;
        which ^= 1;
    }
    p.a_floats = (buf[0] + 3) & ~(size_t)3;
    p.b_floats = (buf[1] + 3) & ~(size_t)3;
    return MTGS_OK;
}

size_t weight_offset(int layer) {        // floats before layer `layer`'s block of `weights`
    size_t o = 0;
    for (int l = 0; l < layer; ++l) o += (size_t)LAYERS[l].k * LAYERS[l].k * LAYERS[l].cin * LAYERS[l].cout + 2 * (size_t)LAYERS[l].cout;
    return o;
}

}  // namespace

extern "C" int mtgs_lpips_workspace_bytes(int H, int W, size_t *bytes) {
    const char *fn = "mtgs_lpips_workspace_bytes";
    MTGS_REQUIRE(bytes != nullptr, MTGS_EINVAL, "%s: null pointer: bytes", fn);
    Plan p;
    if (int rc = make_plan(fn, H, W, p)) return rc;
    *bytes = (p.a_floats + p.b_floats + (size_t)N_LAYERS * DIST_BLOCKS) * sizeof(float);
    return MTGS_OK;
}

extern "C" int mtgs_lpips_weight_floats(size_t *floats) {
    MTGS_REQUIRE(floats != nullptr, MTGS_EINVAL, "mtgs_lpips_weight_floats: null pointer: floats");
    *floats = weight_offset(N_LAYERS);
    return MTGS_OK;
}

extern "C" int mtgs_lpips_repack(int cout, int cin, int kh, int kw, const float *w, float *packed, void *stream) {
    const char *fn = "mtgs_lpips_repack";
    MTGS_REQUIRE(cout > 0 && cin > 0 && kh > 0 && kw > 0, MTGS_EINVAL, "%s: sizes must be positive (%d, %d, %d, %d)", fn, cout, cin, kh, kw);
    MTGS_REQUIRE(w && packed, MTGS_EINVAL, "%s: null pointer: w or packed", fn);
    const int64_t n = (int64_t)cout * cin * kh * kw;
    MTGS_REQUIRE(n < LIMIT, MTGS_EUNSUPPORTED, "%s: 2^31 weights or more", fn);
    lpips_repack_kernel<<<(unsigned)ceil_div64(n, TB), TB, 0, (hipStream_t)stream>>>(cout, cin, kh, kw, w, packed, (int)n);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}

extern "C" int mtgs_lpips_conv(int n, int h, int w, int cin, int cout, int kh, int kw, int stride, int pad, const float *in, const float *packed,
                               const float *bias, int relu, float *out, void *stream) {
    const char *fn = "mtgs_lpips_conv";
    MTGS_REQUIRE(in != nullptr, MTGS_EINVAL, "%s: null pointer: in", fn);
    Conv c{};
    c.in = in; c.wt = packed; c.bias = bias; c.out = out;
    c.n = n; c.h = h; c.w = w; c.cin = cin; c.cout = cout; c.kh = kh; c.kw = kw; c.stride = stride; c.pad = pad; c.relu = relu;
    return launch_conv(fn, LOAD_SCALAR, c, (hipStream_t)stream);
}

extern "C" int mtgs_lpips_conv_first(int H, int W, const float *pred, const float *gt, const uint8_t *mask, int normalize, int cout,
                                     int kh, int kw, int stride, int pad, const float *packed, const float *bias, int relu, float *out,
                                     void *stream) {
    const char *fn = "mtgs_lpips_conv_first";
    MTGS_REQUIRE(pred && gt, MTGS_EINVAL, "%s: null pointer: pred or gt", fn);
    Conv c{};
    c.img0 = pred; c.img1 = gt; c.mask = mask; c.normalize = normalize; c.wt = packed; c.bias = bias; c.out = out;
    c.n = 2; c.h = H; c.w = W; c.cin = 3; c.cout = cout; c.kh = kh; c.kw = kw; c.stride = stride; c.pad = pad; c.relu = relu;
    return launch_conv(fn, LOAD_FIRST, c, (hipStream_t)stream);
}

extern "C" int mtgs_lpips_maxpool(int n, int h, int w, int c, const float *in, float *out, void *stream) {
    return launch_pool("mtgs_lpips_maxpool", n, h, w, c, in, out, (hipStream_t)stream);
}

extern "C" int mtgs_lpips(int H, int W, const float *pred, const float *gt, const uint8_t *mask, const float *weights, int normalize,
                          int norm, float *out, void *ws, size_t ws_bytes, void *stream) {
    const char *fn = "mtgs_lpips";
    Plan p;
    if (int rc = make_plan(fn, H, W, p)) return rc;
    MTGS_REQUIRE(pred && gt && weights && out && ws, MTGS_EINVAL, "%s: null pointer: pred, gt, weights, out or ws", fn);
    MTGS_REQUIRE(norm == MTGS_LPIPS_NORM_SQRT_EPS_INSIDE || norm == MTGS_LPIPS_NORM_EPS_OUTSIDE, MTGS_EINVAL, "%s: unknown norm %d", fn, norm);
    MTGS_REQUIRE((((uintptr_t)ws | (uintptr_t)weights) & 15) == 0, MTGS_EINVAL, "%s: ws and weights must be 16-byte aligned", fn);
    const size_t need = (p.a_floats + p.b_floats + (size_t)N_LAYERS * DIST_BLOCKS) * sizeof(float);
    MTGS_REQUIRE(ws_bytes >= need, MTGS_EWORKSPACE, "%s: workspace %zu < %zu bytes", fn, ws_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    float *buf[2] = {(float *)ws, (float *)ws + p.a_floats};
    float *partials = (float *)ws + p.a_floats + p.b_floats;
    Finish fin{};
    const float *cur = nullptr;          // the previous tap
    int cur_buf = 1, h = H, w = W;
    for (int l = 0; l < N_LAYERS; ++l) {
        const Layer &L = LAYERS[l];
        const float *wt = weights + weight_offset(l);
        const float *bias = wt + (size_t)L.k * L.k * L.cin * L.cout, *lin = bias + L.cout;
        if (L.pool_before) {             // the tap is in buf[0] here (layers 1 and 2 write it there)
            if (int rc = launch_pool(fn, 2, h, w, L.cin, cur, buf[1], st)) return rc;
            cur = buf[1];
            cur_buf = 1;
        }
        Conv c{};
        c.in = cur; c.img0 = pred; c.img1 = gt; c.mask = mask; c.normalize = normalize; c.wt = wt; c.bias = bias;
        c.out = buf[cur_buf ^ 1];
        c.n = 2; c.h = p.ph[l]; c.w = p.pw[l]; c.cin = L.cin; c.cout = L.cout; c.kh = L.k; c.kw = L.k; c.stride = L.stride; c.pad = L.pad; c.relu = 1;
        if (int rc = launch_conv(fn, l == 0 ? LOAD_FIRST : LOAD_SCALAR, c, st)) return rc;
        cur = c.out;
        cur_buf ^= 1;
        h = p.h[l];
        w = p.w[l];
        const int P = h * w;
        static_assert(LAYERS[2].cout <= 64 * DIST_MAX_Q, "lpips_distance holds a pixel's channels in registers");
        const int blocks = (int)(ceil_div64(P, TB / 64) < DIST_BLOCKS ? ceil_div64(P, TB / 64) : DIST_BLOCKS);
        lpips_distance_kernel<<<(unsigned)blocks, TB, 0, st>>>(P, L.cout, norm, cur, lin, partials + (size_t)l * DIST_BLOCKS);
        MTGS_CHECK_LAUNCH(fn);
        fin.blocks[l] = blocks;
        fin.pixels[l] = P;
    }
    lpips_finish_kernel<<<1, DIST_BLOCKS, 0, st>>>(fin, partials, out);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}
