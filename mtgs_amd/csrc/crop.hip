// crop.hip -- rendering inside an oriented crop box (MTGSSceneModel.get_gaussians / get_gaussian_params,
// mtgs_scene_graph.py:457-459, 493-495): `crop_ids = crop_box.within(means)` and one `v[crop_ids]` per collected tensor,
// as a selection and ONE table-driven row gather on the device.
//
// mtgs_crop_select, one call =
//   mtgs_scan::run               keep(i) as the scanned value (evaluated in the partial and in the final pass: a pure function of
//                                the row), the sink writes keep_ids[exclusive prefix] = i and mask[i]; the spine leaves the count
// so the kept indices come out ascending, the order of the reference's boolean mask, with no atomics and no second pass.
// The decision of row i, p = (x, y, z), against the world->box matrix m (3x4 by rows) and the half sizes h:
//   q_k = ((m_k0 x + m_k1 y) + m_k2 z) + m_k3,   kept iff -h_k < q_k && q_k < h_k for k = 0..2
// in fp32, every operation rounded once (compiled with -ffp-contract=off), as mtgs_amd.crop.OrientedBox.within evaluates it
// in torch on the host and tests/test_crop_host.py in NumPy.  NaN fails both comparisons and drops the row.
//
// mtgs_crop_gather, one launch for up to 16 tensors: a tensor's compacted rows are one contiguous run of 4-byte words; a
// workgroup copies 2048 consecutive words of ONE tensor (which one: its block index against the running sum of the tensors'
// block counts, wave-uniform), so every store is coalesced and a row of any width -- 1, 3, 4, 45, 48 floats, an int64 as two
// words -- takes the same code.  The source row of word e is keep_ids[e / row_words]; one 64-bit division per workgroup,
// 32-bit ones per word.
#include "scan.hpp"

namespace {

constexpr int MAX_TENSORS = 16;
constexpr int GB = 256, GITEMS = 8, GTILE = GB * GITEMS;

struct Box {
    float m[12];   // world -> box, 3x4 by rows
    float h[3];    // half sizes
};

// the crop decision on one axis: STRICT on both faces (nerfstudio's OrientedBox.within: pts > -S / 2 and pts < S / 2)
__device__ __forceinline__ bool inside(float q, float h) { return -h < q && q < h; }

struct KeepValue {
    const float *means;
    int64_t stride;
    Box b;
    __device__ int64_t operator()(int64_t i) const {
        const float *p = means + i * stride;
        const float x = p[0], y = p[1], z = p[2];
        bool keep = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float q = ((b.m[4 * k] * x + b.m[4 * k + 1] * y) + b.m[4 * k + 2] * z) + b.m[4 * k + 3];
            keep = keep && inside(q, b.h[k]);
        }
        return keep ? 1 : 0;
    }
};

struct KeepSink {
    int32_t *keep_ids;
    uint8_t *mask;
    __device__ void operator()(int64_t i, int64_t excl, int64_t incl) const {
        const bool keep = incl != excl;
        if (keep) keep_ids[excl] = (int32_t)i;
        if (mask) mask[i] = keep ? 1 : 0;
    }
};

struct GatherTable {
    const uint32_t *src[MAX_TENSORS];
    uint32_t *dst[MAX_TENSORS];
    int64_t first_block[MAX_TENSORS];   // running sum of ceil(n_keep * row_words / GTILE)
    uint32_t row_words[MAX_TENSORS];
    int32_t n;
};

__global__ __launch_bounds__(GB) void crop_gather_kernel(GatherTable t, int64_t n_keep, int64_t n_rows,
                                                         const int32_t *__restrict__ keep_ids) {
    const int64_t b = blockIdx.x;
    int j = 0;
#pragma unroll
    for (int k = 1; k < MAX_TENSORS; ++k)
        if (k < t.n && b >= t.first_block[k]) j = k;
    const uint32_t rw = t.row_words[j];
    const uint32_t *__restrict__ src = t.src[j];
    uint32_t *__restrict__ dst = t.dst[j];
    const int64_t e0 = (b - t.first_block[j]) * GTILE, total = n_keep * rw;
    const int64_t row0 = e0 / rw;
    const uint32_t rem0 = (uint32_t)(e0 - row0 * rw);
#pragma unroll
    for (int i = 0; i < GITEMS; ++i) {
        const uint32_t local = (uint32_t)(i * GB) + threadIdx.x;
        const int64_t e = e0 + local;
        if (e >= total) break;
        const uint32_t off = rem0 + local, dr = off / rw, c = off - dr * rw;
        const int64_t id = keep_ids[row0 + dr];
        if (id >= 0 && id < n_rows) dst[e] = src[id * rw + c];   // an index outside the source (not mtgs_crop_select's) is not followed
    }
}

}  // namespace


extern "C" int mtgs_crop_workspace_bytes(int64_t N, size_t *bytes) {
    const char *fn = "mtgs_crop_workspace_bytes";
    MTGS_COUNT31(fn, N);
    MTGS_NONNULL(fn, bytes);
    *bytes = mtgs_scan::workspace_bytes(N);
    return MTGS_OK;
}

extern "C" int mtgs_crop_select(int64_t N, const float *means, int64_t row_stride, const float *box, int32_t *keep_ids,
                                int64_t *count, uint8_t *mask, void *ws, size_t ws_bytes, void *stream) {
    const char *fn = "mtgs_crop_select";
    MTGS_COUNT31(fn, N);
    MTGS_NONNULL(fn, count);
    MTGS_REQUIRE(((uintptr_t)count & 7) == 0, MTGS_EINVAL, "%s: count must be 8-byte aligned", fn);
    hipStream_t st = (hipStream_t)stream;
    if (N == 0) return mtgs_zero_async(count, sizeof(int64_t), st);
    MTGS_REQUIRE(row_stride >= 3, MTGS_EINVAL, "%s: row_stride < 3 (%lld)", fn, (long long)row_stride);
    MTGS_NONNULL(fn, means); MTGS_NONNULL(fn, box); MTGS_NONNULL(fn, keep_ids); MTGS_NONNULL(fn, ws);
    const size_t need = mtgs_scan::workspace_bytes(N);
    MTGS_REQUIRE(ws_bytes >= need, MTGS_EWORKSPACE, "%s: workspace %zu < %zu bytes", fn, ws_bytes, need);
    MTGS_REQUIRE(((uintptr_t)ws & 7) == 0, MTGS_EINVAL, "%s: workspace must be 8-byte aligned", fn);
    KeepValue value{means, row_stride, {}};
    for (int k = 0; k < 12; ++k) value.b.m[k] = box[k];
    for (int k = 0; k < 3; ++k) value.b.h[k] = box[12 + k];
    mtgs_scan::run(N, value, KeepSink{keep_ids, mask}, (int64_t *)ws, count, st);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}

extern "C" int mtgs_crop_gather(int64_t n_keep, int64_t n_rows, const int32_t *keep_ids, int n_tensors, const uint64_t *src,
                                const uint64_t *dst, const int64_t *row_bytes, void *stream) {
    const char *fn = "mtgs_crop_gather";
    MTGS_COUNT31(fn, n_keep);
    MTGS_COUNT31(fn, n_rows);
    MTGS_REQUIRE(n_tensors >= 1 && n_tensors <= MAX_TENSORS, MTGS_EINVAL, "%s: n_tensors outside [1, %d] (%d)", fn, MAX_TENSORS, n_tensors);
    MTGS_REQUIRE(n_keep <= n_rows, MTGS_EINVAL, "%s: n_keep %lld > n_rows %lld", fn, (long long)n_keep, (long long)n_rows);
    MTGS_NONNULL(fn, src); MTGS_NONNULL(fn, dst); MTGS_NONNULL(fn, row_bytes);
    for (int j = 0; j < n_tensors; ++j)
        MTGS_REQUIRE(row_bytes[j] >= 4 && row_bytes[j] % 4 == 0 && row_bytes[j] <= ((int64_t)1 << 30), MTGS_EINVAL,
                     "%s: row_bytes[%d] must be a multiple of 4 in [4, 2^30] (%lld)", fn, j, (long long)row_bytes[j]);
    if (n_keep == 0) return MTGS_OK;
    MTGS_NONNULL(fn, keep_ids);
    GatherTable t{};
    int64_t blocks = 0;
    for (int j = 0; j < n_tensors; ++j) {
        MTGS_REQUIRE(src[j] != 0 && dst[j] != 0, MTGS_EINVAL, "%s: null pointer: %s[%d]", fn, src[j] ? "dst" : "src", j);
        MTGS_REQUIRE(((src[j] | dst[j]) & 3) == 0, MTGS_EINVAL, "%s: src[%d] and dst[%d] must be 4-byte aligned", fn, j, j);
        t.src[j] = (const uint32_t *)(uintptr_t)src[j];
        t.dst[j] = (uint32_t *)(uintptr_t)dst[j];
        t.row_words[j] = (uint32_t)(row_bytes[j] / 4);
        t.first_block[j] = blocks;
        blocks += ceil_div64(n_keep * (int64_t)t.row_words[j], GTILE);
    }
    t.n = n_tensors;
    MTGS_REQUIRE(blocks < ((int64_t)1 << 31), MTGS_EINVAL, "%s: %lld workgroups: gather fewer tensors per call", fn, (long long)blocks);
    crop_gather_kernel<<<(unsigned)blocks, GB, 0, (hipStream_t)stream>>>(t, n_keep, n_rows, keep_ids);
    MTGS_CHECK_LAUNCH(fn);
    return MTGS_OK;
}
