// refine.hip -- densification of the Gaussian nodes of a scene graph on the device (include/mtgs_refine_scene.h): split /
// duplicate / cull with every per-Gaussian tensor (parameters AND the optimizer's moment rows) compacted and appended by
// kernels, and the split / clone samples drawn from a COUNTER-BASED generator keyed by (node seed, step, node-local Gaussian
// index, sample), so that every rank of a data-parallel job -- whatever its launch geometry -- makes bit-identical decisions
// and rows.  The nodes come in a table in device memory; ONE node is the one-entry case of that table, there is no second path.
//
// Restates VanillaGaussianSplattingModel.refinement_after / split_gaussians / dup_gaussians / cull_gaussians and the
// optimizer surgery dup_in_optim / remove_from_optim
// (/root/reference/mtgs/scene_model/gaussian_model/vanilla_gaussian_splatting.py:392-446, 476-577, 579-699), which run
// as ~60 masked PyTorch ops with half a dozen .item() synchronisations and per-rank torch.randn (:642, :687):
//   avg = xys_grad_norm / vis_counts;  high = avg > densify_grad_thresh
//   split = (max exp(scales) > densify_size_thresh & high) | (max_2Dsize > split_screen_size)        [the latter early on]
//   children (n_split_samples per split): mean + R(q/|q|) (exp(scales) * z),  scales <- log(exp(scales) / 1.6)
//   (the parent's scales shrink IN PLACE too, :657 -- so)  dup = (max exp(scales') <= densify_size_thresh) & high
//   copies of dup (their mean resampled the same way when clone_sample_means, :686-697)
//   new set = [old | children, sample-major | dups];  cull: split parents, sigmoid(opacity) < cull_alpha_thresh, and (later)
//   world-space / screen-space size limits (:585-612); moments: old rows follow, new rows start at zero (:418-437).
// The result order is the reference's (boolean-mask order of that concatenation).
//
// Kernels: classify (per old Gaussian: what it becomes + how many rows survive), then -- after an inclusive scan of the
// survivor counts over all nodes -- index (source row and kind of every output row), geometry (means / scales of every output
// row) and one table-driven launch that moves every remaining tensor of every node.  Roofline: HBM (streaming + gathers).
#include "common.hpp"

namespace {

struct RefineCfg {
    float grad_thresh, size_thresh, split_screen_size, cull_alpha_thresh, cull_scale_thresh, cull_screen_size;
    int nsamps, use_screen_split, cull_big, cull_screen, clone_sample_means;
    uint32_t seed_lo, seed_hi, step;
    float far_radius, far_factor;   // cull rule: beyond |mean| > far_radius the size limit is far_factor * cull_scale_thresh
};
constexpr int MAX_SAMPS = 4;
constexpr float kSplitShrink = 1.6f;

// ---- Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3"): counter (index, slot, step, 0), key seed
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&out)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// three standard normals for (Gaussian index, slot): Box-Muller on uniforms (x + 0.5) * 2^-32
__device__ __forceinline__ void refine_normal3(const RefineCfg &cfg, uint32_t index, uint32_t slot, float (&z)[3]) {
    uint32_t r[4];
    philox4x32_10(index, slot, cfg.step, 0u, cfg.seed_lo, cfg.seed_hi, r);
    const float u0 = ((float)r[0] + 0.5f) * 2.3283064365386963e-10f, u1 = ((float)r[1] + 0.5f) * 2.3283064365386963e-10f;
    const float u2 = ((float)r[2] + 0.5f) * 2.3283064365386963e-10f, u3 = ((float)r[3] + 0.5f) * 2.3283064365386963e-10f;
    const float ra = sqrtf(-2.f * logf(fmaxf(u0, 1e-37f))), rb = sqrtf(-2.f * logf(fmaxf(u2, 1e-37f)));
    z[0] = ra * cosf(6.283185307179586f * u1);
    z[1] = ra * sinf(6.283185307179586f * u1);
    z[2] = rb * cosf(6.283185307179586f * u3);
}
// mean + R(q / |q|) (exp(scales) * z)     (wxyz; mtgs utils.quat_to_rotmat)
__device__ __forceinline__ void sample_mean(const float (&m)[3], const float (&sl)[3], const float4 q, const float (&z)[3], float (&out)[3]) {
    const float inv = 1.0f / sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
    const float w = q.x * inv, x = q.y * inv, y = q.z * inv, zz = q.w * inv;
    const float v0 = expf(sl[0]) * z[0], v1 = expf(sl[1]) * z[1], v2 = expf(sl[2]) * z[2];
    out[0] = m[0] + (1 - 2 * (y * y + zz * zz)) * v0 + 2 * (x * y - w * zz) * v1 + 2 * (x * zz + w * y) * v2;
    out[1] = m[1] + 2 * (x * y + w * zz) * v0 + (1 - 2 * (x * x + zz * zz)) * v1 + 2 * (y * zz - w * x) * v2;
    out[2] = m[2] + 2 * (x * zz - w * y) * v0 + 2 * (y * zz + w * x) * v1 + (1 - 2 * (x * x + y * y)) * v2;
}
__device__ __forceinline__ float max_exp(const float (&sl)[3]) { return fmaxf(fmaxf(expf(sl[0]), expf(sl[1])), expf(sl[2])); }
// cull_gaussians (:579-612) for one row
__device__ __forceinline__ bool culled(const RefineCfg &c, const float (&m)[3], const float (&sl)[3], float opacity_logit, float max2d) {
    bool cull = 1.0f / (1.0f + expf(-opacity_logit)) < c.cull_alpha_thresh;
    if (c.cull_big) {
        const bool far = sqrtf(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]) > c.far_radius;
        cull = cull || max_exp(sl) > (far ? c.far_factor : 1.f) * c.cull_scale_thresh;
        if (c.cull_screen) cull = cull || max2d > c.cull_screen_size;
    }
    return cull;
}
struct Node {
    float m[3], sl[3], sl_cur[3];   // sl_cur: the scales after the in-place shrink of a split parent
    float4 q;
    float opac;
    bool split, dup;
};
__device__ __forceinline__ Node classify(const RefineCfg &c, int64_t i, const float *means, const float *scales, const float *quats,
                                         const float *opacities, const float *grad_norm, const float *vis_counts, const float *max2d) {
    Node n;
#pragma unroll
    for (int k = 0; k < 3; ++k) { n.m[k] = means[i * 3 + k]; n.sl[k] = scales[i * 3 + k]; }
    n.q = reinterpret_cast<const float4 *>(quats)[i];
    n.opac = opacities[i];
    const bool high = grad_norm[i] / vis_counts[i] > c.grad_thresh;
    n.split = (max_exp(n.sl) > c.size_thresh) && high;
    if (c.use_screen_split) n.split = n.split || max2d[i] > c.split_screen_size;
#pragma unroll
    for (int k = 0; k < 3; ++k) n.sl_cur[k] = n.split ? logf(expf(n.sl[k]) / kSplitShrink) : n.sl[k];
    n.dup = (max_exp(n.sl_cur) <= c.size_thresh) && high;
    return n;
}

// ---- the kernels (include/mtgs_refine_scene.h) ---------------------------------------------------------------------------------
// Per node from a table in device memory: the node's thresholds, options, seed, cull rule and phase.  Gaussian indices are
// NODE-LOCAL everywhere (the Philox counter, src_index), so a node refines identically alone and inside any scene.
static_assert(MTGS_REFINE_MAX_COLUMNS == 2 + MAX_SAMPS, "columns: old | MAX_SAMPS children | duplicate");

__device__ __forceinline__ RefineCfg node_cfg(const mtgs_refine_node &d, uint32_t step) {
    RefineCfg c;
    c.grad_thresh = d.thresholds[0]; c.size_thresh = d.thresholds[1]; c.split_screen_size = d.thresholds[2];
    c.cull_alpha_thresh = d.thresholds[3]; c.cull_scale_thresh = d.thresholds[4]; c.cull_screen_size = d.thresholds[5];
    c.nsamps = d.options[0]; c.use_screen_split = d.options[1]; c.cull_big = d.options[2]; c.cull_screen = d.options[3];
    c.clone_sample_means = d.options[4];
    c.seed_lo = (uint32_t)d.seed; c.seed_hi = (uint32_t)(d.seed >> 32); c.step = step;
    c.far_radius = d.far_radius; c.far_factor = d.far_factor;
    return c;
}
// the node whose workgroups contain `block` (first_block ascending; the search of densify_stats_batch_kernel)
template <int64_t mtgs_refine_node::*FIRST>
__device__ __forceinline__ int find_node(const mtgs_refine_node *__restrict__ table, int n_nodes, int64_t block) {
    int lo = 0, hi = n_nodes - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].*FIRST <= block) lo = mid; else hi = mid - 1;
    }
    return __builtin_amdgcn_readfirstlane(lo);
}

__global__ __launch_bounds__(256) void refine_scene_classify_kernel(const mtgs_refine_node *__restrict__ table, int n_nodes,
                                                                   int64_t n_total, int n_columns, uint32_t step,
                                                                   int32_t *__restrict__ counts /* [n_columns + 1][n_total] */,
                                                                   uint8_t *__restrict__ flags, uint8_t *__restrict__ parents) {
    const mtgs_refine_node &d = table[find_node<&mtgs_refine_node::first_block>(table, n_nodes, (int64_t)blockIdx.x)];
    const int64_t i = ((int64_t)blockIdx.x - d.first_block) * 256 + threadIdx.x;
    if (i >= d.n) return;
    const RefineCfg c = node_cfg(d, step);
    const int64_t g = d.start + i;
    uint32_t f = 0u;                                   // bit 0 old row kept | bit 1+s child s kept | bit 1+nsamps dup kept | bit 7 split
    if (d.phase == MTGS_REFINE_CULL_ONLY) {            // cull_gaussians() without a split mask: rows only leave
        float m[3], sl[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { m[k] = d.means[i * 3 + k]; sl[k] = d.scales[i * 3 + k]; }
        const float m2 = (c.cull_big && c.cull_screen) ? d.max_2dsize[i] : 0.f;
        if (!culled(c, m, sl, d.opacities[i], m2)) f = 1u;
    } else {                                           // MTGS_REFINE_DENSIFY: the only statement of the decisions
        const Node n = classify(c, i, d.means, d.scales, d.quats, d.opacities, d.xys_grad_norm, d.vis_counts, d.max_2dsize);
        f = n.split ? 0x80u : 0u;
        if (!n.split && !culled(c, n.m, n.sl, n.opac, d.max_2dsize[i])) f |= 1u;
        for (int s = 0; s < c.nsamps; ++s) {
            bool keep = false;
            if (n.split) {
                float z[3], cm[3];
                refine_normal3(c, (uint32_t)i, (uint32_t)s, z);
                sample_mean(n.m, n.sl, n.q, z, cm);
                keep = !culled(c, cm, n.sl_cur, n.opac, 0.f);   // (new rows enter with max_2Dsize = 0, :517-524)
            }
            if (keep) f |= 2u << s;
        }
        bool keep_dup = false;
        if (n.dup) {
            float dm[3] = {n.m[0], n.m[1], n.m[2]};
            if (c.clone_sample_means) {
                float z[3];
                refine_normal3(c, (uint32_t)i, (uint32_t)c.nsamps, z);
                sample_mean(n.m, n.sl_cur, n.q, z, dm);
            }
            keep_dup = !culled(c, dm, n.sl_cur, n.opac, 0.f);
        }
        if (keep_dup) f |= 2u << c.nsamps;
    }
    for (int k = 0; k < n_columns; ++k) counts[(int64_t)k * n_total + g] = (int32_t)((f >> k) & 1u);   // (bits above 1 + nsamps are 0)
    counts[(int64_t)n_columns * n_total + g] = (int32_t)(f >> 7);
    flags[g] = (uint8_t)f;
    if (parents) parents[g] = (f & 0x7Eu) != 0u ? 1 : 0;
}

// incl: INCLUSIVE scans of the count rows over the whole concatenation
__global__ __launch_bounds__(256) void refine_scene_index_kernel(const mtgs_refine_node *__restrict__ table, int n_nodes,
                                                                int64_t n_total, const uint8_t *__restrict__ flags,
                                                                const int64_t *__restrict__ incl, int32_t *__restrict__ src_index,
                                                                uint8_t *__restrict__ kind) {
    const mtgs_refine_node &d = table[find_node<&mtgs_refine_node::first_block>(table, n_nodes, (int64_t)blockIdx.x)];
    const int64_t i = ((int64_t)blockIdx.x - d.first_block) * 256 + threadIdx.x;
    if (i >= d.n) return;
    const int64_t g = d.start + i;
    const uint32_t f = flags[g];
    const int ncol = 2 + d.options[0];
    for (int k = 0; k < ncol; ++k) {
        if ((f >> k) & 1u) {
            const int64_t local = d.col_base[k] + (incl[(int64_t)k * n_total + g] - 1 - d.scan_base[k]);
            if (local < 0 || local >= d.n_out) continue;      // (a table that does not belong to these scans: write nothing)
            src_index[d.out_start + local] = (int32_t)i;
            kind[d.out_start + local] = (uint8_t)k;           // 0 old | 1 + s child of sample s | 1 + nsamps duplicate
        }
    }
}

__global__ __launch_bounds__(256) void refine_scene_geometry_kernel(const mtgs_refine_node *__restrict__ table, int n_nodes,
                                                                   uint32_t step, const int32_t *__restrict__ src_index,
                                                                   const uint8_t *__restrict__ kind, const uint8_t *__restrict__ flags,
                                                                   float *__restrict__ out_means, float *__restrict__ out_scales) {
    const mtgs_refine_node &d = table[find_node<&mtgs_refine_node::out_first_block>(table, n_nodes, (int64_t)blockIdx.x)];
    const int64_t rl = ((int64_t)blockIdx.x - d.out_first_block) * 256 + threadIdx.x;
    if (rl >= d.n_out) return;
    const RefineCfg c = node_cfg(d, step);
    const int64_t r = d.out_start + rl;
    const int64_t p = src_index[r];
    if (p < 0 || p >= d.n) return;
    const int k = kind[r];
    float m[3], sl[3], sl_cur[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) { m[j] = d.means[p * 3 + j]; sl[j] = d.scales[p * 3 + j]; }
    const bool split = (flags[d.start + p] & 0x80u) != 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) sl_cur[j] = split ? logf(expf(sl[j]) / kSplitShrink) : sl[j];
    float om[3] = {m[0], m[1], m[2]};
    if (k >= 1 && (k <= c.nsamps || c.clone_sample_means)) {
        float z[3];
        refine_normal3(c, (uint32_t)p, (uint32_t)(k - 1), z);
        const float4 q = reinterpret_cast<const float4 *>(d.quats)[p];
        if (k <= c.nsamps) sample_mean(m, sl, q, z, om);     // children: the parent's ORIGINAL scales spread the samples
        else sample_mean(m, sl_cur, q, z, om);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        out_means[r * 3 + j] = om[j];
        out_scales[r * 3 + j] = k == 0 ? sl[j] : sl_cur[j];
    }
}

// Every remaining tensor of every node: one move per (node, tensor).  A workgroup owns MTGS_REFINE_MOVE_DWORDS consecutive dwords
// of its move's destination, in chunks of 1024; a lane four dwords of each chunk, shifted so that the four start at a 16-byte
// boundary: one dwordx4 store per lane and chunk, whatever the row width.  Finding the move (a binary search: dependent loads) and
// the row and column of the workgroup's first dword (a 64-bit division on uniform operands) are paid once per workgroup, i.e. per
// 32 KiB moved; a lane's row and column follow from a 32-bit multiply-high and the three dwords after it from an increment.
// Sources are row gathers: a lane's four dwords come as one dwordx4 load where they lie in one row at a 16-byte boundary (every
// load of a 4-dword row), otherwise as dword loads that neighbouring lanes coalesce; src_index / kind are read once per row.
constexpr int MOVE_CHUNK = 1024;
static_assert(MTGS_REFINE_MOVE_DWORDS % MOVE_CHUNK == 0, "whole chunks");
__global__ __launch_bounds__(256) void refine_scene_rows_kernel(const mtgs_refine_move *__restrict__ moves, int n_moves,
                                                               const int32_t *__restrict__ src_index, const uint8_t *__restrict__ kind) {
    int lo = 0, hi = n_moves - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (moves[mid].first_block <= (int64_t)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const mtgs_refine_move &mv = moves[__builtin_amdgcn_readfirstlane(lo)];
    const uint32_t w = (uint32_t)mv.width;
    const int op = mv.op;
    const int64_t total = mv.n_rows * (int64_t)w, n_src = mv.n_src;
    const float cm = mv.clamp_max;
    uint32_t *dst = static_cast<uint32_t *>(mv.dst);
    const uint32_t *src = static_cast<const uint32_t *>(mv.src);
    const int32_t *idx = src_index + mv.out_start;
    const uint8_t *kd = kind + mv.out_start;
    // v = e + pad counts the destination's dwords from the 16-byte boundary at or before dst: a lane's four dwords start at a
    // multiple of four in v.  Only the move's first workgroup has lanes whose dwords begin before element 0.
    const int pad = (int)((reinterpret_cast<uintptr_t>(dst) >> 2) & 3u);
    const int64_t vb = ((int64_t)blockIdx.x - mv.first_block) * MTGS_REFINE_MOVE_DWORDS;
    const int64_t eb = vb - pad > 0 ? vb - pad : 0;                                // the workgroup's first element
    const int skip = (int)(eb - (vb - pad));                                       // 0, or pad in the first workgroup
    const int64_t r0 = eb / (int64_t)w;
    const uint32_t c0 = (uint32_t)(eb - r0 * (int64_t)w);
    const uint32_t magic = 0xFFFFFFFFu / w + 1u;                                   // q / w = umulhi(q, magic) while q * w < 2^32: q < 8192 + w, w <= 32768
    for (int chunk = 0; chunk < MTGS_REFINE_MOVE_DWORDS / MOVE_CHUNK; ++chunk) {
        const int o0 = chunk * MOVE_CHUNK + 4 * (int)threadIdx.x - skip;           // the lane's first dword, relative to eb (< 0: before element 0)
        const int first = o0 < 0 ? 0 : o0;
        if (eb + first >= total) return;
        const uint32_t q = c0 + (uint32_t)first;
        const uint32_t dr = w == 1u ? q : __umulhi(q, magic);
        const int64_t r = r0 + dr;
        const uint32_t col = q - dr * w;
        const bool whole = o0 >= 0 && eb + o0 + 4 <= total;
        uint32_t v[4] = {0u, 0u, 0u, 0u};
        if (op != MTGS_REFINE_ZERO_ALL) {
            int64_t rr = r, p = idx[r];
            uint32_t cc = col;
            bool zero = (op == MTGS_REFINE_ZERO_NEW && kd[r] != 0) || p < 0 || p >= n_src;   // (an index that is no row: zeros, nothing followed)
            const uint32_t *sp = src + p * w + col;
            if (whole && col + 4u <= w && (zero || (reinterpret_cast<uintptr_t>(sp) & 15u) == 0)) {   // four dwords of one row, aligned
                if (!zero) {
                    const uint4 t = *reinterpret_cast<const uint4 *>(sp);
                    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int o = o0 + j;
                    if (o >= 0 && eb + o < total) {
                        if (cc == w) {                                             // the next row
                            cc = 0; ++rr;
                            p = idx[rr];
                            zero = (op == MTGS_REFINE_ZERO_NEW && kd[rr] != 0) || p < 0 || p >= n_src;
                        }
                        v[j] = zero ? 0u : src[p * w + cc];
                        ++cc;
                    }
                }
            }
            if (op == MTGS_REFINE_CLAMP_MAX) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float x = __uint_as_float(v[j]);
                    v[j] = __float_as_uint(x > cm ? cm : x);                       // (torch.clamp(max=): a NaN stays)
                }
            }
        }
        if (whole) {
            *reinterpret_cast<uint4 *>(dst + eb + o0) = uint4{v[0], v[1], v[2], v[3]};
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int o = o0 + j;
                if (o >= 0 && eb + o < total) dst[eb + o] = v[j];
            }
        }
    }
}

}  // namespace

// ---- the entry points (include/mtgs_refine_scene.h) --------------------------------------------------------------------------
extern "C" int mtgs_refine_scene_table_bytes(size_t *node_bytes, size_t *move_bytes) {
    MTGS_REQUIRE(node_bytes, MTGS_EINVAL, "mtgs_refine_scene_table_bytes: null pointer: node_bytes");
    MTGS_REQUIRE(move_bytes, MTGS_EINVAL, "mtgs_refine_scene_table_bytes: null pointer: move_bytes");
    *node_bytes = sizeof(mtgs_refine_node);
    *move_bytes = sizeof(mtgs_refine_move);
    return MTGS_OK;
}

extern "C" int mtgs_refine_scene_classify(int n_nodes, const mtgs_refine_node *table, int64_t total_blocks, int64_t n_total,
                                          int n_columns, int64_t step, int32_t *counts, uint8_t *flags, uint8_t *parents,
                                          void *stream) {
    MTGS_REQUIRE(n_nodes >= 0, MTGS_EINVAL, "mtgs_refine_scene_classify: n_nodes < 0 (%d)", n_nodes);
    MTGS_REQUIRE(n_total >= 0 && n_total < ((int64_t)1 << 31), MTGS_EINVAL,
                 "mtgs_refine_scene_classify: n_total outside [0, 2^31) (%lld)", (long long)n_total);
    MTGS_REQUIRE(n_columns >= 3 && n_columns <= MTGS_REFINE_MAX_COLUMNS, MTGS_EUNSUPPORTED,
                 "mtgs_refine_scene_classify: n_columns outside [3, %d] (%d)", MTGS_REFINE_MAX_COLUMNS, n_columns);
    MTGS_REQUIRE(total_blocks >= 0 && total_blocks <= n_total, MTGS_EINVAL,
                 "mtgs_refine_scene_classify: total_blocks outside [0, n_total] (%lld)", (long long)total_blocks);
    if (n_nodes == 0 || n_total == 0 || total_blocks == 0) return MTGS_OK;
    MTGS_NONNULL("mtgs_refine_scene_classify", table);
    MTGS_NONNULL("mtgs_refine_scene_classify", counts);
    MTGS_NONNULL("mtgs_refine_scene_classify", flags);
    MTGS_REQUIRE((reinterpret_cast<uintptr_t>(table) & 7) == 0, MTGS_EINVAL, "mtgs_refine_scene_classify: table must be 8-byte aligned");
    refine_scene_classify_kernel<<<(unsigned)total_blocks, 256, 0, (hipStream_t)stream>>>(table, n_nodes, n_total, n_columns,
                                                                                          (uint32_t)step, counts, flags, parents);
    MTGS_CHECK_LAUNCH("mtgs_refine_scene_classify");
    return MTGS_OK;
}

extern "C" int mtgs_refine_scene_apply(int n_nodes, const mtgs_refine_node *table, int64_t total_blocks, int64_t out_blocks,
                                       int64_t n_total, int64_t n_out_total, int n_columns, int64_t step, const uint8_t *flags,
                                       const int64_t *incl, int32_t *src_index, uint8_t *kind, float *out_means, float *out_scales,
                                       void *stream) {
    MTGS_REQUIRE(n_nodes >= 0, MTGS_EINVAL, "mtgs_refine_scene_apply: n_nodes < 0 (%d)", n_nodes);
    MTGS_REQUIRE(n_total >= 0 && n_total < ((int64_t)1 << 31), MTGS_EINVAL,
                 "mtgs_refine_scene_apply: n_total outside [0, 2^31) (%lld)", (long long)n_total);
    MTGS_REQUIRE(n_out_total >= 0 && n_out_total < ((int64_t)1 << 31), MTGS_EINVAL,
                 "mtgs_refine_scene_apply: n_out_total outside [0, 2^31) (%lld)", (long long)n_out_total);
    MTGS_REQUIRE(n_columns >= 3 && n_columns <= MTGS_REFINE_MAX_COLUMNS, MTGS_EUNSUPPORTED,
                 "mtgs_refine_scene_apply: n_columns outside [3, %d] (%d)", MTGS_REFINE_MAX_COLUMNS, n_columns);
    MTGS_REQUIRE(total_blocks >= 0 && total_blocks <= n_total, MTGS_EINVAL,
                 "mtgs_refine_scene_apply: total_blocks outside [0, n_total] (%lld)", (long long)total_blocks);
    MTGS_REQUIRE(out_blocks >= 0 && out_blocks <= n_out_total, MTGS_EINVAL,
                 "mtgs_refine_scene_apply: out_blocks outside [0, n_out_total] (%lld)", (long long)out_blocks);
    if (n_nodes == 0 || n_total == 0 || n_out_total == 0 || total_blocks == 0 || out_blocks == 0) return MTGS_OK;
    MTGS_NONNULL("mtgs_refine_scene_apply", table);
    MTGS_NONNULL("mtgs_refine_scene_apply", flags);
    MTGS_NONNULL("mtgs_refine_scene_apply", incl);
    MTGS_NONNULL("mtgs_refine_scene_apply", src_index);
    MTGS_NONNULL("mtgs_refine_scene_apply", kind);
    MTGS_NONNULL("mtgs_refine_scene_apply", out_means);
    MTGS_NONNULL("mtgs_refine_scene_apply", out_scales);
    MTGS_REQUIRE((reinterpret_cast<uintptr_t>(table) & 7) == 0, MTGS_EINVAL, "mtgs_refine_scene_apply: table must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    refine_scene_index_kernel<<<(unsigned)total_blocks, 256, 0, st>>>(table, n_nodes, n_total, flags, incl, src_index, kind);
    refine_scene_geometry_kernel<<<(unsigned)out_blocks, 256, 0, st>>>(table, n_nodes, (uint32_t)step, src_index, kind, flags,
                                                                        out_means, out_scales);
    MTGS_CHECK_LAUNCH("mtgs_refine_scene_apply");
    return MTGS_OK;
}

extern "C" int mtgs_refine_scene_rows(int n_moves, const mtgs_refine_move *moves, int64_t total_blocks, const int32_t *src_index,
                                      const uint8_t *kind, void *stream) {
    MTGS_REQUIRE(n_moves >= 0, MTGS_EINVAL, "mtgs_refine_scene_rows: n_moves < 0 (%d)", n_moves);
    MTGS_REQUIRE(total_blocks >= 0 && total_blocks < ((int64_t)1 << 31), MTGS_EINVAL,
                 "mtgs_refine_scene_rows: total_blocks outside [0, 2^31) (%lld)", (long long)total_blocks);
    if (n_moves == 0 || total_blocks == 0) return MTGS_OK;
    MTGS_NONNULL("mtgs_refine_scene_rows", moves);
    MTGS_NONNULL("mtgs_refine_scene_rows", src_index);
    MTGS_NONNULL("mtgs_refine_scene_rows", kind);
    MTGS_REQUIRE((reinterpret_cast<uintptr_t>(moves) & 7) == 0, MTGS_EINVAL, "mtgs_refine_scene_rows: moves must be 8-byte aligned");
    refine_scene_rows_kernel<<<(unsigned)total_blocks, 256, 0, (hipStream_t)stream>>>(moves, n_moves, src_index, kind);
    MTGS_CHECK_LAUNCH("mtgs_refine_scene_rows");
    return MTGS_OK;
}
