"""What tests/test_gpu_densify_edges.py compares the densification kernels (csrc/stats.hip, csrc/refine.hip) with when it calls them
directly through the C ABI -- TEST INFRASTRUCTURE ONLY, NumPy, no GPU:

  * the three tables (mtgs_refine_node, mtgs_refine_move, mtgs_stats_desc) as NumPy records whose layouts are the ones
    mtgs_amd.densify reads from the headers, and the host arithmetic of include/mtgs_refine_scene.h that fills them;
  * flags_ref: the flag byte, the `parents` mask and the `counts` rows of every Gaussian, derived from the keep / kind / src_index /
    splits of tests/refine_scene_refs.refinement_after for ANY option set of the kernel (the wrapper can only produce the option
    sets a training step has);
  * move_ref: the row mover as a plain gather on uint32 words;
  * the sample positions: uniforms_f32 is the KERNEL'S DEFINITION of its uniforms (Philox word -> float32, + 0.5f, * 2^-32, each
    rounded to float32); sample_ref64 continues from those float32 uniforms in float64 and returns with every number the sum of the
    |terms| it was made of; sample_f32 rounds every operation to float32 in the kernel's order and exists only to MEASURE the two
    constants below (tests/test_refine_edge_refs_host.py) -- it is never compared with the device;
  * the inputs of the GPU precision test (precision_cases), so that the constants are measured on exactly those.
"""
from functools import lru_cache

import numpy as np

from mtgs_amd import densify as D
from mtgs_amd.densify import RefineConfig
from oracle.refine_oracle import philox4x32_10
from tests import blend_refs as B
from tests import refine_scene_refs as R

F = np.float32
EPS = B.EPS
NODE, MOVE, STATS = D._REFINE_NODE, D._REFINE_MOVE, D._STATS_DESC
DENSIFY, CULL_ONLY = D._DENSIFY, D._CULL_ONLY
COPY, ZERO_NEW, CLAMP_MAX, ZERO_ALL = D._COPY, D._ZERO_NEW, D._CLAMP_MAX, D._ZERO_ALL
MOVE_DWORDS = D._MOVE_DWORDS
MAX_COLUMNS = D._SCENE_ABI.constants["MTGS_REFINE_MAX_COLUMNS"]
SHRINK = 1.6
OFF = 1e30

device_bound = B.device_bound
worst_ratio = B.worst_ratio

# The worst |sample_f32 - sample_ref64| / (2^-24 terms) over precision_cases(), MEASURED on the CPU by
# tests/test_refine_edge_refs_host.py::test_constants -- never against a HIP kernel -- which also asserts that the float32 restatement
# stays within them.  Measured 2026-10-21, rounded up in the second decimal: means 6.302, scales 2.485.
SAMPLE_MEANS = 6.31
SAMPLE_SCALES = 2.49


# ---- tables ---------------------------------------------------------------------------------------------------------------------------
def blocks_of(n):
    return (np.asarray(n, dtype=np.int64) + 255) // 256


def stats_table(n, start, pointers, first_block=True):
    """mtgs_stats_desc records: pointers[i] = (xys_grad_norm, vis_counts, max_2dsize) of node i; first_block = running sum of
    ceil(n / 256) (the batch kernel's) or zero (the rows kernel does not read it)."""
    n = np.asarray(n, dtype=np.int64)
    tab = np.zeros(len(n), dtype=STATS)
    tab["n"], tab["start"] = n, start
    if first_block:
        tab["first_block"] = np.cumsum(blocks_of(n)) - blocks_of(n)
    for j, k in enumerate(("xys_grad_norm", "vis_counts", "max_2dsize")):
        tab[k] = [p[j] for p in pointers]
    return tab


def node_table(nodes):
    """mtgs_refine_node records before the host read.  nodes: dicts with n, the seven pointers, seed, thresholds[6], options[5],
    far_radius, far_factor, phase."""
    tab = np.zeros(len(nodes), dtype=NODE)
    n = np.asarray([d["n"] for d in nodes], dtype=np.int64)
    tab["n"], tab["start"], tab["first_block"] = n, np.cumsum(n) - n, np.cumsum(blocks_of(n)) - blocks_of(n)
    for k in ("means", "scales", "quats", "opacities", "xys_grad_norm", "vis_counts", "max_2dsize", "seed", "thresholds", "options",
              "far_radius", "far_factor", "phase"):
        tab[k] = [d[k] for d in nodes]
    return tab


def fill_after_scan(tab, counts, n_columns):
    """The host arithmetic after the prefix sums: counts[(n_columns + 1), n_total] -> (incl int64, table with scan_base, col_base,
    n_out, out_start, out_first_block).  A node's unused columns have no survivors, so their bases do not matter."""
    tab = tab.copy()
    incl = np.cumsum(counts.astype(np.int64), axis=1)
    n = tab["n"]
    ends = np.cumsum(n) - 1
    bound = np.where(ends >= 0, incl[:, np.maximum(ends, 0)], 0)           # (an empty first node: nothing before it)
    before = np.concatenate([np.zeros((n_columns + 1, 1), dtype=np.int64), bound[:, :-1]], axis=1)
    tot = (bound - before)[:n_columns]
    n_out = tot.sum(axis=0)
    tab["n_out"], tab["out_start"] = n_out, np.cumsum(n_out) - n_out
    tab["out_first_block"] = np.cumsum(blocks_of(n_out)) - blocks_of(n_out)
    tab["scan_base"][:, :n_columns] = before[:n_columns].T
    tab["col_base"][:, :n_columns] = (np.cumsum(tot, axis=0) - tot).T
    return incl, tab


def move_blocks(n_rows, width):
    return (np.asarray(n_rows, dtype=np.int64) * np.asarray(width, dtype=np.int64) + 3 + MOVE_DWORDS - 1) // MOVE_DWORDS


def move_table(moves):
    """mtgs_refine_move records; moves: dicts with n_rows, out_start, n_src, src, dst, width, op, clamp_max."""
    tab = np.zeros(len(moves), dtype=MOVE)
    for k in ("n_rows", "out_start", "n_src", "src", "dst", "width", "op", "clamp_max"):
        tab[k] = [m[k] for m in moves]
    blocks = move_blocks(tab["n_rows"], tab["width"])
    tab["first_block"] = np.cumsum(blocks) - blocks
    return tab, int(blocks.sum())


# ---- decisions ------------------------------------------------------------------------------------------------------------------------
def ref_config(thresholds, options, step, phase=None):
    """A RefineConfig under which tests/refine_scene_refs.refinement_after applies, at `step`, exactly the rules the kernel applies
    for (thresholds[6], options[5]): a rule the options switch off but the reference's step gating would switch on gets the threshold OFF,
    which no statistic reaches (finite, so that refine_scene_refs.near_rows can still measure a distance from it)."""
    phase = DENSIFY if phase is None else phase
    t = [float(v) for v in thresholds]
    S, screen_split, cull_big, cull_screen, clone = (int(v) for v in options)
    cull_screen = cull_screen and cull_big
    assert step >= 2
    screen = screen_split or cull_screen
    return RefineConfig(refine_every=1, reset_alpha_every=step - 1 if cull_big else step, stop_split_at=step + 1 if phase == DENSIFY else 0,
                        continue_cull_post_densification=True, densify_from_iter=0, stop_screen_size_at=step + 1 if screen else 0,
                        densify_grad_thresh=t[0], densify_size_thresh=t[1], split_screen_size=t[2] if screen_split else OFF,
                        cull_alpha_thresh=t[3], cull_scale_thresh=t[4], cull_screen_size=t[5] if cull_screen else OFF,
                        n_split_samples=S, clone_sample_means=bool(clone))


def refinement(p, stats, thresholds, options, step, seed, rule=(100.0, 40.0), phase=None):
    with np.errstate(all="ignore"):
        return R.refinement_after(p, stats, ref_config(thresholds, options, step, phase), step, seed, rule)


def flags_ref(p, stats, thresholds, options, step, seed, rule=(100.0, 40.0), phase=None, n_columns=MAX_COLUMNS):
    """(flags u8 [N], parents u8 [N], counts i32 [n_columns + 1, N], masks): bit 0 old row kept | bit 1 + s child s kept | bit 1 + S
    duplicate kept | bit 7 split, from the keep / kind / src_index / splits of the restatement."""
    N, S = p["means"].shape[0], int(options[0])
    masks = refinement(p, stats, thresholds, options, step, seed, rule, phase)[2]
    flags = np.zeros(N, dtype=np.uint8)
    np.bitwise_or.at(flags, masks["src_index"], (1 << masks["kind"]).astype(np.uint8))
    flags[masks["splits"]] |= 0x80
    counts = np.zeros((n_columns + 1, N), dtype=np.int32)
    for k in range(2 + S):
        counts[k] = (flags >> k) & 1
    counts[n_columns] = flags >> 7
    return flags, ((flags & 0x7E) != 0).astype(np.uint8), counts, masks


# ---- the row mover --------------------------------------------------------------------------------------------------------------------
def move_ref(src, src_index, kind, op, clamp_max=0.0):
    """dst[r] = op(src[src_index[r]]) on uint32 words; src [n_src, width]."""
    src = np.asarray(src, dtype=np.uint32)
    idx = np.asarray(src_index, dtype=np.int64)
    ok = (idx >= 0) & (idx < src.shape[0])
    out = np.zeros((idx.size, src.shape[1]), dtype=np.uint32)
    if op == ZERO_ALL:
        return out
    out[ok] = src[idx[ok]]
    if op == ZERO_NEW:
        out[np.asarray(kind) != 0] = 0
    if op == CLAMP_MAX:
        x = out.view(F)
        with np.errstate(invalid="ignore"):
            out = np.where(x > F(clamp_max), F(clamp_max), x).view(np.uint32)
    return out


def worst_width(limit=32768):
    """The width w <= limit that maximises (8191 + w) * (magic * w - 2^32), magic = 0xFFFFFFFF // w + 1: the largest quotient error
    q * (magic * w - 2^32) / (w * 2^32) the multiply-high division of refine_scene_rows_kernel ever sees."""
    w = np.arange(2, limit + 1, dtype=np.int64)
    magic = 0xFFFFFFFF // w + 1
    return int(w[np.argmax((8191 + w) * (magic * w - (1 << 32)))])


# the widths given to the row mover: the issue's list and the worst width (tests/test_refine_edge_refs_host.py checks the division)
MOVE_WIDTHS = sorted({1, 2, 3, 4, 5, 7, 8, 45, 48, 8191, 8192, 8193, 32767, 32768, worst_width()})


# ---- the samples ----------------------------------------------------------------------------------------------------------------------
def philox_words(seed, step, index, slot):
    index = np.asarray(index, dtype=np.uint32).reshape(-1)
    c = np.stack([index, np.full_like(index, slot), np.full_like(index, step), np.zeros_like(index)], 1)
    return philox4x32_10(c, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))


def uniforms_f32(seed, step, index, slot):
    """[n, 4] float32: ((float)word + 0.5f) * 2^-32, every operation rounded to float32 -- the kernel's definition."""
    r = philox_words(seed, step, index, slot).astype(F)
    return (r + F(0.5)) * F(2.0 ** -32)


def _rot_abs(w, x, y, z):
    """The rotation entries and, per entry, the sum of the absolute values of the products it is made of."""
    rot = [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
           [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
           [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]
    a = np.abs
    mag = [[1 + 2 * (y * y + z * z), 2 * (a(x * y) + a(w * z)), 2 * (a(x * z) + a(w * y))],
           [2 * (a(x * y) + a(w * z)), 1 + 2 * (x * x + z * z), 2 * (a(y * z) + a(w * x))],
           [2 * (a(x * z) + a(w * y)), 2 * (a(y * z) + a(w * x)), 1 + 2 * (x * x + y * y)]]
    return rot, mag


def sample_ref64(means, scales, quats, u, shrunk=False):
    """float64 from the float32 uniforms u [n, 4]: z = Box-Muller(u), mean + R(q / |q|) (exp(s) z) with s = scales, or
    log(exp(scales) / 1.6) where `shrunk` (the duplicate of a split parent), and the shrunk scales log(exp(scales) / 1.6).
    Returns (means, mean terms, shrunk scales, scale terms); terms one level below the components: |m_k| + sum_j A_kj e^{s_j} rho_j
    with rho the Box-Muller RADIUS of the lane (a z near 0 carries rho ulp(2 pi), not a relative error), and |s| + 1."""
    m, s, q, u = (np.asarray(v, dtype=np.float64) for v in (means, scales, quats, u))
    ra, rb = np.sqrt(-2 * np.log(u[:, 0])), np.sqrt(-2 * np.log(u[:, 2]))
    z = np.stack([ra * np.cos(2 * np.pi * u[:, 1]), ra * np.sin(2 * np.pi * u[:, 1]), rb * np.cos(2 * np.pi * u[:, 3])], 1)
    rho = np.stack([ra, ra, rb], 1)
    small = np.log(np.exp(s) / SHRINK)
    spread = np.exp(np.where(np.asarray(shrunk).reshape(-1, 1), small, s))
    qn = q / np.linalg.norm(q, axis=-1, keepdims=True)
    rot, mag = _rot_abs(qn[:, 0], qn[:, 1], qn[:, 2], qn[:, 3])
    out, terms = np.empty_like(m), np.empty_like(m)
    for k in range(3):
        out[:, k] = m[:, k] + sum(rot[k][j] * spread[:, j] * z[:, j] for j in range(3))
        terms[:, k] = np.abs(m[:, k]) + sum(mag[k][j] * spread[:, j] * rho[:, j] for j in range(3))
    return out, terms, small, np.abs(s) + 1.0


def sample_f32(means, scales, quats, u, shrunk=False):
    """The same with every operation rounded to float32, in the order of csrc/refine.hip (refine_normal3, sample_mean, sl_cur).
    Only for measuring SAMPLE_MEANS / SAMPLE_SCALES."""
    m, s, q, u = (np.asarray(v, dtype=F) for v in (means, scales, quats, u))
    one, two, tau = F(1), F(2), F(6.283185307179586)
    ra = np.sqrt(F(-2) * np.log(np.maximum(u[:, 0], F(1e-37))))
    rb = np.sqrt(F(-2) * np.log(np.maximum(u[:, 2], F(1e-37))))
    z = [ra * np.cos(tau * u[:, 1]), ra * np.sin(tau * u[:, 1]), rb * np.cos(tau * u[:, 3])]
    small = np.log(np.exp(s) / F(SHRINK))
    sl = np.where(np.asarray(shrunk).reshape(-1, 1), small, s)
    inv = one / np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
    w, x, y, zz = q[:, 0] * inv, q[:, 1] * inv, q[:, 2] * inv, q[:, 3] * inv
    v0, v1, v2 = np.exp(sl[:, 0]) * z[0], np.exp(sl[:, 1]) * z[1], np.exp(sl[:, 2]) * z[2]
    out = np.stack([m[:, 0] + (one - two * (y * y + zz * zz)) * v0 + two * (x * y - w * zz) * v1 + two * (x * zz + w * y) * v2,
                    m[:, 1] + two * (x * y + w * zz) * v0 + (one - two * (x * x + zz * zz)) * v1 + two * (y * zz - w * x) * v2,
                    m[:, 2] + two * (x * zz - w * y) * v0 + two * (y * zz + w * x) * v1 + (one - two * (x * x + y * y)) * v2], 1)
    assert out.dtype == F and small.dtype == F
    return out, small


def geometry_ref(p, src_index, kind, splits, S, clone, seed, step):
    """out_means / out_scales of the output rows (src_index, kind) of one node: (means, mean terms, scales, scale terms, sampled
    [n_out] bool, shrunk [n_out] bool).  Rows that are not sampled / not shrunk are BIT COPIES: their value is the float32 input and
    their terms are 0 (worst_ratio then asks for equality)."""
    src, kind = np.asarray(src_index), np.asarray(kind)
    m, s, q = p["means"][src], p["scales"][src], p["quats"][src]
    child = (kind >= 1) & (kind <= S)
    dup = kind == 1 + S
    sampled = child | (dup & bool(clone))
    shrunk = np.asarray(splits)[src] & (kind != 0)          # children, and the duplicate of a split parent
    u = np.zeros((src.size, 4), dtype=F)
    for k in range(1, 2 + S):
        rows = kind == k
        u[rows] = uniforms_f32(seed, step, src[rows], k - 1)
    u[~sampled] = 0.5
    sm, smt, small, smallt = sample_ref64(m, s, q, u, shrunk & dup)
    means = np.where(sampled[:, None], sm, m.astype(np.float64))
    mterms = np.where(sampled[:, None], smt, 0.0)
    scales = np.where(shrunk[:, None], small, s.astype(np.float64))
    sterms = np.where(shrunk[:, None], smallt, 0.0)
    return means, mterms, scales, sterms, sampled, shrunk


# ---- the inputs of the GPU precision test ---------------------------------------------------------------------------------------------
# Philox word 0 of (seed, UNIT_RA_STEP, index 0, slot 0) is 4294967283: its float32 uniform is exactly 1.0, ra = 0, the child is
# displaced along the third axis only.  Word 2 of (seed, UNIT_RB_STEP, 0, 0) likewise: rb = 0, the first two axes only.
PRECISION_SEED = 1234567
UNIT_RA_STEP, UNIT_RB_STEP = 6276890, 2569880
PRECISION_N = 257
PRECISION_S = 2
PRECISION_STEPS = (UNIT_RA_STEP, UNIT_RB_STEP)
PRECISION_KINDS = ("old", "child", "dup")
# thresholds: grad, size, split screen, alpha, cull scale, cull screen -- nothing is culled but the split parents, and cull_big is off
_PRECISION_THRESHOLDS = {"old": (0.5, 0.005, 100.0, 0.005, 0.5, 150.0), "child": (0.5, 0.005, 100.0, 0.005, 0.5, 150.0),
                         "dup": (0.5, 1000.0, 100.0, 0.005, 0.5, 150.0)}


@lru_cache(maxsize=None)
def precision_node(which):
    """257 rows that all become `which`: "old" (gradient below the threshold), "child" (all split, two samples) or "dup" (all
    duplicated; the odd rows are split by screen size first, so that their duplicate takes the shrunk scales and they have children
    too).  Quaternion norms 1e-3 .. 1e3, exp(scale) 0.01 .. 800, row 0 identity-rotated at the origin with unit scales.
    Returns (params, stats, thresholds, options without clone_sample_means)."""
    g = np.random.default_rng({"old": 71, "child": 72, "dup": 73}[which])
    N = PRECISION_N
    f = lambda a: np.ascontiguousarray(a, dtype=F)
    q = g.standard_normal((N, 4))
    q = q / np.linalg.norm(q, axis=-1, keepdims=True) * 10.0 ** g.uniform(-3, 3, (N, 1))
    scales = np.log(0.01) + g.random((N, 3)) * (np.log(800.0) - np.log(0.01))
    means = (g.random((N, 3)) * 2 - 1) * np.array([60.0, 8.0, 140.0])
    means[0], scales[0], q[0] = 0.0, 0.0, (1.0, 0.0, 0.0, 0.0)
    p = {"means": f(means), "scales": f(scales), "quats": f(q), "opacities": f(np.full((N, 1), 3.0))}
    high = which != "old"
    m2 = np.zeros(N)
    if which == "dup":
        m2[1::2] = 120.0
    stats = (f(np.full(N, 4.0 if high else 0.0)), f(np.full(N, 2.0)), f(m2))
    return p, stats, _PRECISION_THRESHOLDS[which], (PRECISION_S, int(which == "dup"), 0, 0)


def precision_cases():
    """[(which, clone, step)] of the GPU precision test"""
    return [(w, c, s) for w in PRECISION_KINDS for c in (1, 0) for s in PRECISION_STEPS]


def precision_reference(which, clone, step):
    """(params, stats, thresholds, options, masks, geometry_ref(...)) of one precision case"""
    p, stats, th, opt = precision_node(which)
    opt = opt + (clone,)
    masks = refinement(p, stats, th, opt, step, PRECISION_SEED)[2]
    geo = geometry_ref(p, masks["src_index"], masks["kind"], masks["splits"], PRECISION_S, clone, PRECISION_SEED, step)
    return p, stats, th, opt, masks, geo


def measure_constants():
    """{"means": worst |sample_f32 - sample_ref64| / (2^-24 terms), "scales": ...} over the rows of precision_cases()"""
    worst = {"means": 0.0, "scales": 0.0}
    for which, clone, step in precision_cases():
        p, _, _, opt, masks, (means, mterms, scales, sterms, sampled, shrunk) = precision_reference(which, clone, step)
        src, kind = masks["src_index"], masks["kind"]
        u = np.zeros((src.size, 4), dtype=F)
        for k in range(1, 2 + PRECISION_S):
            u[kind == k] = uniforms_f32(PRECISION_SEED, step, src[kind == k], k - 1)
        u[~sampled] = 0.5
        dup_shrunk = shrunk & (kind == 1 + PRECISION_S)
        m32, s32 = sample_f32(p["means"][src], p["scales"][src], p["quats"][src], u, dup_shrunk)
        if sampled.any():
            worst["means"] = max(worst["means"], worst_ratio(m32[sampled], means[sampled], mterms[sampled]))
        if shrunk.any():
            worst["scales"] = max(worst["scales"], worst_ratio(s32[shrunk], scales[shrunk], sterms[shrunk]))
    return worst


# ---- the option nodes of the classify test --------------------------------------------------------------------------------------------
OPTION_STEP = 4000
OPTION_SEED = 777
OPTION_THRESHOLDS = (0.004, 0.6, 100.0, 0.005, 0.1, 150.0)
# n_split_samples 2; options 1 to 4 (split by screen | cull by world size | cull by screen size | clone_sample_means), each toggled
# alone from "all off" and from "all on" (option 3 does nothing without option 2; option 4 changes a flag only under option 2, where
# the duplicate is culled at its drawn position)
def _toggled(base):
    return [tuple(base)] + [tuple(b ^ (i == j) for j, b in enumerate(base)) for i in range(4)]


OPTION_SETS = tuple((2,) + o for o in _toggled((0, 0, 0, 0)) + _toggled((1, 1, 1, 1)))


OPTION_PLANTED = 24


@lru_cache(maxsize=None)
def option_node():
    """64 rows (refine_scene_refs.clean_node) with no decision within 2 * MARGIN of its threshold under any of OPTION_SETS.  The first
    24 lie 0.21 .. 0.5 inside or outside the far radius with a size between the near and the far limit, so that a sample drawn on
    the other side of the radius is culled and one on the parent's side is not: rows 0-7 split (their children are spread by the
    ORIGINAL scales, about 1), rows 8-23 are duplicated (option 4 shows in the flags).  The first seed whose draw is clean and
    has a child and a duplicate across the radius is taken -- chosen here, on the CPU."""
    combos = [(ref_config(OPTION_THRESHOLDS, o, OPTION_STEP), OPTION_STEP, True) for o in OPTION_SETS]
    base = R.clean_node(64, 31, combos, OPTION_SEED)
    K = OPTION_PLANTED
    for seed in range(31, 61):
        g = np.random.default_rng(seed)
        p, stats = {k: v.copy() for k, v in base[0].items()}, tuple(v.copy() for v in base[1])
        p["opacities"][:K] = 2.0
        stats[0][:K], stats[1][:K], stats[2][:K] = 0.5, 2.0, 7.0
        side = np.zeros(K)
        bad = np.arange(64) < K
        for _ in range(200):                               # draw the planted rows that are near a threshold again, as clean_node does
            for i in np.flatnonzero(bad):
                d = g.standard_normal(3)
                side[i] = g.choice([-1.0, 1.0])
                p["means"][i] = (d / np.linalg.norm(d) * (100.0 + side[i] * g.uniform(0.21, 0.5))).astype(F)
                p["scales"][i] = np.log(g.uniform(0.9, 1.5, 3) if i < 8 else g.uniform(0.3, 0.55, 3)).astype(F)
            bad = np.zeros(64, bool)
            for o in OPTION_SETS:
                bad |= R.near_rows(refinement(p, stats, OPTION_THRESHOLDS, o, OPTION_STEP, OPTION_SEED), 64, 2 * R.MARGIN)
            assert not bad[K:].any()
            if not bad.any():
                break
        else:
            continue
        on, off = (flags_ref(p, stats, OPTION_THRESHOLDS, (2, 1, 1, 1, c), OPTION_STEP, OPTION_SEED)[0] for c in (1, 0))
        far = side[:8] > 0                                 # a child of a far parent culled, a child of a near parent kept
        if (on[8:K] != off[8:K]).any() and ((on[:8][far] & 6) != 6).any() and ((on[:8][~far] & 6) != 0).any():
            return p, stats
    raise AssertionError("no clean draw")


# ---- the node table of the classify / index / geometry tests ----------------------------------------------------------------------
TABLE_N = (0, 1, 255, 256, 257, 0)
TABLE_S = (1, 2, 4, 3, 1, 2)
TABLE_STEP = 4000
TABLE_COLUMNS = 6


def table_options(i):
    return (TABLE_S[i], 1, 1, 1, int(i % 2 == 0))


def table_thresholds(i):
    return (0.001 * (1 + 0.1 * i), 0.2 + 0.02 * (i % 3), 100.0, 0.005 + 0.001 * (i % 2), 0.5, 150.0)


@lru_cache(maxsize=None)
def table_nodes():
    """[(params, stats, thresholds, options, seed)]: an empty node first and last; every decision at least 2 * MARGIN from its threshold"""
    out = []
    for i, N in enumerate(TABLE_N):
        th, opt, seed = table_thresholds(i), table_options(i), 9000 + 13 * i + (i << 35)
        p, stats, _, _ = R.clean_node(N, 60 + i, [(ref_config(th, opt, TABLE_STEP), TABLE_STEP, True)], seed)
        out.append((p, stats, th, opt, seed))
    return out


# ---- one node per comparison, at equality -----------------------------------------------------------------------------------------------
EQ_N, EQ_STEP, EQ_SEED = 8, 4000, 4242
# rule -> (decisions of refinement_after that sit at equality, what is varied: an index into thresholds or "far_radius",
#          the flag byte of all eight rows at equality -- WRITTEN OUT BY HAND: bit 0 old kept, bits 1-2 children, bit 3 duplicate,
#          bit 7 split -- and what the rule decides there)
EQ_RULES = {
    "avg_grad":       (("avg_grad",), 0, 0x01, "0.75 / 3 > 0.25 is false: not high, no duplicate"),
    "size_split":     (("size_split", "size_dup"), 1, 0x09, "exp(0) > 1 is false: no split (and the duplicate below)"),
    "screen_split":   (("screen_split",), 2, 0x01, "37 > 37 is false: no split"),
    "size_dup":       (("size_split", "size_dup"), 1, 0x09, "exp(0) <= 1 is true: duplicate"),
    "alpha":          (("alpha",), 3, 0x01, "sigmoid(0) < 0.5 is false: kept"),
    "far_radius":     (("norm",), "far_radius", 0x00, "|(100, 0, 0)| > 100 is false: near, limit 0.5 < exp(0), culled"),
    "size_cull_near": (("size_cull_near",), 4, 0x01, "exp(0) > 1 * 1 is false: kept"),
    "size_cull_far":  (("size_cull_far",), 4, 0x01, "exp(0) > 2 * 0.5 is false: kept"),
    "screen_cull":    (("screen_cull",), 5, 0x01, "37 > 37 is false: kept"),
}


@lru_cache(maxsize=None)
def equality_node(rule):
    """(params, stats, thresholds, options, (far_radius, far_factor)) of the eight-row node of `rule`: the compared value equals the
    threshold in float64 and in any correct float32 evaluation; every other decision is far from its threshold."""
    g = np.random.default_rng(sorted(EQ_RULES).index(rule))
    N = EQ_N
    f = lambda a: np.ascontiguousarray(a, dtype=F)
    th = [0.001, 0.2, 100.0, 0.005, 0.5, 150.0]
    opt, far = [2, 0, 0, 0, 0], (1000.0, 40.0)
    means = np.zeros((N, 3))
    means[:, 0] = 1.0 + np.arange(N)
    small = np.log(g.uniform(0.01, 0.1, (N, 3)))                   # exp far below every size threshold
    unit = np.concatenate([np.zeros((N, 1)), np.log(g.uniform(0.05, 0.3, (N, 2)))], 1)     # max exp(scale) = exp(0)
    scales, opac = small, np.full((N, 1), 3.0)
    gn, vc, m2 = np.zeros(N), np.full(N, 3.0), np.full(N, 5.0)     # not high
    if rule == "avg_grad":
        gn[:], th[0] = 0.75, 0.25
    elif rule in ("size_split", "size_dup"):
        scales, gn[:], th[1] = unit, 9.0, 1.0
    elif rule == "screen_split":
        m2[:], th[2], opt[1] = 37.0, 37.0, 1
    elif rule == "alpha":
        opac[:], th[3] = 0.0, 0.5
    elif rule == "far_radius":
        means[:, 0], scales, opt[2], far = 100.0, unit, 1, (100.0, 40.0)
    elif rule == "size_cull_near":
        scales, opt[2], th[4] = unit, 1, 1.0
    elif rule == "size_cull_far":
        means[:, 0], scales, opt[2], far = 200.0 + np.arange(N), unit, 1, (100.0, 2.0)
    elif rule == "screen_cull":
        m2[:], th[5], opt[2], opt[3] = 37.0, 37.0, 1, 1
    else:
        raise KeyError(rule)
    p = {"means": f(means), "scales": f(scales), "quats": f(g.standard_normal((N, 4))), "opacities": f(opac)}
    return p, (f(gn), f(vc), f(m2)), tuple(float(F(v)) for v in th), tuple(opt), far


def equality_variants(rule):
    """[(tag, thresholds, (far_radius, far_factor))]: the varied threshold at the value, one float32 ulp below it and one above"""
    _, _, th, _, far = equality_node(rule)
    what = EQ_RULES[rule][1]
    out = []
    for tag, to in (("equal", None), ("below", -np.inf), ("above", np.inf)):
        t, fr = list(th), list(far)
        if what == "far_radius":
            fr[0] = float(F(fr[0]) if to is None else np.nextafter(F(fr[0]), F(to)))
        else:
            t[what] = float(F(t[what]) if to is None else np.nextafter(F(t[what]), F(to)))
        out.append((tag, tuple(t), tuple(fr)))
    return out


def zero_visibility_node():
    """vis_counts = 0: rows 0-3 with gradient 0 (0 / 0 = NaN: not high), rows 4-7 with a gradient (x / 0 = inf: high -> duplicate).
    (params, stats, thresholds, options, flags written out by hand)"""
    p, stats, th, opt, _ = equality_node("avg_grad")
    gn = np.array([0, 0, 0, 0, 0.5, 1e-30, 3.0, 1e30], dtype=F)
    return p, (gn, np.zeros(EQ_N, dtype=F), stats[2]), th, opt, np.array([1, 1, 1, 1, 9, 9, 9, 9], dtype=np.uint8)
