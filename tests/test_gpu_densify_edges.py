"""The densification kernels (csrc/stats.hip, csrc/refine.hip) called directly through the C ABI at the sizes, thresholds and addresses
where they branch, against the NumPy references of tests/refine_edge_refs.py (whose own claims tests/test_refine_edge_refs_host.py
checks without a GPU).

The canary rule of tests/test_gpu_bin_edges.py holds for every call: every output has slack behind it (the row mover's destinations
in front of them too) and is pre-filled with one bit pattern; a test asserts what was written AND that everything else still holds
the pattern.  A pointer the contract calls "not followed" gets a POISON buffer of +inf, never null: read, it would flip the decision.
No test passes arguments meant to make a kernel read or write outside what it was given.

Which test reaches which kernel and branch:
  densify_stats_kernel          test_stats_single: n = 1, one block - 1, one block, one block + 1, two blocks + 1; radii -1 / 0 (invisible: the
                                bits stay, NaN payloads included), 1, 2^24 + 1 (the float conversion rounds); max_2dsize below, at and
                                above the radius; three accumulated steps
  densify_stats_batch_kernel    test_stats_batch: the binary search over first_block with an empty node first, in the middle and last;
                                bit-equal to the single-node kernel
  densify_stats_rows_kernel     test_stats_rows: n_vis 0 / 1 / 256 / 257, col 0 and 2, row_stride 4 / 16 / 17; ids before the first node, in
                                a gap (an empty node's start), behind the last node; n_vis_dev null, below the capacity, above it
                                (clamped); test_stats_rows_refuses: row_stride 3 and col 1
  refine_scene_classify_kernel  test_classify_at_equality: every comparison (average gradient, size split, screen split, size duplicate,
                                alpha, far radius, world size near and far, screen cull) with its threshold at the value, one ulp below
                                and one above; test_classify_zero_visibility: 0 / 0 and x / 0; test_classify_cull_only: the phase that
                                follows no statistics pointer; test_classify_table: find_node over first_block with empty nodes first and
                                last, n_split_samples 1 .. 4 under n_columns = 6 (unused columns zero, the split row at n_columns),
                                parents null and non-null, every node identical to itself alone; test_classify_options: options 1 - 4,
                                the children's and the duplicate's cull at their DRAWN position
  refine_scene_index_kernel     test_index_and_geometry_table: the reference order (old, children sample-major, duplicates) per node, nothing
                                outside [out_start, out_start + n_out); a scan_base raised by 3: `local < 0` writes nothing
  refine_scene_geometry_kernel  test_index_and_geometry_table (find_node over out_first_block, a src_index that is no row: nothing written);
                                test_geometry_precision: old rows, children, duplicates of unsplit and of split parents, clone_sample_means
                                on and off, a uniform of exactly 1.0 in either radius, against float64 within device_bound
  refine_scene_rows_kernel      test_rows_widths: width 1 (no multiply-high) .. 32768 and the worst width of the division; destination and
                                source 0 - 3 dwords behind a 16-byte boundary (the shifted dwordx4 store, the dwordx4 / dword gather);
                                totals around 1, 4, 5, one and two workgroups minus the pad; the four ops; indices that are no row;
                                CLAMP_MAX over NaN, +-inf, -0.0 and the clamp itself; test_rows_twelve_moves: the binary search over
                                first_block with one-row moves beside three-workgroup moves"""
import functools

import numpy as np
import pytest
import torch

from tests import refine_edge_refs as E
from tests.test_gpu_bin_edges import CAN, SL, _call, _st, can, host, up

pytestmark = pytest.mark.gpu

F = np.float32
EINVAL = 1
CANB = np.frombuffer(np.int32(CAN).tobytes(), dtype=np.uint8)
MEANS_BOUND, SCALES_BOUND = E.device_bound(E.SAMPLE_MEANS), E.device_bound(E.SAMPLE_SCALES)
WORST = {}                                               # quantity -> largest got / bound of this session (printed by the tests)


# ---- helpers --------------------------------------------------------------------------------------------------------------------------
def fcan(n):
    return can(int(n) + SL).view(torch.float32)


def bcan(n):
    """n bytes and at least SL words behind them, every word the canary"""
    return can((int(n) + 3) // 4 + SL).view(torch.uint8)


def words(t):
    return host(t.contiguous().view(torch.int32))


def tail_is_canary(t, n):
    """everything behind the first n elements of a 4-byte tensor"""
    return bool((words(t)[int(n):] == CAN).all())


def bytes_are_canary(h, lo, hi):
    return bool((h[lo:hi] == CANB[np.arange(lo, hi) % 4]).all())


def fup(a):
    return up(np.ascontiguousarray(a, dtype=F))


def table(tab):
    return torch.from_numpy(tab.view(np.uint8).reshape(-1).copy()).cuda()


def rc_of(name, *a):
    from mtgs_amd import _lib
    return getattr(_lib.load(), name)(*a)


@functools.lru_cache(maxsize=None)
def poison():
    return torch.full((4096,), float("inf"), dtype=torch.float32, device="cuda")


def note(what, ratio):
    WORST[what] = max(WORST.get(what, 0.0), float(ratio))
    print(f"got / bound: {what} {ratio:.4f} (largest so far {WORST[what]:.4f})")


# ---- the statistics -------------------------------------------------------------------------------------------------------------------
W_IMG, H_IMG = 1001, 751                                 # half sizes 500.5 and 375.5: exact in float32, no power of two
RADII = np.array([-1, 0, 1, (1 << 24) + 1, 37, 5, -7, 2], dtype=np.int32)


def stats_init(r0, g):
    """The three arrays before the first step: arbitrary BIT PATTERNS (NaN payloads among them) where the element is invisible,
    numbers where it is visible, max_2dsize below, at and above the first radius."""
    n, vis = r0.size, r0 > 0
    junk = lambda: g.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    junk_nan = junk()
    junk_nan[::3] = 0x7FC12345
    gn = np.where(vis, (g.random(n) * 3).astype(F).view(np.uint32), junk_nan).view(F)
    vc = np.where(vis, g.integers(0, 9, n).astype(F).view(np.uint32), junk()).view(F)
    m2 = np.where(vis, (r0.astype(F) + g.integers(-1, 2, n).astype(F)).view(np.uint32), junk()).view(F)
    return gn, vc, m2


def stats_inputs(n, seed, steps=3):
    """radii per step (the same elements visible in every step, with other sizes), gradients per step, the arrays before the first
    step and the visibility"""
    g = np.random.default_rng(seed)
    r0 = RADII[(np.arange(n) + seed) % RADII.size]
    vis = r0 > 0
    radii = [r0] + [np.where(vis, np.roll(RADII[RADII > 0], t)[np.arange(n) % 5], r0).astype(np.int32) for t in range(1, steps)]
    grads = [(g.standard_normal((n, 2)) * 10.0 ** g.uniform(-6, 1, (n, 1))).astype(F) for _ in range(steps)]
    return radii, grads, stats_init(r0, g), vis


def stats_ref(radii, grads, init, vis):
    """float64 sums with their bound 2^-24 (3 |g| + |acc|) per step -- two roundings of the products, the sum and the root for g, one
    rounding of the accumulate -- and the exact counts and maxima; an invisible element keeps its bits."""
    gn, vc, m2 = init
    acc = np.where(vis, gn.astype(np.float64), 0.0)
    bound = np.zeros_like(acc)
    cnt, mx = np.where(vis, vc, F(0)), np.where(vis, m2, F(0))
    for r, g2 in zip(radii, grads):
        g = np.hypot(g2[:, 0].astype(np.float64) * (0.5 * W_IMG), g2[:, 1].astype(np.float64) * (0.5 * H_IMG))
        acc = np.where(vis, acc + g, acc)
        bound += np.where(vis, E.EPS * (3 * g + np.abs(acc)), 0.0)
        cnt = np.where(vis, cnt + F(1), cnt)
        mx = np.where(vis, np.maximum(mx, r.astype(F)), mx)
    return acc, bound, cnt, mx


def check_stats(where, outs, n, init, vis, acc, bound, cnt, mx):
    gn, vc, m2 = (host(t) for t in outs)
    for t in outs:
        assert tail_is_canary(t, n), f"{where}: wrote behind an output"
    hid = ~vis
    for got, was in zip((gn, vc, m2), init):
        assert np.array_equal(got[:n].view(np.uint32)[hid], was.view(np.uint32)[hid]), f"{where}: an invisible element changed"
    assert np.array_equal(vc[:n][vis], cnt[vis]) and np.array_equal(m2[:n][vis], mx[vis]), where
    err = np.abs(gn[:n].astype(np.float64) - acc)[vis]
    assert (err <= bound[vis]).all(), (where, float((err / bound[vis]).max()))
    if vis.any():
        note("xys_grad_norm", (err / bound[vis]).max())


def with_canary(a):
    t = fcan(a.size)
    t[:a.size] = up(a.view(np.int32)).view(torch.float32)
    return t


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_stats_single(hip_lib, n):
    assert np.float32((1 << 24) + 1) == 1 << 24
    for seed in ((0, 3) if n == 1 else (0,)):            # n = 1: an invisible and a visible element
        radii, grads, init, vis = stats_inputs(n, seed)
        outs = [with_canary(a) for a in init]
        for r, g in zip(radii, grads):
            d_r, d_g = up(r), fup(g)
            _call("mtgs_densify_stats", n, d_r.data_ptr(), d_g.data_ptr(), W_IMG, H_IMG, *(t.data_ptr() for t in outs), _st())
        check_stats(f"n={n} seed={seed}", outs, n, init, vis, *stats_ref(radii, grads, init, vis))
        assert vis.any() or n == 1


BATCH_SIZES = (0, 1, 255, 0, 256, 257, 0)


def test_stats_batch(hip_lib):
    """An empty node first, in the middle and last (their pointers are poison); every node bit-equal to the single-node kernel on
    its slice and within the bound of float64; canaries behind every node's arrays."""
    lead = 3                                             # the nodes' rows start behind three rows of no node
    n_all = lead + sum(BATCH_SIZES)
    radii, grads, _, _ = stats_inputs(n_all, 1, steps=2)
    starts = lead + np.cumsum(BATCH_SIZES) - np.array(BATCH_SIZES)
    per_node = []                                        # (arrays before the first step, visibility): the collected arrays' on the node's slice
    for j, (n, s) in enumerate(zip(BATCH_SIZES, starts)):
        r0 = radii[0][s:s + n]
        per_node.append((stats_init(r0, np.random.default_rng(10 + j)), r0 > 0))
    outs = [[with_canary(a) for a in init] if n else None for (init, _), n in zip(per_node, BATCH_SIZES)]
    single = [[with_canary(a) for a in init] if n else None for (init, _), n in zip(per_node, BATCH_SIZES)]
    ptrs = [[t.data_ptr() for t in o] if o else [poison().data_ptr()] * 3 for o in outs]
    tab = E.stats_table(BATCH_SIZES, starts, ptrs)
    assert tab["first_block"].tolist() == [0, 0, 1, 2, 2, 3, 5]
    d_tab = table(tab)
    for r, g in zip(radii, grads):
        d_r, d_g = up(r), fup(g)
        _call("mtgs_densify_stats_batch", len(BATCH_SIZES), d_tab.data_ptr(), 5, d_r.data_ptr(), d_g.data_ptr(), W_IMG, H_IMG, _st())
        for o, n, s in zip(single, BATCH_SIZES, starts):
            if n:
                _call("mtgs_densify_stats", n, d_r[s:].data_ptr(), d_g[s:].data_ptr(), W_IMG, H_IMG, *(t.data_ptr() for t in o), _st())
    assert bool(torch.isinf(poison()).all())
    for j, (n, s) in enumerate(zip(BATCH_SIZES, starts)):
        if not n:
            continue
        init, vis = per_node[j]
        sl = [[r[s:s + n] for r in radii], [g[s:s + n] for g in grads]]
        assert all(np.array_equal(a > 0, vis) for a in sl[0])
        check_stats(f"node {j}", outs[j], n, init, vis, *stats_ref(sl[0], sl[1], init, vis))
        for a, b in zip(outs[j], single[j]):
            assert np.array_equal(words(a), words(b)), f"node {j}: the batch differs from the single-node kernel"


ROWS_NODES = ((10, 40), (50, 0), (60, 300))              # (start, n): ten rows before the first node, an empty node, a gap behind it
ROWS_TOTAL = 400


def rows_ids(n_vis, seed):
    """n_vis DIFFERENT flat ids: of a node, and -- from four rows on -- before the first node, in the gap and behind the last node"""
    g = np.random.default_rng(seed)
    valid = np.concatenate([np.arange(s, s + n) for s, n in ROWS_NODES])
    alien = np.array([3, 55, 380, 0, 50, 59, 360, 399, 9])
    ids = np.concatenate([alien[:min(len(alien), n_vis // 4)], g.permutation(valid)])[:n_vis]
    return g.permutation(ids).astype(np.int32)


@pytest.mark.parametrize("row_stride", [4, 16, 17])
@pytest.mark.parametrize("col", [0, 2])
@pytest.mark.parametrize("n_vis", [0, 1, 256, 257])
def test_stats_rows(hip_lib, n_vis, col, row_stride):
    """The compact rows against float64 and, bit for bit, against the batch kernel on the scattered dense gradient.  Every radius is
    positive, so an id that belongs to no node or lies behind the device count would be counted if it were followed."""
    g = np.random.default_rng(n_vis * 100 + col * 10 + row_stride)
    cap = max(n_vis, 1)
    radii = g.integers(1, 200, ROWS_TOTAL).astype(np.int32)
    rows = (g.standard_normal((cap, row_stride)) * 10.0 ** g.uniform(-6, 1, (cap, 1))).astype(F)
    inits = [stats_init(radii[s:s + n], g) if n else None for s, n in ROWS_NODES]          # (every radius is positive: numbers everywhere)
    d_radii, d_rows = up(radii), with_canary(rows.reshape(-1))
    packed = lambda c: up(np.array([(c << 32) | 0xFFFFFFFF], dtype=np.int64))
    id_sets = [rows_ids(n_vis, 7)] if n_vis != 1 else [np.array([v], dtype=np.int32) for v in (77, 3, 55, 380)]
    for ids in id_sets:
        for count in (None, n_vis // 2, n_vis + 5):
            live = n_vis if count is None else min(count, n_vis)
            outs = [[with_canary(a) for a in init] if init else None for init in inits]
            dense = [[with_canary(a) for a in init] if init else None for init in inits]
            ptrs = lambda o: [[t.data_ptr() for t in x] if x else [poison().data_ptr()] * 3 for x in o]
            starts, sizes = [s for s, _ in ROWS_NODES], [n for _, n in ROWS_NODES]
            d_ids = up(np.concatenate([ids, np.zeros(1, np.int32)]))            # (never null, n_vis = 0 included)
            dev_count = None if count is None else packed(count)
            t_rows, t_dense = table(E.stats_table(sizes, starts, ptrs(outs), first_block=False)), table(E.stats_table(sizes, starts, ptrs(dense)))
            _call("mtgs_densify_stats_rows", n_vis, d_ids.data_ptr(), d_rows.data_ptr(), row_stride, col, d_radii.data_ptr(), len(ROWS_NODES),
                  t_rows.data_ptr(), W_IMG, H_IMG,
                  None if dev_count is None else dev_count.data_ptr(), _st())
            # the same update through the dense kernels: the gradient scattered, radii 0 where no live row points
            grad = np.zeros((ROWS_TOTAL, 2), dtype=F)
            r_dense = np.zeros(ROWS_TOTAL, dtype=np.int32)
            grad[ids[:live]] = rows[:live, col:col + 2]
            r_dense[ids[:live]] = radii[ids[:live]]
            d_rd, d_gd = up(r_dense), fup(grad)
            _call("mtgs_densify_stats_batch", len(ROWS_NODES), t_dense.data_ptr(), int(E.blocks_of(sizes).sum()), d_rd.data_ptr(),
                  d_gd.data_ptr(), W_IMG, H_IMG, _st())
            for j, (s, n) in enumerate(ROWS_NODES):
                if not n:
                    continue
                vis = r_dense[s:s + n] > 0
                where = f"n_vis={n_vis} count={count} node {j}"
                check_stats(where, outs[j], n, inits[j], vis, *stats_ref([r_dense[s:s + n]], [grad[s:s + n]], inits[j], vis))
                for a, b in zip(outs[j], dense[j]):
                    assert np.array_equal(words(a), words(b)), f"{where}: the rows kernel differs from the batch kernel"
            assert tail_is_canary(d_rows, cap * row_stride) and bool(torch.isinf(poison()).all())


def test_stats_rows_refuses(hip_lib):
    d = can(64)
    args = lambda stride, col: (1, d.data_ptr(), d.data_ptr(), stride, col, d.data_ptr(), 1, d.data_ptr(), W_IMG, H_IMG, None, _st())
    assert rc_of("mtgs_densify_stats_rows", *args(3, 0)) == EINVAL
    assert rc_of("mtgs_densify_stats_rows", *args(4, 1)) == EINVAL
    assert bool((d == CAN).all())


# ---- classify -------------------------------------------------------------------------------------------------------------------------
class Node:
    """One node's inputs on the device.  stats None: the three statistics pointers are poison."""

    def __init__(self, p, stats, thresholds, options, seed, far=(100.0, 40.0), phase=E.DENSIFY, poison_max2d=False):
        self.n = p["means"].shape[0]
        self.keep = [fup(p[k]) if self.n else poison() for k in ("means", "scales", "quats", "opacities")]
        self.stats = [fup(s) for s in stats] if (stats is not None and self.n) else [poison()] * 3
        if poison_max2d:
            self.stats[2] = poison()
        assert self.n <= 1024 or stats is not None
        self.desc = dict(n=self.n, seed=seed, thresholds=thresholds, options=options, far_radius=far[0], far_factor=far[1], phase=phase)
        for k, t in zip(("means", "scales", "quats", "opacities", "xys_grad_norm", "vis_counts", "max_2dsize"), self.keep + self.stats):
            self.desc[k] = t.data_ptr()


def run_classify(nodes, n_columns, step, with_parents=True):
    """(flags u8 [n_total], counts i32 [n_columns + 1, n_total], parents u8 [n_total] | None, table); canaries checked"""
    tab = E.node_table([nd.desc for nd in nodes])
    n_total, blocks = int(tab["n"].sum()), int(E.blocks_of(tab["n"]).sum())
    counts, flags, parents, d_tab = can((n_columns + 1) * n_total + SL), bcan(n_total), bcan(n_total), table(tab)
    _call("mtgs_refine_scene_classify", len(nodes), d_tab.data_ptr(), blocks, n_total, n_columns, step, counts.data_ptr(),
          flags.data_ptr(), parents.data_ptr() if with_parents else None, _st())
    assert tail_is_canary(counts, (n_columns + 1) * n_total), "classify wrote behind counts"
    hf, hp = host(flags), host(parents)
    assert bytes_are_canary(hf, n_total, hf.size), "classify wrote behind flags"
    assert bytes_are_canary(hp, n_total if with_parents else 0, hp.size), "classify wrote behind parents (or into a null parents)"
    assert bool(torch.isinf(poison()).all())
    return hf[:n_total].copy(), host(counts)[:(n_columns + 1) * n_total].reshape(n_columns + 1, n_total).copy(), \
        (hp[:n_total].copy() if with_parents else None), tab


@pytest.mark.parametrize("rule", list(E.EQ_RULES))
def test_classify_at_equality(hip_lib, rule):
    """Eight rows whose compared value is exact in any correct float32 evaluation: only the comparison operator decides."""
    p, stats, _, opt, _ = E.equality_node(rule)
    by_hand = E.EQ_RULES[rule][2]
    for tag, th, far in E.equality_variants(rule):
        want, want_parents, want_counts, _ = E.flags_ref(p, stats, th, opt, E.EQ_STEP, E.EQ_SEED, far, n_columns=4)
        flags, counts, parents, _ = run_classify([Node(p, stats, th, opt, E.EQ_SEED, far)], 4, E.EQ_STEP)
        assert np.array_equal(flags, want), (rule, tag, flags, want)
        assert tag != "equal" or (flags == by_hand).all(), (rule, E.EQ_RULES[rule][3], flags)
        assert np.array_equal(counts, want_counts) and np.array_equal(parents, want_parents), (rule, tag)


def test_classify_zero_visibility(hip_lib):
    p, stats, th, opt, by_hand = E.zero_visibility_node()
    flags, counts, parents, _ = run_classify([Node(p, stats, th, opt, E.EQ_SEED)], 4, E.EQ_STEP)
    assert np.array_equal(flags, by_hand), flags
    assert np.array_equal(parents, (by_hand & 0x7E) != 0) and np.array_equal(counts[3], (by_hand >> 3) & 1)


def test_classify_cull_only(hip_lib):
    """MTGS_REFINE_CULL_ONLY with the screen rule off: no statistics pointer is followed (all three are +inf poison), only column 0
    is ever set, parents is all zero.  With the screen rule on, max_2dsize is the one that is read."""
    p, stats, th, _, seed = E.table_nodes()[4]                   # 257 rows; its decisions are clean under every rule
    kept = {}
    for opt in ((2, 1, 1, 0, 1), (2, 1, 0, 1, 1), (2, 0, 1, 1, 0)):
        want, _, want_counts, _ = E.flags_ref(p, stats, th, opt, E.TABLE_STEP, seed, phase=E.CULL_ONLY)
        screen = opt[2] and opt[3]
        node = Node(p, stats if screen else None, th, opt, seed, phase=E.CULL_ONLY)
        if screen:
            node.desc["xys_grad_norm"] = node.desc["vis_counts"] = poison().data_ptr()
        flags, counts, parents, _ = run_classify([node], E.MAX_COLUMNS, E.TABLE_STEP)
        assert np.array_equal(flags, want) and set(np.unique(flags)) == {0, 1}, opt
        assert np.array_equal(counts, want_counts) and not counts[1:].any() and not parents.any(), opt
        kept[opt] = int(flags.sum())
    assert kept[(2, 0, 1, 1, 0)] < kept[(2, 1, 1, 0, 1)] < kept[(2, 1, 0, 1, 1)], kept      # each rule culls rows of its own


@pytest.mark.parametrize("opt", E.OPTION_SETS, ids=lambda o: "".join(str(v) for v in o))
def test_classify_options(hip_lib, opt):
    """Options 1 to 4 toggled alone from "all off" and from "all on" on one 64-row node whose children and duplicates are culled at
    their drawn positions, some across the far radius from their parent."""
    p, stats = E.option_node()
    want, want_parents, want_counts, _ = E.flags_ref(p, stats, E.OPTION_THRESHOLDS, opt, E.OPTION_STEP, E.OPTION_SEED, n_columns=4)
    unused = not (opt[1] or (opt[2] and opt[3]))          # no rule uses max_2dsize: +inf there must change nothing
    flags, counts, parents, _ = run_classify([Node(p, stats, E.OPTION_THRESHOLDS, opt, E.OPTION_SEED, poison_max2d=unused)], 4, E.OPTION_STEP)
    assert np.array_equal(flags, want), np.flatnonzero(flags != want)
    assert np.array_equal(counts, want_counts) and np.array_equal(parents, want_parents)


@functools.lru_cache(maxsize=None)
def table_nodes_dev():
    return [Node(p, stats, th, opt, seed) for p, stats, th, opt, seed in E.table_nodes()]


def table_reference():
    return [E.flags_ref(p, stats, th, opt, E.TABLE_STEP, seed, n_columns=E.TABLE_COLUMNS) if p["means"].shape[0] else None
            for p, stats, th, opt, seed in E.table_nodes()]


def test_classify_table(hip_lib):
    """n = (0, 1, 255, 256, 257, 0) with 1, 2, 4, 3, 1, 2 split samples under six columns."""
    nodes, ref = table_nodes_dev(), table_reference()
    C = E.TABLE_COLUMNS
    flags, counts, parents, tab = run_classify(nodes, C, E.TABLE_STEP)
    flags2, counts2, none, _ = run_classify(nodes, C, E.TABLE_STEP, with_parents=False)
    assert none is None and np.array_equal(flags, flags2) and np.array_equal(counts, counts2)
    assert tab["first_block"].tolist() == [0, 0, 1, 2, 3, 5]
    for j, (nd, r) in enumerate(zip(nodes, ref)):
        if not nd.n:
            continue
        s, S = int(tab["start"][j]), E.TABLE_S[j]
        sl = slice(s, s + nd.n)
        assert np.array_equal(flags[sl], r[0]) and np.array_equal(parents[sl], r[1]) and np.array_equal(counts[:, sl], r[2]), j
        assert not counts[2 + S:C, sl].any() and np.array_equal(counts[C, sl], flags[sl] >> 7), f"node {j}: an unused column / the split row"
        assert (r[0] & 0x80).any() and (r[0] & 1).any() or nd.n == 1
        alone = run_classify([nd], C, E.TABLE_STEP)
        assert np.array_equal(alone[0], flags[sl]) and np.array_equal(alone[1], counts[:, sl]) and np.array_equal(alone[2], parents[sl]), j


# ---- index and geometry ---------------------------------------------------------------------------------------------------------------
def run_apply(nodes, tab, counts, n_columns, step, flags, raise_scan=None):
    """The prefix sums and the host arithmetic here, then mtgs_refine_scene_apply.  (src_index, kind, out_means, out_scales) on the
    host WITH their slack, and the filled table."""
    incl, tab = E.fill_after_scan(tab, counts, n_columns)
    if raise_scan is not None:
        tab["scan_base"][raise_scan, 0] += 3
    n_total, n_out = int(tab["n"].sum()), int(tab["n_out"].sum())
    src, kind, om, os_ = can(n_out + SL), bcan(n_out), fcan(3 * n_out), fcan(3 * n_out)
    d_flags, d_tab, d_incl = up(flags), table(tab), up(incl)
    _call("mtgs_refine_scene_apply", len(nodes), d_tab.data_ptr(), int(E.blocks_of(tab["n"]).sum()), int(E.blocks_of(tab["n_out"]).sum()),
          n_total, n_out, n_columns, step, d_flags.data_ptr(), d_incl.data_ptr(), src.data_ptr(), kind.data_ptr(), om.data_ptr(),
          os_.data_ptr(), _st())
    h = host(src), host(kind), host(om), host(os_)
    assert (h[0][n_out:] == CAN).all() and bytes_are_canary(h[1], n_out, h[1].size), "apply wrote behind src_index / kind"
    assert tail_is_canary(om, 3 * n_out) and tail_is_canary(os_, 3 * n_out), "apply wrote behind out_means / out_scales"
    return h, tab


def check_geometry(where, p, masks, S, clone, seed, step, got_means, got_scales):
    """out_means / out_scales of one node against geometry_ref: bit copies where nothing is sampled / shrunk, the bounds elsewhere"""
    means, mterms, scales, sterms, sampled, shrunk = E.geometry_ref(p, masks["src_index"], masks["kind"], masks["splits"], S, clone, seed, step)
    src = masks["src_index"]
    assert np.array_equal(got_means[~sampled].view(np.uint32), p["means"][src][~sampled].view(np.uint32)), f"{where}: a mean that is a copy"
    assert np.array_equal(got_scales[~shrunk].view(np.uint32), p["scales"][src][~shrunk].view(np.uint32)), f"{where}: scales that are a copy"
    assert np.isfinite(got_means).all() and np.isfinite(got_scales).all(), where
    rm = E.worst_ratio(got_means[sampled], means[sampled], mterms[sampled]) / MEANS_BOUND
    rs = E.worst_ratio(got_scales[shrunk], scales[shrunk], sterms[shrunk]) / SCALES_BOUND
    if sampled.any():
        note("sample means", rm)
    if shrunk.any():
        note("sample scales", rs)
    assert rm <= 1.0 and rs <= 1.0, (where, rm, rs)


def test_index_and_geometry_table(hip_lib):
    """The table of test_classify_table through the index and geometry kernels: per node the reference order, the sample positions
    within their bound, nothing outside [out_start, out_start + n_out).  Then node 3 with scan_base[0] raised by 3: the first three
    kept old rows have local < 0 and are written nowhere, the others land three rows earlier, so the last three rows of column 0
    are never indexed -- src_index and kind keep the canary there and the geometry kernel, which finds no row, writes nothing."""
    nodes, ref = table_nodes_dev(), table_reference()
    C = E.TABLE_COLUMNS
    flags, counts, _, tab0 = run_classify(nodes, C, E.TABLE_STEP)
    (src, kind, om, os_), tab = run_apply(nodes, tab0, counts, C, E.TABLE_STEP, flags)
    for j, (nd, r) in enumerate(zip(nodes, ref)):
        lo, n_out = int(tab["out_start"][j]), int(tab["n_out"][j])
        if not nd.n:
            assert n_out == 0
            continue
        masks = r[3]
        assert n_out == masks["keep"].sum()
        assert np.array_equal(src[lo:lo + n_out], masks["src_index"]) and np.array_equal(kind[lo:lo + n_out], masks["kind"]), j
        p, _, _, opt, seed = E.table_nodes()[j]
        check_geometry(f"node {j}", p, masks, opt[0], opt[4], seed, E.TABLE_STEP, om[3 * lo:3 * (lo + n_out)].reshape(-1, 3),
                       os_[3 * lo:3 * (lo + n_out)].reshape(-1, 3))
    J = 3
    (src2, kind2, om2, os2), tab2 = run_apply(nodes, tab0, counts, C, E.TABLE_STEP, flags, raise_scan=J)
    lo, old = int(tab["out_start"][J]), int(ref[J][2][0].sum())
    assert old > 6 and tab2["scan_base"][J, 0] == tab["scan_base"][J, 0] + 3
    want_src, want_kind, want_om, want_os = src.copy(), kind.copy(), om.copy(), os_.copy()
    want_src[lo:lo + old - 3], want_kind[lo:lo + old - 3] = src[lo + 3:lo + old], kind[lo + 3:lo + old]
    want_om[3 * lo:3 * (lo + old - 3)], want_os[3 * lo:3 * (lo + old - 3)] = om[3 * (lo + 3):3 * (lo + old)], os_[3 * (lo + 3):3 * (lo + old)]
    want_src[lo + old - 3:lo + old] = CAN
    want_kind[lo + old - 3:lo + old] = CANB[np.arange(lo + old - 3, lo + old) % 4]
    want_om.view(np.int32)[3 * (lo + old - 3):3 * (lo + old)] = CAN
    want_os.view(np.int32)[3 * (lo + old - 3):3 * (lo + old)] = CAN
    assert np.array_equal(src2, want_src) and np.array_equal(kind2, want_kind)
    assert np.array_equal(om2.view(np.int32), want_om.view(np.int32)) and np.array_equal(os2.view(np.int32), want_os.view(np.int32))
    assert not np.isin(src[lo:lo + 3], src2[lo:lo + old - 3]).any()                  # the first three kept old rows are nowhere


@pytest.mark.parametrize("which, clone, step", E.precision_cases(), ids=lambda v: str(v))
def test_geometry_precision(hip_lib, which, clone, step):
    """257 rows of one kind, quaternion norms 1e-3 .. 1e3, exp(scale) 0.01 .. 800, at the two steps whose Philox key gives Gaussian 0,
    sample 0 a uniform of exactly 1.0.  Old rows and unsampled duplicates: bit copies.  Sampled means and shrunk scales: within
    device_bound(SAMPLE_*) x 2^-24 x terms of sample_ref64."""
    p, stats, th, opt, masks, _ = E.precision_reference(which, clone, step)
    nd = Node(p, stats, th, opt, E.PRECISION_SEED)
    C = 2 + E.PRECISION_S
    want = E.flags_ref(p, stats, th, opt, step, E.PRECISION_SEED, n_columns=C)
    flags, counts, _, tab0 = run_classify([nd], C, step)
    assert np.array_equal(flags, want[0]) and np.array_equal(counts, want[2])
    (src, kind, om, os_), tab = run_apply([nd], tab0, counts, C, step, flags)
    n_out = int(tab["n_out"][0])
    assert n_out == masks["keep"].sum() and np.array_equal(src[:n_out], masks["src_index"]) and np.array_equal(kind[:n_out], masks["kind"])
    got_m, got_s = om[:3 * n_out].reshape(-1, 3), os_[:3 * n_out].reshape(-1, 3)
    check_geometry(f"{which} clone={clone} step={step}", p, masks, E.PRECISION_S, clone, E.PRECISION_SEED, step, got_m, got_s)
    if which == "child":                                 # Gaussian 0 (identity rotation, origin, unit scales), sample 0: the child is z itself
        row = int(np.flatnonzero((masks["src_index"] == 0) & (masks["kind"] == 1))[0])
        if step == E.UNIT_RA_STEP:
            assert got_m[row, 0] == 0 and got_m[row, 1] == 0 and abs(got_m[row, 2]) > 0.1, got_m[row]
        else:
            assert got_m[row, 2] == 0 and abs(got_m[row, 0]) + abs(got_m[row, 1]) > 0.1, got_m[row]


# ---- the row mover --------------------------------------------------------------------------------------------------------------------
CLAMP = 0.75
SPECIAL = np.array([0x7FC00001, 0x7F800000, 0xFF800000, 0x80000000, np.array(CLAMP, F).view(np.uint32), np.nextafter(F(CLAMP), F(1)).view(np.uint32),
                    0xFFC12345, np.nextafter(F(CLAMP), F(0)).view(np.uint32)], dtype=np.uint32)
BAD_INDEX = np.array([-1, 0, 2 ** 31 - 1, -2 ** 31], dtype=np.int64)      # (0 stands for n_src)
OPS = (E.COPY, E.ZERO_NEW, E.CLAMP_MAX, E.ZERO_ALL)


def move_totals(pad):
    B = E.MOVE_DWORDS
    return (1, 4, 5, B - pad - 1, B - pad, B - pad + 1, B, 2 * B - pad, 2 * B - pad + 1)


def run_moves(specs, n_src_of, seed):
    """specs: [(width, n_rows, dst pad, src pad, op)].  One launch; every destination lies in ONE arena of canary words, `dst pad`
    dwords behind a 16-byte boundary with at least four canary words in front of and behind it; the sources of a (width, src pad) are
    shared.  Asserts that the whole arena equals move_ref's rows in a sea of canary (a NaN that CLAMP_MAX read must come out a NaN)."""
    g = np.random.default_rng(seed)
    sources, moves, cursor, n_idx = {}, [], 0, 0
    for w, n_rows, dpad, spad, op in specs:
        if (w, spad) not in sources:
            n_src = n_src_of(w)
            a = g.integers(0, 1 << 32, n_src * w, dtype=np.uint64).astype(np.uint32)
            a[:min(a.size, SPECIAL.size)] = SPECIAL[:a.size]
            t = up(np.concatenate([np.zeros(spad, dtype=np.uint32), a]))[spad:]
            assert t.data_ptr() % 16 == 4 * spad
            sources[(w, spad)] = (a.reshape(n_src, w), t)
        start = (cursor + 3) // 4 * 4 + 4 + dpad
        cursor = start + n_rows * w + 4
        moves.append([w, n_rows, start, spad, op, n_idx])
        n_idx += n_rows
    arena = can(cursor + 8)
    assert arena.data_ptr() % 16 == 0
    idx = np.empty(n_idx, dtype=np.int64)
    kind = g.integers(0, 4, n_idx).astype(np.uint8) * (g.random(n_idx) < 0.5)
    want = np.full(cursor + 8, CAN, dtype=np.int32).view(np.uint32)
    nan_ok = np.zeros(cursor + 8, dtype=bool)
    recs = []
    for w, n_rows, start, spad, op, o in moves:
        a, t = sources[(w, spad)]
        n_src = a.shape[0]
        ix = g.integers(0, n_src, n_rows)
        ix[:min(n_rows, SPECIAL.size)] = np.arange(min(n_rows, SPECIAL.size)) % n_src      # the rows that begin with the special values
        bad = g.random(n_rows) < (0.08 if n_rows > 1 else 0.25)
        ix[bad] = np.where(BAD_INDEX == 0, n_src, BAD_INDEX)[g.integers(0, 4, int(bad.sum()))]
        idx[o:o + n_rows] = ix
        ref = E.move_ref(a, ix, kind[o:o + n_rows], op, CLAMP).reshape(-1)
        want[start:start + ref.size] = ref
        if op == E.CLAMP_MAX:
            nan_ok[start:start + ref.size] = np.isnan(ref.view(F))
        recs.append(dict(n_rows=n_rows, out_start=o, n_src=n_src, src=t.data_ptr(), dst=arena.data_ptr() + 4 * start, width=w, op=op,
                         clamp_max=CLAMP))
    tab, blocks = E.move_table(recs)
    d_idx, d_kind, d_tab = up(idx.astype(np.int32)), up(kind), table(tab)
    _call("mtgs_refine_scene_rows", len(recs), d_tab.data_ptr(), blocks, d_idx.data_ptr(), d_kind.data_ptr(), _st())
    got = host(arena).view(np.uint32)
    assert np.isnan(got.view(F)[nan_ok]).all(), "CLAMP_MAX turned a NaN into a number"
    diff = np.flatnonzero((got != want) & ~nan_ok)
    if diff.size:
        at = int(diff[0])
        mv = max((m for m in moves if m[2] - 8 <= at), key=lambda m: m[2])
        raise AssertionError(f"{diff.size} words differ, the first at arena word {at}: got {got[at]:#x}, want {want[at]:#x}; move "
                             f"(width, rows, start, src pad, op, idx) = {mv}, word {at - mv[2]} of it")
    for a, t in sources.values():
        assert np.array_equal(host(t).view(np.uint32), a.reshape(-1)), "a source changed"
    return tab, blocks


@pytest.mark.parametrize("w", E.MOVE_WIDTHS)
def test_rows_widths(hip_lib, w):
    """Every destination pad x source pad x total x op of one width in one launch.  Wide rows take the nearest row count, and one, two
    and three rows: the largest move is 3 x 32768 dwords."""
    specs = []
    for dpad in range(4):
        rows = sorted({max(1, int(round(t / w))) for t in move_totals(dpad)} | ({1, 2, 3} if w >= 8191 else set()))
        for spad in range(4):
            for op in OPS:
                specs += [(w, r, dpad, spad, op) for r in rows]
    assert max(s[1] * w for s in specs) <= 3 * 32768
    run_moves(specs, lambda w: 37 if w < 8191 else 3, seed=w)


def test_rows_twelve_moves(hip_lib):
    """Twelve moves of mixed widths, pads and ops in one launch: a one-row move directly behind a three-workgroup move and another
    directly in front of one."""
    specs = [(1, 1, 1, 0, E.COPY), (4, 5000, 3, 0, E.ZERO_NEW), (3, 1, 2, 1, E.CLAMP_MAX), (45, 100, 1, 3, E.COPY), (7, 9, 0, 2, E.ZERO_ALL),
             (5, 1, 3, 3, E.COPY), (8, 2500, 2, 1, E.CLAMP_MAX), (8193, 2, 1, 2, E.ZERO_NEW), (2, 1, 0, 0, E.ZERO_NEW), (48, 171, 3, 1, E.COPY),
             (1, 8190, 2, 3, E.CLAMP_MAX), (32768, 1, 1, 1, E.COPY)]
    tab, blocks = run_moves(specs, lambda w: 37 if w < 8191 else 3, seed=12)
    assert tab["first_block"].tolist() == [0, 1, 4, 5, 6, 7, 8, 11, 14, 15, 17, 19] and blocks == 24
