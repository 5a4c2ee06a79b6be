"""tests/refine_edge_refs.py without a GPU: its references agree with tests/refine_scene_refs.py and oracle/refine_oracle.py where they
overlap, the two constants of the sample positions are MEASURED here (float32 restatement against float64, never a HIP kernel), the
inputs of the equality tests sit exactly on their thresholds, the two recorded Philox keys give a uniform of exactly 1.0, and the
width that stresses the row mover's multiply-high division hardest is computed and checked."""
import numpy as np
import pytest

from oracle import refine_oracle as ro
from tests import refine_edge_refs as E
from tests import refine_scene_refs as R

F = np.float32


# ---- the references agree where they overlap ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
def test_flags_and_moves_reproduce_the_restatement(kind):
    """One seeded node per kind: the output order rebuilt from flags_ref (old rows, children sample-major, duplicates) is the
    restatement's src_index / kind, and move_ref with them reproduces every tensor it returns: parameters (COPY), moments (ZERO_NEW),
    the opacity reset (CLAMP_MAX on the parameter, ZERO_ALL on its moments)."""
    from mtgs_amd.densify import RefineConfig
    step, seed, N = R.RESET_STEP, 99 + (5 << 34), 3000
    cfg = RefineConfig(stop_split_at=20000, densify_from_iter=0, n_split_samples=3)
    p, stats, moments, _ = R.raw_node(N, 17, kind)
    new, new_m, masks = R.refinement_after(p, stats, cfg, step, seed, moments=moments)
    assert masks["reset"] and masks["splits"].sum() > 30 and masks["dups"].sum() > 30
    th = (cfg.densify_grad_thresh, cfg.densify_size_thresh, cfg.split_screen_size, cfg.cull_alpha_thresh, cfg.cull_scale_thresh, cfg.cull_screen_size)
    opt = (3, 1, 1, 1, 1)                                         # step 3100: > 3000 and < stop_screen_size_at
    flags, parents, counts, _ = E.flags_ref(p, stats, th, opt, step, seed, n_columns=5)
    src = np.concatenate([np.flatnonzero((flags >> k) & 1) for k in range(5)])
    knd = np.concatenate([np.full(int(((flags >> k) & 1).sum()), k) for k in range(5)])
    assert np.array_equal(src, masks["src_index"]) and np.array_equal(knd, masks["kind"])
    assert np.array_equal(flags >> 7, masks["splits"].astype(np.uint8)) and np.array_equal(counts[5], flags >> 7)
    assert np.array_equal(counts[:5].sum(0), [bin(v & 0x7F).count("1") for v in flags])
    want_parents = np.zeros(N, bool)
    want_parents[src[knd > 0]] = True
    assert np.array_equal(parents.astype(bool), want_parents)
    cap = float(F(np.log(0.01 / 0.99)))
    words = lambda a: np.ascontiguousarray(a, dtype=F).reshape(a.shape[0], -1).view(np.uint32)
    for k, v in p.items():
        if k in ("means", "scales"):
            continue
        reset = k == "opacities"
        got = E.move_ref(words(v), src, knd, E.CLAMP_MAX if reset else E.COPY, cap).view(F)
        want = np.minimum(new[k], cap) if reset else new[k]
        assert np.array_equal(got, want.reshape(got.shape).astype(F)), k
        for h in (0, 1):
            got = E.move_ref(words(moments[k][h]), src, knd, E.ZERO_ALL if reset else E.ZERO_NEW).view(F)
            assert np.array_equal(got, new_m[k][h].reshape(got.shape).astype(F)), (k, h)


def test_move_ref_zero_rows_and_clamp():
    src = np.arange(12, dtype=np.uint32).reshape(4, 3) + 1
    idx = np.array([3, -1, 4, 2 ** 31 - 1, -2 ** 31, 0])
    out = E.move_ref(src, idx, np.zeros(6), E.COPY)
    assert np.array_equal(out[[0, 5]], src[[3, 0]]) and not out[1:5].any()
    x = np.array([[np.nan, np.inf, -np.inf, -0.0, 2.5, 2.4999998, 3.0]], dtype=F)
    got = E.move_ref(x.view(np.uint32), [0], [0], E.CLAMP_MAX, 2.5).view(F)[0]
    assert np.isnan(got[0]) and np.array_equal(got[1:], np.array([2.5, -np.inf, -0.0, 2.5, 2.4999998, 2.5], dtype=F))
    assert np.signbit(got[3])


def test_sample_ref64_equals_the_oracle_away_from_a_uniform_of_one():
    """normals3 (float64 uniforms) + quat_to_rotmat against sample_ref64 (float32 uniforms) on the Gaussian indices, slots and steps of
    the GPU precision test, unit scales: within 1e-6 wherever every uniform is below 1 - 2^-20 -- the two differ only through the
    rounding of the uniforms."""
    g = np.random.default_rng(1)
    idx = np.arange(E.PRECISION_N)
    q = g.standard_normal((idx.size, 4)) * 10.0 ** g.uniform(-3, 3, (idx.size, 1))
    rot = ro.quat_to_rotmat(q / np.linalg.norm(q, axis=-1, keepdims=True))
    m = g.standard_normal((idx.size, 3))
    seen = 0
    for step in E.PRECISION_STEPS:
        for slot in range(E.PRECISION_S + 1):
            u = E.uniforms_f32(E.PRECISION_SEED, step, idx, slot)
            got = E.sample_ref64(m, np.zeros((idx.size, 3)), q, u)[0]
            want = m + np.einsum("nij,nj->ni", rot, ro.normals3(E.PRECISION_SEED, step, idx, slot))
            ok = (u < 1 - 2.0 ** -20).all(1)
            seen += int(ok.sum())
            assert np.abs(got - want)[ok].max() <= 1e-6, (step, slot, np.abs(got - want)[ok].max())
    assert seen >= 6 * E.PRECISION_N - 2


def test_sample_f32_is_float32_throughout():
    p, _, _, _ = E.precision_node("child")
    u = E.uniforms_f32(5, 6, np.arange(E.PRECISION_N), 0)
    assert u.dtype == F
    out, small = E.sample_f32(p["means"], p["scales"], p["quats"], u)
    assert out.dtype == F and small.dtype == F and np.isfinite(out).all() and np.isfinite(small).all()


# ---- the constants --------------------------------------------------------------------------------------------------------------------
def test_constants():
    """SAMPLE_MEANS / SAMPLE_SCALES: the float32 restatement's distance from sample_ref64 in units of 2^-24 x terms, over the inputs
    of the GPU precision test.  The recorded values hold, and are not more than a rounding above what is measured."""
    got = E.measure_constants()
    rec = {"means": E.SAMPLE_MEANS, "scales": E.SAMPLE_SCALES}
    msg = f"recorded {rec}, measured {got}"
    for k in rec:
        assert got[k] <= rec[k], msg
        assert got[k] > rec[k] - 0.02, msg               # recorded = measured, rounded up in the second decimal
    # every kind of row took part
    kinds = set()
    for which, clone, step in E.precision_cases():
        masks = E.precision_reference(which, clone, step)[4]
        kinds |= set(np.unique(masks["kind"]).tolist())
        assert masks["keep"].sum() >= E.PRECISION_N
    assert kinds == {0, 1, 2, 3}


def test_precision_nodes_are_what_they_say():
    for which, want in (("old", {0}), ("child", {1, 2}), ("dup", {0, 1, 2, 3})):
        p, stats, th, opt, masks, geo = E.precision_reference(which, 1, E.UNIT_RA_STEP)
        assert set(np.unique(masks["kind"]).tolist()) == want
        q = np.linalg.norm(p["quats"].astype(np.float64), axis=-1)
        assert q.min() < 3e-3 and q.max() > 3e2 and np.exp(p["scales"]).min() < 0.02 and np.exp(p["scales"]).max() > 600
        for name, v, t, _ in masks["decisions"]:
            with np.errstate(all="ignore"):
                assert np.min(np.abs(v - t) / abs(t)) > 0.1, (which, name)
    # the duplicate of a split parent takes the shrunk scales: both kinds of duplicate are there
    masks, (_, _, _, _, sampled, shrunk) = E.precision_reference("dup", 1, E.UNIT_RA_STEP)[4:]
    dup = masks["kind"] == 3
    assert (shrunk & dup).sum() > 100 and (~shrunk & dup).sum() > 100 and sampled[dup].all()
    assert not E.precision_reference("dup", 0, E.UNIT_RA_STEP)[5][4][dup].any()


# ---- exact boundary inputs ------------------------------------------------------------------------------------------------------------
def test_the_boundary_values_are_exact():
    assert np.exp(0.0) == 1.0 and np.exp(F(0.0)) == F(1.0)
    assert 1.0 / (1.0 + np.exp(-0.0)) == 0.5
    assert np.linalg.norm(np.array([100.0, 0.0, 0.0])) == 100.0
    assert 0.75 / 3 == 0.25 and F(0.75) / F(3) == F(0.25)
    assert 2 * 0.5 == 1 and F(2) * F(0.5) == F(1)
    assert np.nextafter(F(0.5), F(1)) * F(2) == np.nextafter(F(1), F(2)) and np.nextafter(F(0.5), F(0)) * F(2) == np.nextafter(F(1), F(0))


@pytest.mark.parametrize("rule", list(E.EQ_RULES))
def test_equality_nodes_sit_on_their_threshold(rule):
    """At the threshold the compared float64 value EQUALS it for all eight rows, every other decision is at least MARGIN away, and
    the flags written out by hand are flags_ref's; one ulp to one side changes the flags, one ulp to the other does not."""
    at, _, by_hand, _ = E.EQ_RULES[rule]
    p, stats, _, opt, _ = E.equality_node(rule)
    flags = {}
    for tag, th, far in E.equality_variants(rule):
        f, parents, counts, masks = E.flags_ref(p, stats, th, opt, E.EQ_STEP, E.EQ_SEED, far)
        flags[tag] = f
        seen = set()
        for name, v, t, src in masks["decisions"]:
            d = np.abs(v - t)
            if name in at and tag == "equal":
                assert (d == 0).all(), (rule, name)
                seen.add(name)
            elif name not in at:
                assert (d > R.MARGIN * abs(t)).all(), (rule, tag, name)
        assert tag != "equal" or seen == set(at)
    assert (flags["equal"] == by_hand).all(), (rule, flags["equal"])
    changed = [tag for tag in ("below", "above") if not np.array_equal(flags[tag], flags["equal"])]
    assert len(changed) == 1, (rule, changed)


def test_zero_visibility_flags():
    p, stats, th, opt, by_hand = E.zero_visibility_node()
    assert np.array_equal(E.flags_ref(p, stats, th, opt, E.EQ_STEP, E.EQ_SEED)[0], by_hand)


def test_no_sampled_decision_of_the_option_and_table_nodes_is_near_its_threshold():
    """The children's cull at their drawn position (and every other decision) is at least MARGIN from its threshold, so the float32
    kernel and the float64 restatement must agree on every flag."""
    p, stats = E.option_node()
    seen = set()
    for opt in E.OPTION_SETS:
        r = E.refinement(p, stats, E.OPTION_THRESHOLDS, opt, E.OPTION_STEP, E.OPTION_SEED)
        assert min(R.margins(r).values()) >= R.MARGIN, opt
        seen.add(E.flags_ref(p, stats, E.OPTION_THRESHOLDS, opt, E.OPTION_STEP, E.OPTION_SEED)[0].tobytes())
    # of the ten sets, option 3 without option 2 (twice), option 4 without option 2 and option 3 beside option 1 (whatever is wider than
    # cull_screen_size was split by split_screen_size) change no flag
    assert len(seen) == 6, len(seen)
    for (p, stats, th, opt, seed), n in zip(E.table_nodes(), E.TABLE_N):
        assert p["means"].shape[0] == n
        if n:
            assert min(R.margins(E.refinement(p, stats, th, opt, E.TABLE_STEP, seed)).values()) >= R.MARGIN


# ---- a uniform of exactly 1 -----------------------------------------------------------------------------------------------------------
def test_the_recorded_keys_give_a_uniform_of_exactly_one():
    """Word 0 of (1234567, 6276890, 0, 0) and word 2 of (1234567, 2569880, 0, 0) round to 2^32 in float32: u = 1.0, radius 0.  With
    float64 uniforms the radius is sqrt(-2 log(1 - d / 2^32)): 2.14e-4 for the second key (d = 98.5) -- more than 1e-4, and more than
    the whole tolerance the float64-uniform reference used to need -- and 7.63e-5 for the first (d = 12.5): that one stays BELOW 1e-4,
    whatever the angle, so for it the measured radius is asserted instead."""
    w = E.philox_words(E.PRECISION_SEED, E.UNIT_RA_STEP, [0], 0)[0]
    assert int(w[0]) == 4294967283
    u = E.uniforms_f32(E.PRECISION_SEED, E.UNIT_RA_STEP, [0], 0)[0]
    assert u[0] == F(1.0) and (u[1:] < 1 - 2.0 ** -20).all()
    w = E.philox_words(E.PRECISION_SEED, E.UNIT_RB_STEP, [0], 0)[0]
    assert int(w[2]) == 4294967197
    v = E.uniforms_f32(E.PRECISION_SEED, E.UNIT_RB_STEP, [0], 0)[0]
    assert v[2] == F(1.0) and (v[[0, 1, 3]] < 1 - 2.0 ** -20).all()
    ident, zero = np.array([[1.0, 0, 0, 0]]), np.zeros((1, 3))
    a = E.sample_ref64(zero, zero, ident, u[None])[0][0]
    b = E.sample_ref64(zero, zero, ident, v[None])[0][0]
    assert a[0] == 0 and a[1] == 0 and abs(a[2]) > 0.1                     # the third axis only
    assert b[2] == 0 and abs(b[0]) + abs(b[1]) > 0.1                       # the first two only
    da = np.abs(ro.normals3(E.PRECISION_SEED, E.UNIT_RA_STEP, [0], 0)[0] - a).max()
    db = np.abs(ro.normals3(E.PRECISION_SEED, E.UNIT_RB_STEP, [0], 0)[0] - b).max()
    assert db > 1e-4, db
    assert 5e-5 < da <= np.sqrt(-2 * np.log1p(-12.5 / 2 ** 32)) < 1e-4, da


# ---- the widths of the row mover ------------------------------------------------------------------------------------------------------
def test_the_worst_width_divides_exactly():
    """q * magic >> 32 == q // w at every q = k w - 1 and k w below 8192 + w (the kernel's q = column of the workgroup's first dword
    + at most 8191), for the width that maximises (8191 + w)(magic w - 2^32) -- and for every other width of the GPU test."""
    worst = E.worst_width()
    w = np.arange(2, 32769, dtype=np.int64)
    score = (8191 + w) * ((0xFFFFFFFF // w + 1) * w - (1 << 32))
    assert score[worst - 2] == score.max() and worst in E.MOVE_WIDTHS and score.max() < 1 << 32
    for w in E.MOVE_WIDTHS[1:]:
        magic = 0xFFFFFFFF // w + 1
        k = np.arange(1, (8192 + w) // w + 1, dtype=np.uint64)
        for q in (k * np.uint64(w) - np.uint64(1), k * np.uint64(w)):
            q = q[q < 8192 + w]
            assert np.array_equal((q * np.uint64(magic)) >> np.uint64(32), q // np.uint64(w)), w


def test_table_builders_match_the_header_arithmetic():
    tab, blocks = E.move_table([dict(n_rows=r, out_start=0, n_src=1, src=0, dst=0, width=w, op=0, clamp_max=0.0)
                                for r, w in ((1, 1), (8189, 1), (8190, 1), (2, 8192), (1, 5))])
    assert tab["first_block"].tolist() == [0, 1, 2, 4, 7] and blocks == 8
    nodes = [dict(n=n, means=0, scales=0, quats=0, opacities=0, xys_grad_norm=0, vis_counts=0, max_2dsize=0, seed=1, thresholds=(0,) * 6,
                  options=(1, 0, 0, 0, 0), far_radius=1.0, far_factor=1.0, phase=E.DENSIFY) for n in (0, 3, 257, 0, 2)]
    tab = E.node_table(nodes)
    assert tab["start"].tolist() == [0, 0, 3, 260, 260] and tab["first_block"].tolist() == [0, 0, 1, 3, 3]
    counts = np.zeros((4, 262), dtype=np.int32)
    counts[0, [0, 2, 5, 260]] = 1
    counts[1, [1, 261]] = 1
    counts[2, [4]] = 1
    incl, tab = E.fill_after_scan(tab, counts, 3)
    assert tab["n_out"].tolist() == [0, 3, 2, 0, 2] and tab["out_start"].tolist() == [0, 0, 3, 5, 5]
    assert tab["out_first_block"].tolist() == [0, 0, 1, 2, 2]
    assert tab["scan_base"][:, :3].tolist() == [[0, 0, 0], [0, 0, 0], [2, 1, 0], [3, 1, 1], [3, 1, 1]]
    assert tab["col_base"][:, :3].tolist() == [[0, 0, 0], [0, 2, 3], [0, 1, 1], [0, 0, 0], [0, 1, 2]]
    assert incl.dtype == np.int64 and incl[0, -1] == 4
