"""tests/blend_refs.py without a GPU: the float64 backward equals finite differences of the float64 forward, the two forms of its
output map into each other, the scenes show the edges they are named for on well-conditioned pixels, and the fp32 C oracle
(oracle/gsplat_oracle.c: an independent implementation in gsplat's evaluation order) lies within the constants stored in
blend_refs -- the numbers tests/test_gpu_blend_edges.py derives its bounds from.  Nothing here runs a HIP kernel."""
import numpy as np
import pytest

from tests import blend_refs as R


class _Params:
    """Float64 stand-ins of a scene's arrays."""

    def __init__(self, sc):
        self.means, self.conics, self.opac = (np.array(v, dtype=np.float64) for v in (sc.means, sc.conics, sc.opac))
        self.colors, self.depths = np.array(sc.colors, dtype=np.float64), np.array(sc.depths, dtype=np.float64)
        self.bg = np.array(sc.bg, dtype=np.float64)

    def channels(self):
        return np.concatenate([self.colors, self.depths[:, None]], axis=1)


def test_backward_is_the_gradient_of_the_forward():
    """Central differences of sum(render G) + sum(alpha Ga) in every input of a smooth 40-Gaussian tile (expected depth and a
    background included), against the dense rows of the backward: 1e-6 of each group's largest gradient."""
    sc = R.gradient_check_scene()
    p = _Params(sc)
    rng = np.random.RandomState(1)
    fwd, _, _ = R.forward(sc, p)
    f = fwd[0]
    assert not f["critical"].any() and not f["clamped"].any() and (1.0 - f["alpha"]).min() > 1e-2
    assert f["last"].min() >= 30                                                   # nothing terminates
    G, Ga = rng.standard_normal(f["render"].shape), rng.standard_normal(f["alpha"].shape)

    def loss():
        o = R.forward(sc, p)[0][0]
        return float((o["render"] * G).sum() + (o["alpha"] * Ga).sum())

    got = R.backward(sc, {0: dict(alpha=f["alpha"], last=f["last"], render=f["render"])}, {0: G}, {0: Ga}, params=p, rounded=False)["dense"]
    groups = [("means", p.means, (0, 1)), ("conics", p.conics, (4, 5, 6)), ("opacities", p.opac[:, None], (7,)),
              ("colors", p.colors, (8, 9, 10)), ("depths", p.depths[:, None], (11,))]
    for name, arr, cols in groups:
        fd = np.zeros((sc.n, len(cols)))
        for g in range(sc.n):
            for k in range(len(cols)):
                x = arr[g, k]
                h = 1e-5 * max(abs(x), 1e-2)
                arr[g, k] = x + h
                up = loss()
                arr[g, k] = x - h
                dn = loss()
                arr[g, k] = x
                fd[g, k] = (up - dn) / (2 * h)
        an = got[:, list(cols)]
        err = np.abs(fd - an).max() / np.abs(an).max()
        print(f"finite differences, {name}: {err:.2e} of the largest gradient")
        assert err <= 1e-6, name


@pytest.mark.parametrize("name", R.SCENES)
def test_packed_rows_map_to_dense_gradients(name):
    """v_x = -o (a sum h dx + b sum h dy), the conic gradient from the second moments, v_o = sum h: the raw-moment rows and the
    per-pixel sums of gsplat's form are two outputs of one walk and must not drift apart (float64 rounding of a cancelling sum:
    1e-10 of its sum of |terms|)."""
    sc, _, _, _, _, _, _, bw = R.reference(name)
    mapped = R.rows_to_dense(sc, bw["rows"])
    assert np.isfinite(mapped).all() and np.isfinite(bw["dense"]).all()
    assert (np.abs(mapped - bw["dense"]) <= 1e-10 * bw["dense_terms"]).all()
    assert (np.abs(bw["dense"]) <= bw["dense_terms"] * (1 + 1e-9)).all() and (np.abs(bw["rows"]) <= bw["rows_terms"] * (1 + 1e-9)).all()
    assert (bw["dense"][:, 2:4] >= np.abs(bw["dense"][:, 0:2]) * (1 - 1e-9)).all()


def test_scene_table_covers_what_it_promises():
    tiles = {k: tuple(R.scene(n).tiles for n in v) for k, v in R.THRESHOLD_GRIDS.items()}
    assert tiles == {1536: (1535, 1536), 3000: (2999, 3000), 6000: (5999, 6000), 16000: (15999, 16000)}
    scs = [R.scene(n) for n in R.SCENES]
    assert {s.DT for s in scs} == {1, 3, 4, 5, 7, 8, 16, 32}
    for flag in ("has_depth", "ed"):
        assert {getattr(s, flag) for s in scs} == {False, True}
    assert {s.bg is None for s in scs} == {False, True}
    assert max(s.C * s.W * s.H for s in scs) <= 4.2e6
    for kind in ("faint", "strong"):          # every list length on both batch sizes: below 1536 tiles and from 16000
        for lo, hi in ((0, 1536), (16000, 1 << 30)):
            lens = set()
            for n in R.SCENES:
                if n.startswith(kind) and lo <= R.scene(n).tiles < hi:
                    lens |= {v.size for v in R.scene(n).lists.values()}
            assert lens >= set(R.LENGTHS) - {0}, (kind, lo, sorted(lens))
    valid = set()
    for s in scs:
        valid |= {s.tile_box(t)[3:] for t in s.lists}
    assert {w for w, _ in valid} >= {1, 8, 16} and {h for _, h in valid} >= {1, 11, 16}
    assert valid & {(1, 11), (8, 11), (1, 1), (8, 1)}, "a corner tile cut on both sides"


@pytest.mark.parametrize("name", R.SCENES)
def test_critical_pixels_are_few_and_the_edges_show(name):
    """A condition on the INPUTS: at most 5 of a tile's 256 pixels lie within 1e-4 of a threshold, and what the scene is named
    for happens on pixels that are compared at rounding level."""
    sc, fwd, hit_any, hit_clear, _, _, _, bw = R.reference(name)
    start, _ = sc.starts()
    for t, f in fwd.items():
        assert int(f["critical"].sum()) <= R.MAX_CRITICAL_PER_TILE, (name, t, int(f["critical"].sum()))
    clear = {t: ~f["critical"] for t, f in fwd.items()}
    m = sc.marks
    if "clamp" in m:
        f = fwd[m["clamp"]]
        assert (f["clamped"] & clear[m["clamp"]]).sum() >= 2, "alpha binds at 0.999 on well-conditioned pixels"
    if "clamp_front" in m:
        f = fwd[m["clamp_front"]]
        assert (f["clamped"] & clear[m["clamp_front"]] & (f["last"] - start[m["clamp_front"]] >= 3)).any(), "something composited behind a bound alpha"
    if "second_batch" in m:
        t = m["second_batch"]
        rel = fwd[t]["last"] - start[t]
        assert ((rel >= 256) & (rel < 511) & clear[t]).sum() >= 16 and len(set(rel[clear[t]])) >= 8, "termination inside the second 256-batch"
    if "last_tile_len" in m:
        assert sc.lists[sc.tiles - 1].size == m["last_tile_len"]
    if sc.cap_pad:
        assert sc.gather_form()[1][-sc.cap_pad:].tolist() == [-1] * sc.cap_pad and (sc.tiles - 1) in sc.lists
    for t in sc.lists:                     # every list longer than two entries leaves something on well-conditioned pixels of its tile
        if sc.lists[t].size > 2:
            assert ((fwd[t]["alpha"] > 0) & clear[t]).any(), (name, t, sc.tile_box(t))
    assert not set(m.get("dead", [])) & hit_any and not set(m.get("culled", [])) & hit_any
    assert set(m.get("grazing", [])) <= hit_clear
    if "shared" in m:
        assert sum(g in hit_clear for g in m["shared"]) >= 10
    if name.startswith("strong"):          # pixels finish at different entries, and a good part of every long list is never reached
        assert len(hit_any) < 0.8 * sum(v.size for v in sc.lists.values())
    if name.startswith("faint"):           # nothing terminates: every entry of every list is composited somewhere
        assert len(hit_any) == sum(v.size for v in sc.lists.values())
    untouched = np.ones(sc.n, bool)
    untouched[sorted(hit_any)] = False
    assert not bw["rows"][untouched].any() and not bw["dense"][untouched].any()


def _full(sc, per_tile, key, fwd, width=None, dtype=np.float32):
    out = np.zeros((sc.C * sc.H * sc.W,) + (() if width is None else (width,)), dtype=dtype)
    for t, f in fwd.items():
        out[f["pix"]] = per_tile[t][key] if key is not None else per_tile[t]
    return out


def oracle_ratios(oracle, name):
    """The C oracle on one scene: worst |oracle - reference| / (2^-24 sum |terms|), forward and per backward group."""
    sc, fwd, _, _, fin, vr, va, bw = R.reference(name)
    start, ids = sc.starts()
    offsets, _ = sc.gather_form()
    N = sc.n // sc.C
    chan = sc.channels().reshape(sc.C, N, sc.DT)
    bg = None
    if sc.bg is not None:
        bg = np.zeros((sc.C, sc.DT), np.float32)
        bg[:, :sc.D] = sc.bg
    opac = np.where(np.isnan(sc.opac), np.float32(0), sc.opac).reshape(sc.C, N)
    args = (sc.means.reshape(sc.C, N, 2), sc.conics.reshape(sc.C, N, 3), chan, opac, bg, sc.W, sc.H, R.TS, offsets, ids)
    render, alphas, last = oracle.blend_fwd(*args)
    render, alphas, last = render.reshape(-1, sc.DT), alphas.reshape(-1), last.reshape(-1)
    worst = 0.0
    for t, f in fwd.items():
        ok = ~f["critical"]
        pix = f["pix"][ok]
        assert np.array_equal(last[pix], f["last"][ok]), (name, t)
        worst = max(worst, R.worst_ratio(render[pix], f["render"][ok], f["render_terms"][ok]),
                    R.worst_ratio(alphas[pix], f["alpha"][ok], f["alpha_terms"][ok]))
    v_render = _full(sc, vr, None, fwd, sc.DT).reshape(sc.C, sc.H, sc.W, sc.DT)
    v_alphas = _full(sc, va, None, fwd).reshape(sc.C, sc.H, sc.W, 1)
    a_in = _full(sc, fin, "alpha", fwd).reshape(sc.C, sc.H, sc.W, 1)
    l_in = _full(sc, fin, "last", fwd, dtype=np.int32).reshape(sc.C, sc.H, sc.W)
    v2d, vabs, vcon, vcol, vop = oracle.blend_bwd(*args, a_in, l_in, v_render, v_alphas, absgrad=True)
    got = np.concatenate([v2d.reshape(-1, 2), vabs.reshape(-1, 2), vcon.reshape(-1, 3), vop.reshape(-1, 1), vcol.reshape(-1, sc.DT)], axis=1)
    back = {}
    for grp, (lo, hi) in dict(R.ROW_GROUPS, channels=(8, 8 + sc.DT)).items():
        back[grp] = R.worst_ratio(got[:, lo:hi], bw["dense"][:, lo:hi], bw["dense_terms"][:, lo:hi])
    return worst, back


def test_oracle_within_constants(oracle):
    """Measures the constants of blend_refs (ORACLE_FWD, ORACLE_BWD) and asserts that the oracle still lies within them: the GPU
    test allows a HIP kernel four times max(constant, 1)."""
    fwd_worst, back_worst = 0.0, {k: 0.0 for k in R.ORACLE_BWD}
    for name in R.SCENES:
        if R.scene(name).ed:
            continue                       # (the oracle has no expected-depth normalisation)
        w, back = oracle_ratios(oracle, name)
        print(f"{name}: forward {w:.2f}  backward " + "  ".join(f"{k} {v:.2f}" for k, v in back.items()))
        fwd_worst = max(fwd_worst, w)
        back_worst = {k: max(v, back[k]) for k, v in back_worst.items()}
    print(f"measured: ORACLE_FWD = {fwd_worst:.2f}  ORACLE_BWD = " + ", ".join(f'"{k}": {v:.2f}' for k, v in back_worst.items()))
    assert fwd_worst <= R.ORACLE_FWD
    for k, v in back_worst.items():
        assert v <= R.ORACLE_BWD[k], (k, v)
