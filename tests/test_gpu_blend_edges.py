"""The compositing kernels (csrc/blend.hip) called directly through the C ABI on the scenes of tests/blend_refs.py, against its
float64 reference: list lengths around both batch sizes, the cull, the 0.999 clamp, degenerate candidates, edge tiles, sentinels,
and a tile grid on each side of every pick_ppl threshold so that every instantiation runs -- the expectations do not depend on
which one does.

Bounds: `blend_refs.device_bound(constant)` x 2^-24 x the sum of |terms| of the very number compared, the constants being the C
oracle's own distance from the reference (measured by tests/test_blend_refs_host.py, never against these kernels).  The backward
is given the REFERENCE's float32 alphas / last_ids / render and a cotangent that is zero on the threshold-critical pixels, so it
is a well-defined function of its inputs and no flipped-decision budget exists in this file.

The canary rule of tests/test_gpu_bin_edges.py holds for every call: outputs have slack behind them and are pre-filled with one
bit pattern (accumulated gradient columns with zeros, as the ABI asks); what was written is asserted AND that everything else
still holds the pattern."""
import numpy as np
import pytest
import torch

from tests import blend_refs as R
from tests.test_gpu_bin_edges import CAN, SL, _call, _st, can, host, up

pytestmark = pytest.mark.gpu

FCAN = float(np.array([CAN], dtype=np.int32).view(np.float32)[0])
BOUND_FWD = R.device_bound(R.ORACLE_FWD)
BOUND_BWD = {k: R.device_bound(v) for k, v in R.ORACLE_BWD.items()}
PACKED = [n for n in R.SCENES if R.scene(n).DT <= 8]
FLIP = 1.5 / 255.0 + 1e-4                                 # tests/util.py::assert_image_close: one flipped decision


def fcan(n):
    return can(n).view(torch.float32)


def zeros_then_canary(n):
    t = fcan(n + SL)
    t[:n] = 0
    return t


def is_canary(t):
    return bool((t.contiguous().view(torch.int32) == CAN).all())


_dev = {}


def device_scene(name):
    """The scene's inputs on the device, in both forms, once per scene."""
    if name not in _dev:
        sc = R.scene(name)
        offsets, flat = sc.gather_form()
        d = dict(means=up(sc.means), conics=up(sc.conics), colors=up(sc.colors), opac=up(sc.opac),
                 depths=None if sc.depths is None else up(sc.depths), bg=None if sc.bg is None else up(sc.bg),
                 # (one zero behind the T offsets of the gather form: the last tile ends at M, the element behind is never the end)
                 offsets=up(np.concatenate([offsets.reshape(-1), np.zeros(1, np.int32)])), flat=up(flat), M=int(flat.size))
        if sc.DT <= 8:
            rec, poff, pids = sc.packed_form()
            d.update(rec=up(rec), poff=up(poff), pids=up(pids))
        _dev[name] = d
    return _dev[name]


def ptr(t):
    return None if t is None else t.data_ptr()


def schedule(sc, d, packed):
    order = can(sc.tiles + SL)
    if packed:
        _call("mtgs_tile_schedule", sc.C, sc.tw, sc.th, ptr(d["poff"]), int(host(d["poff"][-1:])[0]), ptr(order), _st())
    else:
        _call("mtgs_tile_schedule", sc.C, sc.tw, sc.th, ptr(d["offsets"]), d["M"], ptr(order), _st())
    assert torch.equal(order[:sc.tiles].sort().values, torch.arange(sc.tiles, dtype=torch.int32, device="cuda")) and is_canary(order[sc.tiles:])
    return order


def run_forward(sc, d, packed, order, also_zero=None, also_zero_bytes=0):
    P = sc.C * sc.H * sc.W
    render, alphas, last = fcan(P * sc.DT + SL), fcan(P + SL), can(P + SL)
    if packed:
        _call("mtgs_blend_fwd_packed", sc.C, sc.D, int(sc.has_depth), ptr(d["rec"]), ptr(d["bg"]), int(sc.ed), sc.W, sc.H, sc.tw, sc.th,
              ptr(d["poff"]), ptr(d["pids"]), ptr(render), ptr(alphas), ptr(last), ptr(order), also_zero, also_zero_bytes, _st())
    else:
        _call("mtgs_blend_fwd", sc.C, sc.n // sc.C, sc.D, ptr(d["means"]), ptr(d["conics"]), ptr(d["colors"]), ptr(d["opac"]), ptr(d["bg"]),
              ptr(d["depths"]), int(sc.ed), sc.W, sc.H, R.TS, sc.tw, sc.th, ptr(d["offsets"]), ptr(d["flat"]), d["M"], ptr(render),
              ptr(alphas), ptr(last), ptr(order), _st())
    return render, alphas, last


def within(got, ref, terms, bound):
    """The worst |got - ref| / (bound 2^-24 terms): at most 1 to pass; inf where a number without any term is not exactly its reference."""
    return R.worst_ratio(got, ref, terms) / bound


@pytest.mark.parametrize("name,form", [(n, "gather") for n in R.SCENES] + [(n, "packed") for n in PACKED])
def test_forward(hip_lib, name, form):
    packed = form == "packed"
    sc, fwd, _, _, _, _, _, _ = R.reference(name)
    d = device_scene(name)
    P = sc.C * sc.H * sc.W
    order = schedule(sc, d, packed)
    sched = order[:sc.tiles].contiguous()
    render, alphas, last = run_forward(sc, d, packed, None)
    # nothing behind C H W
    assert is_canary(render[P * sc.DT:]) and is_canary(alphas[P:]) and is_canary(last[P:])
    # the same call twice, and every dispatch order, bit for bit
    for o in (None, sched, sched.flip(0).contiguous()):
        r2, a2, l2 = run_forward(sc, d, packed, o)
        assert torch.equal(r2.view(torch.int32), render.view(torch.int32)) and torch.equal(a2.view(torch.int32), alphas.view(torch.int32))
        assert torch.equal(l2, last)
    # every pixel of an empty tile: exactly the background on the colour channels, zero otherwise
    pop = up(np.concatenate([f["pix"] for f in fwd.values()]))
    r = render[:P * sc.DT].view(sc.C, sc.H * sc.W, sc.DT)
    wrong = (r != up(sc.empty_render())[:, None, :]).any(dim=-1).view(-1) | (alphas[:P] != 0) | (last[:P] != 0)
    wrong[pop] = False
    assert not bool(wrong.any()), f"{int(wrong.sum())} pixels of empty tiles are not background"
    # populated tiles
    r_h, a_h, l_h = host(r.view(P, sc.DT)[pop]), host(alphas[:P][pop]), host(last[:P][pop])
    span = np.maximum(1.0, np.abs(sc.channels()).max(axis=0))
    at = 0
    for t, f in fwd.items():
        n = f["pix"].size
        gr, ga, gl = r_h[at:at + n], a_h[at:at + n], l_h[at:at + n]
        at += n
        where = f"{name} {form} tile {t} {sc.tile_box(t)} list of {sc.lists[t].size}"
        ok = ~f["critical"]
        assert np.isfinite(gr).all() and np.isfinite(ga).all(), where
        assert np.array_equal(gl[ok], f["last"][ok]), where + ": last_ids"
        wr = within(gr[ok], f["render"][ok], f["render_terms"][ok], BOUND_FWD)
        wa = within(ga[ok], f["alpha"][ok], f["alpha_terms"][ok], BOUND_FWD)
        print(f"{where}: render {wr:.3f} alpha {wa:.3f} of the bound")
        assert wr <= 1.0 and wa <= 1.0, where + f": render {wr:.2f} alpha {wa:.2f} x the bound"
        # critical pixels: one flipped decision at the most (expected depth is a weighted mean: anywhere in the depth range)
        lim = FLIP * span
        if sc.ed:
            lim[-1] = span[-1]
        assert (np.abs(gr[~ok] - f["render"][~ok]) <= lim).all() and (np.abs(ga[~ok] - f["alpha"][~ok]) <= FLIP).all(), where


@pytest.mark.parametrize("name", PACKED)
def test_touch(hip_lib, name):
    sc, fwd, hit_any, hit_clear, _, _, _, _ = R.reference(name)
    d = device_scene(name)
    touched = torch.full((sc.n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    for order in (None, schedule(sc, d, True)):
        _call("mtgs_blend_touch_packed", sc.C, ptr(d["rec"]), sc.W, sc.H, sc.tw, sc.th, ptr(d["poff"]), ptr(d["pids"]), ptr(order),
              ptr(touched), sc.n, _st())
        t = host(touched)
        assert (t[sc.n:] == 0xA5).all() and set(np.unique(t[:sc.n])) <= {0, 1}
        must, never = np.zeros(sc.n, bool), np.ones(sc.n, bool)
        must[sorted(hit_clear)] = True
        never[sorted(hit_any)] = False
        assert (t[:sc.n][must] == 1).all(), f"{name}: composited Gaussians not touched: {np.flatnonzero(must & (t[:sc.n] == 0))[:8]}"
        assert (t[:sc.n][never] == 0).all(), f"{name}: touched without a pixel: {np.flatnonzero(never & (t[:sc.n] == 1))[:8]}"
        touched.fill_(0xA5)


# ---- backward -----------------------------------------------------------------------------------------------------------------------
_bwd_in = {}


def backward_inputs(name):
    """The reference's float32 forward result and the cotangents as full images on the device."""
    if name not in _bwd_in:
        sc, fwd, _, _, fin, vr, va, _ = R.reference(name)
        P = sc.C * sc.H * sc.W
        pop = up(np.concatenate([f["pix"] for f in fwd.values()]))
        alphas, last = torch.zeros(P, device="cuda"), torch.zeros(P, dtype=torch.int32, device="cuda")
        render = up(sc.empty_render())[:, None, :].expand(sc.C, sc.H * sc.W, sc.DT).reshape(P, sc.DT).contiguous()
        v_render, v_alphas = torch.zeros(P, sc.DT, device="cuda"), torch.zeros(P, device="cuda")
        alphas[pop] = up(np.concatenate([fin[t]["alpha"] for t in fwd]))
        last[pop] = up(np.concatenate([fin[t]["last"] for t in fwd]))
        render[pop] = up(np.concatenate([fin[t]["render"] for t in fwd]))
        v_render[pop] = up(np.concatenate([vr[t] for t in fwd]))
        v_alphas[pop] = up(np.concatenate([va[t] for t in fwd]))
        _bwd_in[name] = (alphas, last, render, v_render, v_alphas)
    return _bwd_in[name]


def check_rows(where, sc, got, ref, terms, hit_any, cols=None):
    """Every component within its group's bound; rows of Gaussians that update no pixel exactly +0.0 in every column."""
    assert np.isfinite(got).all(), where + ": NaN or inf in a gradient row"
    worst = {}
    for grp, (lo, hi) in dict(R.ROW_GROUPS, channels=(8, 8 + sc.DT)).items():
        if cols is not None and grp not in cols:
            continue
        w = within(got[:, lo:hi], ref[:, lo:hi], terms[:, lo:hi], BOUND_BWD[grp])
        worst[grp] = w
        if w > 1.0:
            err = np.abs(got[:, lo:hi] - ref[:, lo:hi]) - BOUND_BWD[grp] * R.EPS * terms[:, lo:hi]
            g = int(np.argmax(err.max(axis=1)))
            tiles = [(t, sc.tile_box(t), int(np.flatnonzero(v == g)[0]), v.size) for t, v in sc.lists.items() if g in v]
            raise AssertionError(f"{where}: {grp} {w:.2f} x the bound at Gaussian {g} (tile, box, position, list length: {tiles}): "
                                 f"got {got[g, lo:hi]} want {ref[g, lo:hi]}")
    print(f"{where}: " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()) + " of the bound")
    dead = np.ones(sc.n, bool)
    dead[sorted(hit_any)] = False
    used = [c for grp, (lo, hi) in dict(R.ROW_GROUPS, channels=(8, 8 + sc.DT)).items() if cols is None or grp in cols for c in range(lo, hi)]
    bits = np.ascontiguousarray(got[dead][:, used]).view(np.int32)
    assert not bits.any(), where + f": rows that must be exactly 0.0: Gaussians {np.flatnonzero(dead)[np.flatnonzero(bits.any(axis=1))][:8]}"


@pytest.mark.parametrize("name", R.SCENES)
def test_backward_gather(hip_lib, name):
    """Dense gsplat arrays with absgrad; then the interleaved row layout with pad columns, v_means2d_abs null and grad_row_index
    a permutation onto compact rows."""
    from mtgs_amd import _lib
    sc, fwd, hit_any, _, _, _, _, bw = R.reference(name)
    d = device_scene(name)
    alphas, last, render, v_render, v_alphas = backward_inputs(name)
    n, DT = sc.n, sc.DT
    head = (sc.C, n // sc.C, sc.D, ptr(d["means"]), ptr(d["conics"]), ptr(d["colors"]), ptr(d["opac"]), ptr(d["bg"]), ptr(d["depths"]),
            int(sc.ed), sc.W, sc.H, R.TS, sc.tw, sc.th, ptr(d["offsets"]), ptr(d["flat"]), d["M"], ptr(alphas), ptr(last), ptr(render),
            ptr(v_render), ptr(v_alphas))
    # dense
    order = schedule(sc, d, False)
    o = {k: zeros_then_canary(n * w) for k, w in (("xy", 2), ("abs", 2), ("conic", 3), ("col", sc.D), ("dep", 1), ("op", 1))}
    _call("mtgs_blend_bwd", *head, ptr(o["xy"]), ptr(o["abs"]), ptr(o["conic"]), ptr(o["col"]), ptr(o["dep"]) if sc.has_depth else None,
          ptr(o["op"]), None, None, ptr(order), _st())
    for k, w in (("xy", 2), ("abs", 2), ("conic", 3), ("col", sc.D), ("dep", 1), ("op", 1)):
        assert is_canary(o[k][n * w:]), f"{name}: written behind {k}"
    parts = [host(o["xy"][:2 * n]).reshape(n, 2), host(o["abs"][:2 * n]).reshape(n, 2), host(o["conic"][:3 * n]).reshape(n, 3),
             host(o["op"][:n]).reshape(n, 1), host(o["col"][:sc.D * n]).reshape(n, sc.D)]
    if sc.has_depth:
        parts.append(host(o["dep"][:n]).reshape(n, 1))
    else:
        assert not host(o["dep"][:n]).any()
    got = np.concatenate(parts, axis=1)
    check_rows(f"{name} gather dense", sc, got, bw["dense"], bw["dense_terms"], hit_any)
    tol = R.EPS * (BOUND_BWD["xy"] * bw["dense_terms"][:, 0:2] + BOUND_BWD["xy_abs"] * bw["dense_terms"][:, 2:4])
    assert (got[:, 2:4] >= np.abs(got[:, 0:2]) - tol).all(), f"{name}: absgrad below |grad|"
    # interleaved rows [xy 2 | |xy| 2 | conic 3 | opacity | channels | pad 4], compact rows by a permutation, no absgrad, no order
    S = -(-(8 + DT) // 4) * 4 + 4
    perm = np.random.RandomState(3).permutation(n).astype(np.int32)
    G = fcan(n * S + SL)
    rows = G[:n * S].view(n, S)
    rows[:, 0:2] = 0
    rows[:, 4:8 + DT] = 0
    base = G.data_ptr()
    _call("mtgs_blend_bwd", *head, base, None, base + 16, base + 32, (base + 4 * (8 + sc.D)) if sc.has_depth else None, base + 28,
          _lib.host_i64([S] * 6), ptr(up(perm)), None, _st())
    h = host(rows)
    assert is_canary(G[n * S:]) and is_canary(rows[:, 2:4]) and is_canary(rows[:, 8 + DT:]), f"{name}: pad or absgrad columns written"
    got2 = h[perm][:, :8 + DT]
    check_rows(f"{name} gather interleaved", sc, got2, bw["dense"], bw["dense_terms"], hit_any, cols=("xy", "conic", "opacity", "channels"))


@pytest.mark.parametrize("name", PACKED)
def test_backward_packed(hip_lib, name):
    """Raw-moment rows: row_stride 16 with absgrad, 24 without (the |xy| columns and the pad keep the canary)."""
    sc, fwd, hit_any, _, _, _, _, bw = R.reference(name)
    d = device_scene(name)
    alphas, last, render, v_render, v_alphas = backward_inputs(name)
    n, DT = sc.n, sc.DT
    order = schedule(sc, d, True)
    for S, absgrad, o in ((16, 1, order), (24, 0, None)):
        G = fcan(n * S + SL)
        rows = G[:n * S].view(n, S)
        rows[:, :8 + DT] = 0
        if not absgrad:
            rows[:, 2:4] = FCAN
        _call("mtgs_blend_bwd_packed", sc.C, sc.D, int(sc.has_depth), ptr(d["rec"]), ptr(d["bg"]), int(sc.ed), sc.W, sc.H, sc.tw, sc.th,
              ptr(d["poff"]), ptr(d["pids"]), ptr(alphas), ptr(last), ptr(render), ptr(v_render), ptr(v_alphas), ptr(G), S, absgrad,
              ptr(o), None, 0, _st())
        assert is_canary(G[n * S:]) and (8 + DT == S or is_canary(rows[:, 8 + DT:])), f"{name}: pad written"
        assert absgrad or is_canary(rows[:, 2:4]), f"{name}: |xy| columns written without absgrad"
        got = host(rows)[:, :8 + DT]
        cols = None if absgrad else ("xy", "conic", "opacity", "channels")
        check_rows(f"{name} packed stride {S}", sc, got, bw["rows"], bw["rows_terms"], hit_any, cols=cols)


def test_clamp_blocks_sigma_and_opacity(hip_lib):
    """A cotangent on ONE pixel, where the list's first Gaussian has o exp(-sigma) > 0.999: its position, conic and opacity columns
    stay exactly 0.0 in both forms, its colour gradient is alpha T v, and the Gaussians behind it still receive theirs through
    the accumulated-behind term."""
    from mtgs_amd import _lib
    name = "edges-6t-d3"
    sc, fwd, _, _, fin, _, _, _ = R.reference(name)
    d = device_scene(name)
    tile = sc.marks["clamp_front"]
    g0 = int(sc.lists[tile][0])
    _, pix, px, py = R._pixels(sc, tile)
    raw = R._entry(sc, g0, px, py)[8]
    p0 = int(np.argmax(raw))
    f = fwd[tile]
    assert raw[p0] > R.ALPHA_MAX * (1 + 2 * R.CRIT_REL) and not f["critical"][p0] and f["last"][p0] > R.scene(name).starts()[0][tile] + 3
    vr = {t: np.zeros_like(x["render"], dtype=np.float32) for t, x in fwd.items()}
    va = {t: np.zeros_like(x["alpha"], dtype=np.float32) for t, x in fwd.items()}
    vr[tile][p0], va[tile][p0] = np.float32([0.75, -1.25, 0.5]), np.float32(0.625)
    want = R.backward(sc, fin, vr, va)
    assert not want["rows"][g0, :8].any() and want["rows"][g0, 8:].all() and np.count_nonzero(want["rows"][:, 7]) >= 3
    alphas, last, render, _, _ = backward_inputs(name)
    P = sc.C * sc.H * sc.W
    v_render, v_alphas = torch.zeros(P, sc.DT, device="cuda"), torch.zeros(P, device="cuda")
    v_render[int(pix[p0])] = up(vr[tile][p0])
    v_alphas[int(pix[p0])] = float(va[tile][p0])
    n = sc.n
    G = torch.zeros(n, 16, device="cuda")
    _call("mtgs_blend_bwd_packed", sc.C, sc.D, 0, ptr(d["rec"]), None, 0, sc.W, sc.H, sc.tw, sc.th, ptr(d["poff"]), ptr(d["pids"]), ptr(alphas),
          ptr(last), ptr(render), ptr(v_render), ptr(v_alphas), ptr(G), 16, 1, None, None, 0, _st())
    got = host(G)[:, :8 + sc.DT]
    assert not got[g0, :8].view(np.int32).any(), got[g0]
    check_rows(f"{name} packed, one clamped pixel", sc, got, want["rows"], want["rows_terms"], set(np.flatnonzero(want["rows_terms"].any(axis=1))))
    D6 = torch.zeros(n, 16, device="cuda")
    base = D6.data_ptr()
    _call("mtgs_blend_bwd", sc.C, n, sc.D, ptr(d["means"]), ptr(d["conics"]), ptr(d["colors"]), ptr(d["opac"]), None, None, 0, sc.W, sc.H, R.TS,
          sc.tw, sc.th, ptr(d["offsets"]), ptr(d["flat"]), d["M"], ptr(alphas), ptr(last), ptr(render), ptr(v_render), ptr(v_alphas), base,
          base + 8, base + 16, base + 32, None, base + 28, _lib.host_i64([16] * 6), None, None, _st())
    got = host(D6)[:, :8 + sc.DT]
    assert not got[g0, :8].view(np.int32).any(), got[g0]
    check_rows(f"{name} gather, one clamped pixel", sc, got, want["dense"], want["dense_terms"], set(np.flatnonzero(want["dense_terms"].any(axis=1))))


# ---- also_zero ----------------------------------------------------------------------------------------------------------------------
def _zero_region(nbytes):
    buf = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf


def _zeroed(buf, nbytes):
    return not bool(buf[:nbytes].any()) and bool((buf[nbytes:] == 0xA5).all())


def _packed_calls(sc, d, poff, C=None):
    """(forward, backward) closures of the packed entry points with an also_zero region."""
    C = sc.C if C is None else C
    P = sc.C * sc.H * sc.W
    alphas, last = torch.zeros(P, device="cuda"), torch.zeros(P, dtype=torch.int32, device="cuda")
    render, v_render, v_alphas = torch.zeros(P, sc.DT, device="cuda"), torch.ones(P, sc.DT, device="cuda"), torch.ones(P, device="cuda")
    G = torch.zeros(sc.n, 16, device="cuda")
    out = fcan(P * sc.DT), fcan(P), can(P)

    def f(z, nb):
        _call("mtgs_blend_fwd_packed", C, sc.D, int(sc.has_depth), ptr(d["rec"]), ptr(d["bg"]), int(sc.ed), sc.W, sc.H, sc.tw, sc.th,
              ptr(poff), ptr(d["pids"]), ptr(out[0]), ptr(out[1]), ptr(out[2]), None, z, nb, _st())

    def b(z, nb):
        _call("mtgs_blend_bwd_packed", C, sc.D, int(sc.has_depth), ptr(d["rec"]), ptr(d["bg"]), int(sc.ed), sc.W, sc.H, sc.tw, sc.th,
              ptr(poff), ptr(d["pids"]), ptr(alphas), ptr(last), ptr(render), ptr(v_render), ptr(v_alphas), ptr(G), 16, 1, None, z, nb, _st())
    return f, b


def test_also_zero(hip_lib):
    """The region the packed kernels clear while they run: one word, one word less than the launch has waves, a few words per wave
    plus one, just over 8 MiB per tile (cleared by the fill kernel instead); with lists, with every tile empty (the backward's
    early returns), and without cameras."""
    name = "edges-6t-d3"
    sc = R.scene(name)
    d = device_scene(name)
    waves = sc.tiles * 4                                   # fewer than 1536 tiles, at most 4 channels: four waves per tile both ways
    sizes = [16, 16 * (waves - 1), 16 * (waves * 3 + 1), sc.tiles * (8 << 20) + 16]
    empty = torch.zeros_like(d["poff"])
    for poff, C in ((d["poff"], None), (empty, None), (d["poff"], 0)):
        for call in _packed_calls(sc, d, poff, C):
            for nb in sizes:
                buf = _zero_region(nb)
                call(buf.data_ptr(), nb)
                assert _zeroed(buf, nb), (C, nb, "empty" if poff is empty else "lists")
                del buf


# ---- argument checks: an error code and no launch -----------------------------------------------------------------------------------
def test_argument_checks(hip_lib):
    name = "edges-6t-d3"
    sc = R.scene(name)
    d = device_scene(name)
    P = sc.C * sc.H * sc.W
    out = fcan(P * 9), fcan(P), can(P)
    z = torch.zeros(P * 9, device="cuda")
    zi = torch.zeros(P, dtype=torch.int32, device="cuda")
    G = fcan(sc.n * 24)

    def fwd(D=sc.D, depths=None, ed=0, W=sc.W, H=sc.H, ts=R.TS, tw=sc.tw, th=sc.th):
        _call("mtgs_blend_fwd", sc.C, sc.n, D, ptr(d["means"]), ptr(d["conics"]), ptr(z), ptr(d["opac"]), None, depths, ed, W, H, ts, tw, th,
              ptr(d["offsets"]), ptr(d["flat"]), d["M"], ptr(out[0]), ptr(out[1]), ptr(out[2]), None, _st())

    def bwd(D=sc.D, depths=None, ed=0, ts=R.TS, tw=sc.tw, th=sc.th):
        _call("mtgs_blend_bwd", sc.C, sc.n, D, ptr(d["means"]), ptr(d["conics"]), ptr(z), ptr(d["opac"]), None, depths, ed, sc.W, sc.H, ts, tw, th,
              ptr(d["offsets"]), ptr(d["flat"]), d["M"], ptr(z), ptr(zi), ptr(z), ptr(z), ptr(z), ptr(G), None, ptr(G), ptr(G), ptr(G), ptr(G),
              None, None, None, _st())

    def pfwd(D=sc.D, wd=0, ed=0, tw=sc.tw, th=sc.th, az=None, nb=0):
        _call("mtgs_blend_fwd_packed", sc.C, D, wd, ptr(d["rec"]), None, ed, sc.W, sc.H, tw, th, ptr(d["poff"]), ptr(d["pids"]), ptr(out[0]),
              ptr(out[1]), ptr(out[2]), None, az, nb, _st())

    def pbwd(D=sc.D, wd=0, ed=0, tw=sc.tw, th=sc.th, S=16, az=None, nb=0):
        _call("mtgs_blend_bwd_packed", sc.C, D, wd, ptr(d["rec"]), None, ed, sc.W, sc.H, tw, th, ptr(d["poff"]), ptr(d["pids"]), ptr(z), ptr(zi),
              ptr(z), ptr(z), ptr(z), ptr(G), S, 1, None, az, nb, _st())

    region = _zero_region(64)
    bad = [lambda: fwd(tw=sc.tw + 1), lambda: fwd(th=sc.th - 1), lambda: bwd(tw=sc.tw + 1), lambda: pfwd(th=sc.th + 1), lambda: pbwd(tw=sc.tw - 1),
           lambda: fwd(ts=8), lambda: bwd(ts=32),
           lambda: fwd(D=9), lambda: fwd(D=8, depths=ptr(d["opac"])), lambda: bwd(D=9), lambda: pfwd(D=9), lambda: pfwd(D=8, wd=1), lambda: pbwd(D=9),
           lambda: fwd(ed=1), lambda: bwd(ed=1), lambda: pfwd(ed=1), lambda: pbwd(ed=1),
           lambda: pbwd(S=8 + sc.D - 1), lambda: pbwd(D=7, wd=1, S=15),
           lambda: pfwd(az=region.data_ptr() + 4, nb=16), lambda: pfwd(az=region.data_ptr(), nb=24), lambda: pbwd(az=region.data_ptr() + 8, nb=16),
           lambda: pbwd(az=region.data_ptr(), nb=8)]
    for k, call in enumerate(bad):
        with pytest.raises(RuntimeError, match="failed"):
            call()
        assert k >= 0
    torch.cuda.synchronize()
    assert all(is_canary(t) for t in out) and is_canary(G) and bool((region == 0xA5).all())
