"""The projection kernels (csrc/project.hip, project_fwd_body.hpp, project_common.hpp, project_bwd.hip) called directly through the C
ABI on the scenes of tests/project_refs.py.

Forward: bit for bit against the C oracle (both round after every operation in one order), at block and camera edges and at every
cull comparison in equality and one ulp beside it.  Backward: against the float64 reference within
`project_refs.device_bound(constant)` x 2^-24 x the sum of |terms| of the very number compared, the constants being the C oracle's
own distance from the reference (measured by tests/test_project_refs_host.py, never against these kernels).  `radii` is an input of
the backward, so every visibility pattern is dictated here.

The canary rule of tests/test_gpu_bin_edges.py holds for every call: outputs have slack behind them and are pre-filled with one bit
pattern (zeros where the ABI asks the caller for zeros); what was written is asserted AND that everything else still holds the
pattern.

Which test reaches what in project_bwd.hip:
  project_bwd_kernel          test_dense_* (C up to 130: the camera slots and the slot beyond them), test_dense_chunk_loop (second round), test_flat_gaussians_comp_zero
  project_bwd_vis_kernel      test_compact_* (streaming, rows only, zeroed with and without raw rows, records, partial sums, device count),
                              test_compact_grid_stride (second round of 8192 blocks)
  project_bwd_expand_kernel   <1> x_channels 9 or no colours, <4> x_channels 1 and 4, <8> x_channels 5 and 8: test_compact_streaming
  viewmat_from_partials       test_compact_partial_sums, test_compact_grid_stride;  viewmat_reduce_kernel: rows only and zeroed with partials
  project_bwd_rows_kernel     test_wire_rows*"""
import functools
import itertools

import numpy as np
import pytest
import torch

from tests import project_refs as R
from tests.test_gpu_bin_edges import CAN, SL, _call, _st, can, host, up

pytestmark = pytest.mark.gpu

F = np.float32
EINVAL = 1
BOUND = {k: R.device_bound(v) for k, v in R.ORACLE_BWD.items()}
WIDTH = {"means": 3, "quats": 4, "scales": 3, "opacities": 1}
BIG, NVIS = R.BIG, R.NVIS


# ---- helpers ----------------------------------------------------------------------------------------------------------------------------
def fcan(n):
    """n floats and the slack behind them, every word the canary."""
    return can(int(n) + SL).view(torch.float32)


def fzero(n):
    """n zeros (what the ABI asks the caller for), the canary behind them."""
    t = fcan(n)
    t[:int(n)] = 0
    return t


def is_canary(t):
    return bool((t.contiguous().view(torch.int32) == CAN).all())


def bits(t):
    return t.contiguous().view(torch.int32)


def ptr(t):
    return None if t is None else t.data_ptr()


def i64(values):
    from mtgs_amd import _lib
    return _lib.host_i64(values)


def rc_of(name, *a):
    """The return code of an entry point that is expected to refuse its arguments."""
    from mtgs_amd import _lib
    return getattr(_lib.load(), name)(*a)


@functools.lru_cache(maxsize=None)
def dev(name):
    sc, f = R.scene(name), R.scene_forward(name)
    return dict(means=up(sc.means), quats=up(sc.quats), scales=up(sc.scales), opac=up(sc.opac), vm=up(sc.viewmats), K=up(sc.Ks),
                conics=up(f["conics32"]), comp=up(f["comp32"]))


def run_bwd(C, N, dv, radii, g, *, aa=True, vm=True, vopac=True, entry="mtgs_project_bwd", strides=None, row_index=None, x_abs=None,
            x_col=None, x_ch=0, x_strides=None, by=(), vis_ids=None, n_vis=0, ws=None, n_vis_dev=None, x_quat=None, x_mean=None,
            raw=None, recs=None, partials=None, dense=True, zeroed=False, rc=False):
    """One backward call; the outputs, each with its slack.  g: the incoming gradients (device tensors or views, None = absent)."""
    mk = fzero if zeroed else fcan
    o = dict(means=mk(N * 3) if dense else None, quats=mk(N * 4) if dense else None, scales=mk(N * 3) if dense else None,
             opacities=mk(N) if dense and vopac else None, viewmat=fcan(C * 16) if vm else None,
             d_m2d=mk(C * N * 2) if "m2d" in by else None, d_abs=mk(C * N * 2) if "abs" in by else None,
             d_col=mk(C * N * x_ch) if "col" in by else None)
    args = (C, N, ptr(dv["means"]), ptr(dv["quats"]), ptr(dv["scales"]), ptr(dv["vm"]), ptr(dv["K"]), R.W, R.H, R.EPS2D, ptr(radii),
            ptr(dv["conics"]), ptr(dv["comp"]) if aa else None, ptr(dv["opac"]), ptr(g["v_means2d"]), ptr(g["v_depths"]),
            ptr(g["v_conics"]), ptr(g.get("v_comp")), ptr(g.get("v_opac_eff")), ptr(o["means"]), ptr(o["quats"]), ptr(o["scales"]),
            ptr(o["viewmat"]), ptr(o["opacities"]), i64(strides), ptr(row_index), ptr(x_abs), ptr(x_col), x_ch, i64(x_strides),
            ptr(o["d_m2d"]), ptr(o["d_abs"]), ptr(o["d_col"]), ptr(vis_ids), n_vis, ptr(ws), ptr(n_vis_dev), ptr(x_quat), ptr(x_mean),
            ptr(raw), ptr(recs), ptr(partials), _st())
    if rc:
        return rc_of(entry, *args)
    _call(entry, *args)
    return o


def check(where, o, ref, C, N, names=("means", "quats", "scales", "opacities", "viewmat"), bound=None):
    """Every output that was asked for: within its bound of the reference (a number without a term: exactly zero), canary behind it."""
    report, bound = [], bound or BOUND
    for k in names:
        t = o.get(k)
        if t is None:
            continue
        n = C * 16 if k == "viewmat" else N * WIDTH[k]
        assert is_canary(t[n:]), f"{where}: wrote behind {k}"
        val, terms = ref[k] if k in ref else (np.zeros(N), np.zeros(N))      # (v_opacities without v_opac_eff: zeros)
        got = host(t[:n]).astype(np.float64).reshape(val.shape)
        assert np.isfinite(got).all(), f"{where}: NaN or inf in {k}"
        w = R.worst_ratio(got, val, terms) / bound[k]
        report.append(f"{k} {w:.3f}")
        if w > 1.0:
            err = np.abs(got - val) - bound[k] * R.B.EPS * terms
            at = np.unravel_index(int(np.argmax(err)), err.shape)
            raise AssertionError(f"{where}: {k} {w:.2f} x the bound at {at}: got {got[at]} want {val[at]} terms {terms[at]}")
    print(f"{where}: " + "  ".join(report) + " of the bound")


def dense_grads(name, with_vcomp=True, with_voe=True):
    cot = R.cotangents(name)
    g = {k: up(cot[k]) for k in ("v_means2d", "v_depths", "v_conics")}
    if with_vcomp:
        g["v_comp"] = up(cot["v_comp"])
    if with_voe:
        g["v_opac_eff"] = up(cot["v_opac_eff"])
    return g


# ---- forward ------------------------------------------------------------------------------------------------------------------------------
def run_fwd(C, N, a, *, eps2d=R.EPS2D, near=R.NEAR, far=R.FAR, clip=0.0, comp=True, opac_eff=True, tiles=True, W=R.W, H=R.H):
    """mtgs_project_fwd on host arrays a = (means, quats, scales, opac, viewmats, Ks): every output with its slack."""
    P = C * N
    d = [None if v is None else up(v) for v in a]
    o = dict(radii=can(P + SL), means2d=fcan(P * 2), depths=fcan(P), conics=fcan(P * 3), comp=fcan(P) if comp else None,
             opac_eff=fcan(P) if opac_eff else None, tiles=can(P + SL) if tiles else None)
    tw, th = (W + 15) // 16, (H + 15) // 16
    _call("mtgs_project_fwd", C, N, ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[4]), ptr(d[5]), W, H, eps2d, near, far, clip, ptr(d[3]),
          ptr(o["radii"]), ptr(o["means2d"]), ptr(o["depths"]), ptr(o["conics"]), ptr(o["comp"]), ptr(o["opac_eff"]), 16, tw, th,
          ptr(o["tiles"]), _st())
    return o


def check_fwd(where, oracle, C, N, a, o, **kw):
    """Bit for bit the oracle's, culled rows +0 in every float output, opac_eff and the tile counts as documented."""
    means, quats, scales, opac, vm, K = a
    W, H = kw.get("W", R.W), kw.get("H", R.H)
    P = C * N
    ref = oracle.project_fwd(means, quats, scales, vm, K, W, H, eps2d=kw.get("eps2d", R.EPS2D), near=kw.get("near", R.NEAR),
                             far=kw.get("far", R.FAR), radius_clip=kw.get("clip", 0.0), calc_compensations=True)
    radii = host(o["radii"])
    assert np.array_equal(radii[:P], ref[0].reshape(-1)) and (radii[P:] == CAN).all(), where + ": radii"
    for key, r, w in (("means2d", ref[1], 2), ("depths", ref[2], 1), ("conics", ref[3], 3), ("comp", ref[4], 1)):
        if o[key] is None:
            continue
        got = host(bits(o[key]))
        assert np.array_equal(got[:P * w], np.ascontiguousarray(r).view(np.int32).reshape(-1)), f"{where}: {key} not bit-exact"
        assert (got[P * w:] == CAN).all(), f"{where}: wrote behind {key}"
        assert not got[:P * w].reshape(P, w)[radii[:P] == 0].any(), f"{where}: culled rows of {key} are not +0"
    if o["opac_eff"] is not None:
        want = np.where(ref[0] > 0, opac[None] * ref[4] if o["comp"] is not None else np.broadcast_to(opac[None], (C, N)), F(0)).astype(F)
        got = host(bits(o["opac_eff"]))
        assert np.array_equal(got[:P], want.view(np.int32).reshape(-1)) and (got[P:] == CAN).all(), where + ": opac_eff"
    if o["tiles"] is not None:
        cnt = can(P + SL)
        _call("mtgs_isect_count", C, N, ptr(o["means2d"]), ptr(o["radii"]), 16, (W + 15) // 16, (H + 15) // 16, ptr(cnt), _st())
        assert torch.equal(cnt, o["tiles"]), where + ": tiles_per_gauss differs from mtgs_isect_count"
        assert not host(cnt)[:P][radii[:P] == 0].any()
    return ref


def forward_arrays(C, N, seed=0):
    """N Gaussians of the large scene in front of the first C cameras of c3-n257, every fifth one enlarged: on the screen, off each of its
    edges, and reaching it only through their radius."""
    a, b = R.scene("c3-n257"), R.scene(BIG)
    pick = np.random.RandomState(seed).permutation(b.N)[:N]
    scales = b.scales[pick].copy()
    scales[::5] *= 4.0
    return b.means[pick], b.quats[pick], scales, b.opac[pick], a.viewmats[:C], a.Ks[:C]


@pytest.mark.parametrize("C,N", [(1, 1), (1, 255), (1, 256), (1, 257), (3, 257), (2, 1301)])
@pytest.mark.parametrize("comp", [True, False])
def test_forward_sizes(hip_lib, oracle, C, N, comp):
    """One thread per pair: the last block partly filled, and with C = 3, N = 257 a block on two cameras (idx / N)."""
    a = forward_arrays(C, N)
    o = run_fwd(C, N, a, comp=comp)
    ref = check_fwd(f"C={C} N={N} comp={comp}", oracle, C, N, a, o)
    if N > 200:
        vis = ref[0] > 0
        assert 0.15 < vis.mean() < 0.95, "culled and kept pairs in one launch"
        tiles = host(o["tiles"])[:C * N].reshape(C, N)
        full = (-(-2 * ref[0] // 16)) ** 2                      # an interval of 2 r pixels covers at least ceil(2 r / 16) tiles
        assert (vis & (tiles < full)).sum() > 5, "rectangles clipped at an image border"
        m2, r = ref[1], ref[0]
        for what, cut in (("left", m2[..., 0] - r < 0), ("right", m2[..., 0] + r > R.W), ("top", m2[..., 1] - r < 0),
                          ("bottom", m2[..., 1] + r > R.H)):
            assert (vis & cut).any(), f"no rectangle clipped at the {what} border"


@pytest.mark.parametrize("C,N", [(0, 5), (3, 0)])
def test_forward_of_nothing(hip_lib, C, N):
    a = forward_arrays(max(C, 1), max(N, 1))
    d = [up(v) for v in a]
    outs = [can(8), fcan(8), fcan(8), fcan(8), fcan(8), fcan(8), can(8)]
    _call("mtgs_project_fwd", C, N, ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[4]), ptr(d[5]), R.W, R.H, R.EPS2D, R.NEAR, R.FAR, 0.0,
          ptr(d[3]), ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), ptr(outs[3]), ptr(outs[4]), ptr(outs[5]), 16, 10, 6, ptr(outs[6]), _st())
    assert all(is_canary(t) for t in outs)


# A camera of exactly representable numbers: identity pose, fx = fy = 64, cx = cy = 32, 64 x 64 pixels, depth 1: means2d = 64 x + 32 exactly.
EW = EH = 64
EK = np.array([[[64, 0, 32], [0, 64, 32], [0, 0, 1]]], dtype=F)
EVM = np.eye(4, dtype=F)[None]


def _edge_arrays(means, scales=None, quats=None):
    n = len(means)
    means = np.asarray(means, dtype=F).reshape(n, 3)
    scales = np.full((n, 3), 0.03, F) if scales is None else np.asarray(scales, dtype=F).reshape(n, 3)
    quats = np.tile(np.array([[1, 0, 0, 0]], F), (n, 1)) if quats is None else np.asarray(quats, dtype=F).reshape(n, 4)
    return means, quats, scales, np.full(n, 0.5, F), EVM, EK


def test_forward_cull_edges(hip_lib, oracle):
    """z == near and z == far are kept, one ulp outside is culled; a NaN mean passes the depth test and falls at det > 0; a zero
    quaternion; eps2d = 0 with a zero scale (det == 0); radius_clip equal to a radius."""
    near, far = F(0.5), F(8.0)
    up1, dn1 = (lambda v: np.nextafter(F(v), F(np.inf))), (lambda v: np.nextafter(F(v), F(-np.inf)))
    means = [(0, 0, near), (0, 0, dn1(near)), (0, 0, far), (0, 0, up1(far)), (np.nan, 0, 2), (0, 0, np.nan), (0.1, 0, 2), (0, 0.1, 2)]
    quats = [(1, 0, 0, 0)] * 6 + [(0, 0, 0, 0), (2, 0, 0, 0)]
    a = _edge_arrays(means, quats=quats)
    kw = dict(near=float(near), far=float(far), W=EW, H=EH)
    o = run_fwd(1, len(means), a, **kw)
    ref = check_fwd("planes", oracle, 1, len(means), a, o, **kw)
    assert (ref[0][0] > 0).tolist() == [True, False, True, False, False, False, False, True]
    # det == 0: no blur and no extent
    a = _edge_arrays([(0, 0, 2), (0, 0, 2)], scales=[(0, 0, 0), (0.05, 0.05, 0.05)])
    kw = dict(eps2d=0.0, W=EW, H=EH)
    o = run_fwd(1, 2, a, **kw)
    ref = check_fwd("det == 0", oracle, 1, 2, a, o, **kw)
    assert (ref[0][0] > 0).tolist() == [False, True]
    # radius_clip: radius <= clip culls
    a = _edge_arrays([(0, 0, 2), (0, 0, 1)], scales=[(0.1, 0.1, 0.1), (0.3, 0.3, 0.3)])
    r0 = oracle.project_fwd(a[0], a[1], a[2], EVM, EK, EW, EH)[0][0]
    assert 0 < r0[0] < r0[1]
    for clip, want in ((float(r0[0]), [False, True]), (float(r0[0]) - 0.5, [True, True]), (float(r0[1]), [False, False])):
        kw = dict(clip=clip, W=EW, H=EH)
        o = run_fwd(1, 2, a, **kw)
        ref = check_fwd(f"radius_clip {clip}", oracle, 1, 2, a, o, **kw)
        assert (ref[0][0] > 0).tolist() == want


def _radius_at(oracle, x, y):
    a = _edge_arrays([(x, y, 1)])
    return int(oracle.project_fwd(a[0], a[1], a[2], EVM, EK, EW, EH)[0][0, 0])


def test_forward_screen_edges(hip_lib, oracle):
    """mean + radius <= 0 and mean - radius >= size on both axes: at equality the pair is culled, with the projected mean one ulp inside
    it is kept.  64 x + 32 is exact at the edge, so equality is equality in the kernel's own arithmetic."""
    means, want = [], []
    for axis, side in itertools.product((0, 1), (-1, 1)):
        r = 5
        for _ in range(4):                 # the radius depends on the position through the Jacobian's third column: a fixed point,
            x = (-r - 32) / 64.0 if side < 0 else (64 + r - 32) / 64.0      # read one ulp inside, where the pair is kept
            inside = F(x)
            while F(64) * inside + F(32) == F(64) * F(x) + F(32):          # (one ulp of the PROJECTED mean, which is coarser beyond 64)
                inside = np.nextafter(inside, F(0.0))
            r2 = _radius_at(oracle, *((inside, 0.0) if axis == 0 else (0.0, inside)))
            if r2 == r:
                break
            r = r2
        assert r2 == r and abs(x) < 0.64, "no fixed point of the radius inside the clamp"
        for v, keep in ((x, False), (inside, True)):
            means.append((v, 0, 1) if axis == 0 else (0, v, 1))
            want.append(keep)
    a = _edge_arrays(means)
    kw = dict(W=EW, H=EH)
    o = run_fwd(1, len(means), a, **kw)
    ref = check_fwd("screen edges", oracle, 1, len(means), a, o, **kw)
    assert (ref[0][0] > 0).tolist() == want
    tiles = host(o["tiles"])[:len(means)]
    assert (tiles[np.array(want)] >= 1).all()


# ---- backward, dense kernel ---------------------------------------------------------------------------------------------------------------
def _dense_cases():
    out = []
    for name in R.SCENES:
        sc = R.scene(name)
        keys = list(sc.masks) if sc.C < 60 else [k for k in sc.masks if k in ("none", "all", "mixed", "one-camera", "one@0", "one@63", "wave3")]
        out += [(name, k) for k in keys]
    return out


@pytest.mark.parametrize("name,mask", _dense_cases())
def test_dense_patterns(hip_lib, name, mask):
    """Every scene (N on both sides of the block, C = 65 and 130 beyond the 64 camera slots) with every visibility pattern: nothing
    visible, everything, one pair at thread 0 / 63 / 64 / 255, waves 0-2 empty, one camera only."""
    sc, dv = R.scene(name), dev(name)
    radii = up(sc.masks[mask].astype(np.int32) * 3)
    o = run_bwd(sc.C, sc.N, dv, radii, dense_grads(name))
    ref = R.reference(name, mask)
    check(f"{name} {mask}", o, ref, sc.C, sc.N)
    if mask == "none":
        assert not any(bits(o[k][:n]).any() for k, n in (("means", sc.N * 3), ("quats", sc.N * 4), ("scales", sc.N * 3), ("opacities", sc.N),
                                                         ("viewmat", sc.C * 16)))


@pytest.mark.parametrize("vm", [True, False])
@pytest.mark.parametrize("aa,vcomp,voe", [(True, True, True), (True, False, True), (True, True, False), (True, False, False),
                                          (False, False, True), (False, False, False)])
def test_dense_options(hip_lib, aa, vcomp, voe, vm):
    name, mask = "c3-n257", "mixed"
    sc, dv = R.scene(name), dev(name)
    radii = up(sc.masks[mask].astype(np.int32))
    o = run_bwd(sc.C, sc.N, dv, radii, dense_grads(name, vcomp, voe), aa=aa, vm=vm)
    check(f"aa={aa} v_comp={vcomp} v_opac_eff={voe} vm={vm}", o, R.reference(name, mask, aa, vcomp, voe), sc.C, sc.N)
    # without v_opacities (and therefore without v_opac_eff)
    if not voe:
        o = run_bwd(sc.C, sc.N, dv, radii, dense_grads(name, vcomp, False), aa=aa, vm=vm, vopac=False)
        check("v_opacities NULL", o, R.reference(name, mask, aa, vcomp, False), sc.C, sc.N)


def _interleaved(name, perm_seed):
    """The gradients of a scene as rows of ONE buffer of 16 floats [m2d 2 | abs 2 | conic 3 | opac_eff | colours 4 | depth | comp | 2 pad],
    row of pair idx = perm[idx]; one more row of NaN behind them, where the index of every culled pair points."""
    sc, cot = R.scene(name), R.cotangents(name)
    P = sc.C * sc.N
    r = np.random.RandomState(perm_seed)
    perm = r.permutation(P).astype(np.int32) if perm_seed else np.arange(P, dtype=np.int32)
    buf = np.full((P + 1, 16), np.nan, F)
    rows = np.zeros((P, 16), F)
    rows[:, 0:2], rows[:, 4:7], rows[:, 7] = cot["v_means2d"].reshape(P, 2), cot["v_conics"].reshape(P, 3), cot["v_opac_eff"].reshape(P)
    rows[:, 2:4], rows[:, 8:12] = r.uniform(0, 1, (P, 2)), r.standard_normal((P, 4))
    rows[:, 12], rows[:, 13] = cot["v_depths"].reshape(P), cot["v_comp"].reshape(P)
    buf[perm] = rows
    return perm, rows, up(buf)


@pytest.mark.parametrize("perm_seed", [0, 5])
@pytest.mark.parametrize("x_ch", [1, 4, 5, 8, 9])
def test_dense_interleaved_rows_and_byproducts(hip_lib, perm_seed, x_ch):
    """grad_row_strides of an interleaved buffer, grad_row_index as a permutation, the three dense by-products with their zeros at
    culled pairs; x_channels up to 9 (the colour source then runs over the row's later columns: any floats will do)."""
    name, mask = "c2-n600", "mixed"
    sc, dv = R.scene(name), dev(name)
    P = sc.C * sc.N
    vis = sc.masks[mask].reshape(-1)
    perm, rows, buf = _interleaved(name, perm_seed)
    index = np.where(vis, perm, P).astype(np.int32)
    flat = buf.view(-1)
    g = dict(v_means2d=flat[0:], v_conics=flat[4:], v_opac_eff=flat[7:], v_depths=flat[12:], v_comp=flat[13:])
    col0 = 7 if x_ch == 9 else 8                              # nine channels: columns 7 .. 15
    o = run_bwd(sc.C, sc.N, dv, up(vis.astype(np.int32)), g, strides=[16] * 5, row_index=up(index) if perm_seed else None,
                x_abs=flat[2:], x_col=flat[col0:], x_ch=x_ch, x_strides=[16, 16], by=("m2d", "abs", "col"))
    check(f"interleaved perm={perm_seed} x_channels={x_ch}", o, R.reference(name, mask), sc.C, sc.N)
    for key, lo, hi in (("d_m2d", 0, 2), ("d_abs", 2, 4), ("d_col", col0, col0 + x_ch)):
        want = np.where(vis[:, None], rows[:, lo:hi], F(0)).astype(F)
        got = host(bits(o[key]))
        n = P * (hi - lo)
        assert np.array_equal(got[:n], want.view(np.int32).reshape(-1)) and (got[n:] == CAN).all(), key


def _placed(N, idx, name="c1-n600"):
    """The first len(idx) Gaussians of a scene at the places idx of otherwise zero-filled arrays of N: device inputs, radii, the
    cotangents of those rows and the per-pair derivatives."""
    sc, f, cot = R.scene(name), R.scene_forward(name), R.cotangents(name)
    k = len(idx)
    at = torch.from_numpy(np.asarray(idx, dtype=np.int64)).cuda()
    dv = dict(vm=up(sc.viewmats), K=up(sc.Ks))
    for key, src, w in (("means", sc.means, 3), ("quats", sc.quats, 4), ("scales", sc.scales, 3), ("opac", sc.opac, 0),
                        ("conics", f["conics32"][0], 3), ("comp", f["comp32"][0], 0)):
        t = torch.zeros((N, w) if w else (N,), device="cuda")
        t[at] = up(src[:k])
        dv[key] = t
    d = R.derivatives(sc.means, sc.quats, sc.scales, sc.viewmats, sc.Ks, np.zeros(k, np.int64), np.arange(k))
    V, M = R.cotangent_matrix(d, sc.opac, cot["v_means2d"], cot["v_depths"], cot["v_conics"], cot["v_comp"], cot["v_opac_eff"], True)
    ref = R.backward(1, k, d, V, M, sc.opac, cot["v_opac_eff"], True)
    rows = {key: cot[key][0, :k] for key in ("v_means2d", "v_depths", "v_conics", "v_comp", "v_opac_eff")}
    return dv, at, rows, ref


def check_placed(where, o, ref, N, at, k):
    """The rows `at` of the dense outputs against the reference of the k placed Gaussians; every other row exactly +0.0."""
    sub = {}
    for key, w in WIDTH.items():
        t = o[key]
        assert is_canary(t[N * w:]), f"{where}: wrote behind {key}"
        rows = t[:N * w].view(N, w)
        sub[key] = torch.cat([rows[at].reshape(-1), can(SL).view(torch.float32)])
        rest = bits(rows).clone()
        rest[at] = 0
        assert not bool(rest.any()), f"{where}: {key} is not exactly zero outside the rows with a gradient"
    sub["viewmat"] = o["viewmat"]
    check(where, sub, ref, 1, k)


def test_dense_chunk_loop(hip_lib):
    """2048 blocks x 256 + 300 Gaussians: blocks 0 and 1 take a second round, the last one partly filled.  Visible: 200 scattered over the
    first round, 200 in block 0's second round, all 44 of the last partial chunk."""
    N = 2048 * 256 + 300
    r = np.random.RandomState(3)
    idx = np.concatenate([np.sort(r.choice(2048 * 256, 200, replace=False)), 2048 * 256 + np.sort(r.choice(256, 200, replace=False)),
                          np.arange(2048 * 256 + 256, N)])
    k = idx.size
    dv, at, rows, ref = _placed(N, idx)
    radii = torch.zeros(N, dtype=torch.int32, device="cuda")
    radii[at] = 2
    g = {}
    for key, v in rows.items():
        t = torch.zeros((N,) + v.shape[1:], device="cuda")
        t[at] = up(v)
        g[key] = t
    o = run_bwd(1, N, dv, radii, g)
    check_placed("chunk loop", o, ref, N, at, k)


def test_flat_gaussians_comp_zero(hip_lib, oracle):
    """comp == 0 (two zero scales: det_orig <= 0 before the blur, eps2d > 0): the forward bit for bit the oracle's, compensation 0
    included, and the backward -- where the division by comp + 1e-6 decides and autograd has no derivative -- against the oracle's
    project_bwd within (device_bound(c) + c) x 2^-24 terms, c = ORACLE_BWD_FLAT, in the dense kernel and the compact path."""
    a, fwd, mask, cot, ref = R.flat_case(oracle.project_fwd)
    n = a[0].shape[0]
    o = run_fwd(1, n, a)
    check_fwd("flat Gaussians", oracle, 1, n, a, o)
    assert (host(bits(o["comp"]))[:n][mask[0]] == 0).all() and mask.sum() >= 10
    want = R.oracle_flat(oracle)
    dv = dict(means=up(a[0]), quats=up(a[1]), scales=up(a[2]), opac=up(a[3]), vm=up(a[4]), K=up(a[5]), conics=up(fwd[3]), comp=up(fwd[4]))
    g = {k: up(v) for k, v in cot.items()}
    radii = up(mask.astype(np.int32))
    ids = np.flatnonzero(mask[0]).astype(np.int32)
    index = np.full(n, CAN, np.int32)
    index[ids] = np.arange(ids.size)
    rows = {k: up(np.ascontiguousarray(v[0, ids])) for k, v in cot.items()}
    ws = fcan(ids.size * 12)
    for where, out in (("flat dense", run_bwd(1, n, dv, radii, g)),
                       ("flat compact", run_bwd(1, n, dv, radii, rows, row_index=up(index), vis_ids=up(ids), n_vis=ids.size, ws=ws))):
        for k, w in dict(WIDTH, viewmat=16).items():
            size = w if k == "viewmat" else n * w
            assert is_canary(out[k][size:]), f"{where}: wrote behind {k}"
            got = host(out[k][:size]).astype(np.float64).reshape(ref[k][0].shape)
            c = R.ORACLE_BWD_FLAT[k]
            r_orc = R.worst_ratio(got, want[k].astype(np.float64).reshape(got.shape), ref[k][1]) / (R.device_bound(c) + c)
            r_ref = R.worst_ratio(got, *ref[k]) / R.device_bound(c)
            print(f"{where}: {k} {r_orc:.3f} of the bound against the oracle, {r_ref:.3f} against the reference")
            assert r_orc <= 1.0 and r_ref <= 1.0, f"{where}: {k} {r_orc:.2f} / {r_ref:.2f} x the bound"
        assert bool((out["opacities"][:n] == 0).all()), "v_opacities = v_opac_eff x 0"
    assert is_canary(ws[ids.size * 12:])


# ---- backward, compact path -----------------------------------------------------------------------------------------------------------------
def compact_device(n_vis, ids):
    sc = R.scene(BIG)
    radii = np.zeros(sc.N, np.int32)
    radii[ids] = 4
    index = np.full(sc.N, CAN, np.int32)                      # (read for the visible Gaussians only)
    index[ids] = np.arange(n_vis)
    return up(radii), up(index), up(ids)


def check_ws(where, ws, n, ref, ids):
    assert is_canary(ws[n * 12:]), where + ": wrote behind vis_ws"
    got = host(ws[:n * 12]).astype(np.float64).reshape(n, 12)
    val, terms = R.ws_rows(ref, ids[:n])
    for name, lo, hi in (("means", 0, 3), ("quats", 3, 7), ("scales", 7, 10), ("opacities", 10, 12)):
        w = R.worst_ratio(got[:, lo:hi], val[:, lo:hi], terms[:, lo:hi]) / BOUND[name]
        assert w <= 1.0, f"{where}: workspace rows, {name}: {w:.2f} x the bound"


@pytest.mark.parametrize("n_vis,x_ch", list(zip(NVIS, (1, 4, 5, 8, 9))) + [(257, 1), (513, 4), (255, 8), (256, 9), (1, 5)])
def test_compact_streaming(hip_lib, n_vis, x_ch):
    """The per-visible pass and the streaming pass behind it, N = 1301 (no multiple of 4 or 256): rows that are zero, rows that live
    through one cotangent only, the x_* addends, the by-products through every instantiation of the streaming pass (x_channels 1, 4 ->
    <4>; 5, 8 -> <8>; 9 -> <1> with per-lane colour stores)."""
    sc, dv = R.scene(BIG), dev(BIG)
    N = sc.N
    ids, rows, zero, d, _ = R.compact_case(n_vis)
    radii, index, vis_ids = compact_device(n_vis, ids)
    t = {k: up(v) for k, v in rows.items()}
    ws = fcan(n_vis * 12)
    o = run_bwd(1, N, dv, radii, t, row_index=index, vis_ids=vis_ids, n_vis=n_vis, ws=ws, x_quat=t["x_quat"], x_mean=t["x_mean"],
                x_abs=t["x_abs"], x_col=t["x_col"], x_ch=x_ch, x_strides=[2, 12], by=("m2d", "abs", "col"))
    ref = R.compact_reference(rows, ids, d)
    where = f"compact n_vis={n_vis} x_channels={x_ch}"
    check(where, o, ref, 1, N)
    check_ws(where, ws, n_vis, ref, ids)
    for key, src in (("d_m2d", rows["v_means2d"]), ("d_abs", rows["x_abs"]), ("d_col", rows["x_col"][:, :x_ch])):
        want = R.scatter(N, ids, np.ascontiguousarray(src))[0]
        got = host(bits(o[key]))
        assert np.array_equal(got[:want.size], want.view(np.int32).reshape(-1)) and (got[want.size:] == CAN).all(), f"{where}: {key}"
    # the rows that are zero in everything: exactly zero results
    dead = ids[zero]
    for key, w in WIDTH.items():
        assert not bits(o[key][:N * w].view(N, w)[torch.from_numpy(dead.astype(np.int64)).cuda()]).any(), f"{where}: {key} of zero rows"
    # v_opacities NULL (and no v_opac_eff), classic mode, no addends
    g = {k: t[k] for k in ("v_means2d", "v_depths", "v_conics")}
    ws = fcan(n_vis * 12)
    o = run_bwd(1, N, dv, radii, g, aa=False, vopac=False, row_index=index, vis_ids=vis_ids, n_vis=n_vis, ws=ws)
    check(where + " classic, v_opacities NULL", o, R.compact_reference(rows, ids, d, False, False, False, False, False), 1, N)


def test_compact_all_rows_zero(hip_lib):
    """count == 0 in every block: all outputs zero, v_viewmats zero, and vm_partials still written in full."""
    sc, dv = R.scene(BIG), dev(BIG)
    n_vis = 513
    ids, rows, _, d, _ = R.compact_case(n_vis)
    radii, index, vis_ids = compact_device(n_vis, ids)
    t = {k: torch.zeros_like(up(v)) for k, v in rows.items()}
    blocks = hip_blocks(n_vis)
    assert blocks == 3
    for partials in (None, fcan(12 * blocks)):
        ws = fcan(n_vis * 12)
        o = run_bwd(1, sc.N, dv, radii, t, row_index=index, vis_ids=vis_ids, n_vis=n_vis, ws=ws, x_quat=t["x_quat"], x_mean=t["x_mean"],
                    partials=partials)
        for key, n in (("means", sc.N * 3), ("quats", sc.N * 4), ("scales", sc.N * 3), ("opacities", sc.N), ("viewmat", 16)):
            assert not bits(o[key][:n]).any() and is_canary(o[key][n:]), key
        assert not bits(ws[:n_vis * 12]).any() and is_canary(ws[n_vis * 12:])
        if partials is not None:
            assert not bits(partials[:12 * blocks]).any() and is_canary(partials[12 * blocks:])


def hip_blocks(n_vis):
    import ctypes
    b = ctypes.c_int64(-1)
    _call("mtgs_project_bwd_blocks", n_vis, ctypes.byref(b))
    return int(b.value)


def test_blocks_query(hip_lib):
    assert [hip_blocks(n) for n in (0, 1, 256, 257, 8192 * 256, 8192 * 256 + 1, 1 << 30)] == [1, 1, 1, 2, 8192, 8192, 8192]


@pytest.mark.parametrize("n_vis", NVIS)
@pytest.mark.parametrize("with_recs,zeroed", [(False, False), (True, False), (True, True), (False, True)])
def test_compact_raw_rows(hip_lib, n_vis, with_recs, zeroed):
    """Raw-moment rows: converted in place to the documented meaning and used as the incoming gradients; with `recs` the conic and the
    blended opacity come from the record (the dense conics are NaN then).  In the zeroed form the absgrad by-product comes out of the
    conversion and the dense stores follow it: the combination the fused path runs."""
    sc, dv = R.scene(BIG), dict(dev(BIG))
    N = sc.N
    ids, _, zero, d, _ = R.compact_case(n_vis)
    G, v_comp = R.raw_case(n_vis)
    rows, mags, conv, mag = R.row_gradients(G, ids, True, depth_col=11, v_comp=v_comp)
    radii, index, vis_ids = compact_device(n_vis, ids)
    recs = None
    if with_recs:
        rec = np.zeros((n_vis, 16), F)
        rec[:, 2:5], rec[:, 5] = R.scene_forward(BIG)["conics32"][0, ids], R.blended_opacity(ids)
        recs = up(rec)
        dv["conics"] = torch.full_like(dv["conics"], float("nan"))
    buf = torch.cat([up(G).view(-1), can(SL).view(torch.float32)])
    g = dict(v_means2d=buf[0:], v_conics=buf[4:], v_opac_eff=buf[7:], v_depths=buf[11:], v_comp=up(v_comp))
    ws = fcan(n_vis * 12)
    o = run_bwd(1, N, dv, radii, g, strides=[12, 12, 12, 1, 12], row_index=index, vis_ids=vis_ids, n_vis=n_vis, ws=ws, raw=buf,
                recs=recs, x_abs=buf[2:], x_col=buf[8:], x_ch=3, x_strides=[12, 12], by=("m2d", "abs", "col"), zeroed=zeroed,
                entry="mtgs_project_bwd_zeroed" if zeroed else "mtgs_project_bwd")
    where = f"raw rows n_vis={n_vis} recs={with_recs} zeroed={zeroed}"
    # the rows read back converted: [v_xy | |v_xy| | v_conic | v_opacity_eff], the rest of the row and the zero rows untouched
    assert is_canary(buf[n_vis * 12:])
    back = host(buf[:n_vis * 12]).reshape(n_vis, 12)
    assert np.array_equal(back[:, 7:].view(np.int32), G[:, 7:].view(np.int32)) and not back[zero].view(np.int32).any(), where
    w = R.worst_ratio(back[:, :7], conv[:, :7], mag[:, :7]) / R.device_bound(1.0)
    assert w <= 1.0, f"{where}: converted rows {w:.2f} x the bound"
    ref = R.compact_reference(rows, ids, d, xq=False, xm=False, mags=mags)
    check(where, o, ref, 1, N)
    if zeroed:
        assert is_canary(ws), where + ": vis_ws was written"
    else:
        check_ws(where, ws, n_vis, ref, ids)
    for key, lo, hi in (("d_m2d", 0, 2), ("d_abs", 2, 4), ("d_col", 8, 11)):
        want = R.scatter(N, ids, np.ascontiguousarray(back[:, lo:hi]))[0].reshape(-1)
        got = host(o[key])
        assert (host(bits(o[key]))[want.size:] == CAN).all(), f"{where}: wrote behind {key}"
        if zeroed:      # (a -0.0 of the conversion is not stored over the caller's +0.0)
            assert np.array_equal(got[:want.size], want) and not np.signbit(got[:want.size][want == 0]).any(), f"{where}: {key}"
        else:
            assert np.array_equal(got[:want.size].view(np.int32), want.view(np.int32)), f"{where}: {key}"


@pytest.mark.parametrize("n_vis", [257, 513])
def test_compact_partial_sums(hip_lib, n_vis):
    """vm_partials: the camera's gradient within the bound like the atomic form, and bit for bit the same over three repeats."""
    sc, dv = R.scene(BIG), dev(BIG)
    ids, rows, _, d, _ = R.compact_case(n_vis)
    radii, index, vis_ids = compact_device(n_vis, ids)
    t = {k: up(v) for k, v in rows.items()}
    ref = R.compact_reference(rows, ids, d)
    blocks = hip_blocks(n_vis)
    seen = []
    for rep in range(3):
        partials, ws = fcan(12 * blocks), fcan(n_vis * 12)
        o = run_bwd(1, sc.N, dv, radii, t, row_index=index, vis_ids=vis_ids, n_vis=n_vis, ws=ws, x_quat=t["x_quat"], x_mean=t["x_mean"],
                    partials=partials)
        check(f"partial sums n_vis={n_vis}", o, ref, 1, sc.N)
        assert is_canary(partials[12 * blocks:]) and not bool((bits(partials[:12 * blocks]) == CAN).any()), "every block leaves its 12 sums"
        seen.append(bits(o["viewmat"]).clone())
    assert torch.equal(seen[0], seen[1]) and torch.equal(seen[0], seen[2])
    assert bool(seen[0][:16].any())
    # rows only with partial sums: viewmat_reduce_kernel
    partials, ws = fcan(12 * blocks), fcan(n_vis * 12)
    o = run_bwd(1, sc.N, dv, radii, t, row_index=index, vis_ids=vis_ids, n_vis=n_vis, ws=ws, x_quat=t["x_quat"], x_mean=t["x_mean"],
                partials=partials, dense=False)
    check("rows only, partial sums", o, ref, 1, sc.N, names=("viewmat",))
    check_ws("rows only, partial sums", ws, n_vis, ref, ids)


def test_compact_device_count(hip_lib):
    """n_vis_dev below the capacity: rows behind the count are not read (they hold NaN) and not written in vis_ws; radii > 0 only for
    the Gaussians that have a row below the count, as the contract asks."""
    sc, dv = R.scene(BIG), dev(BIG)
    cap, count = 513, 300
    ids, rows, _, d, _ = R.compact_case(cap)
    radii, index, vis_ids = compact_device(cap, ids)
    radii[torch.from_numpy(ids[count:].astype(np.int64)).cuda()] = 0
    live = {k: v.copy() for k, v in rows.items()}
    t = {}
    for k, v in rows.items():
        p = v.copy()
        p[count:] = np.nan
        live[k][count:] = 0
        t[k] = up(p)
    n_vis_dev = up(np.array([(count << 32) | 12345], dtype=np.int64))
    ws = fcan(cap * 12)
    o = run_bwd(1, sc.N, dv, radii, t, row_index=index, vis_ids=vis_ids, n_vis=cap, ws=ws, n_vis_dev=n_vis_dev, x_quat=t["x_quat"],
                x_mean=t["x_mean"])
    d300 = R.derivatives(sc.means, sc.quats, sc.scales, sc.viewmats, sc.Ks, np.zeros(count, np.int64), ids[:count])
    ref = R.compact_reference({k: v[:count] for k, v in live.items()}, ids[:count], d300)
    check("device count", o, ref, 1, sc.N)
    assert is_canary(ws[count * 12:]), "rows behind the device count were written"
    check_ws("device count", ws, count, ref, ids)


@pytest.mark.parametrize("n_vis", NVIS)
def test_compact_rows_only(hip_lib, n_vis):
    """No dense output at all: vis_ws is the result."""
    sc, dv = R.scene(BIG), dev(BIG)
    ids, rows, _, d, _ = R.compact_case(n_vis)
    radii, index, vis_ids = compact_device(n_vis, ids)
    t = {k: up(v) for k, v in rows.items()}
    ws = fcan(n_vis * 12)
    o = run_bwd(1, sc.N, dv, radii, t, row_index=index, vis_ids=vis_ids, n_vis=n_vis, ws=ws, x_quat=t["x_quat"], x_mean=t["x_mean"], dense=False)
    ref = R.compact_reference(rows, ids, d)
    check(f"rows only n_vis={n_vis}", o, ref, 1, sc.N, names=("viewmat",))
    check_ws(f"rows only n_vis={n_vis}", ws, n_vis, ref, ids)
    assert not bits(ws[:n_vis * 12].view(n_vis, 12)[:, 11]).any(), "the pad column is +0"


@pytest.mark.parametrize("n_vis,x_ch,partials", [(1, 1, False), (255, 4, True), (256, 5, False), (257, 8, True), (513, 9, False)])
def test_compact_zeroed(hip_lib, n_vis, x_ch, partials):
    """mtgs_project_bwd_zeroed: the streaming form's numbers (-0.0 against +0.0 allowed), places without a gradient exactly as the caller
    zeroed them, vis_ws untouched."""
    sc, dv = R.scene(BIG), dev(BIG)
    N = sc.N
    ids, rows, zero, d, _ = R.compact_case(n_vis)
    radii, index, vis_ids = compact_device(n_vis, ids)
    t = {k: up(v) for k, v in rows.items()}
    kw = dict(row_index=index, vis_ids=vis_ids, n_vis=n_vis, x_quat=t["x_quat"], x_mean=t["x_mean"], x_abs=t["x_abs"], x_col=t["x_col"],
              x_ch=x_ch, x_strides=[2, 12], by=("m2d", "abs", "col"))
    ws0 = fcan(n_vis * 12)
    stream = run_bwd(1, N, dv, radii, t, ws=ws0, **kw)
    ws = fcan(n_vis * 12)
    pt = fcan(12 * hip_blocks(n_vis)) if partials else None
    o = run_bwd(1, N, dv, radii, t, ws=ws, entry="mtgs_project_bwd_zeroed", zeroed=True, partials=pt, **kw)
    assert is_canary(ws), "vis_ws was written"
    ref = R.compact_reference(rows, ids, d)
    check(f"zeroed n_vis={n_vis}", o, ref, 1, N)
    sizes = dict(means=N * 3, quats=N * 4, scales=N * 3, opacities=N, d_m2d=N * 2, d_abs=N * 2, d_col=N * x_ch)
    for key, n in sizes.items():
        assert is_canary(o[key][n:]), key
        assert torch.equal(o[key][:n], stream[key][:n]), f"zeroed n_vis={n_vis}: {key} differs from the streaming form"      # (-0.0 == +0.0)
    gone = np.ones(N, bool)
    gone[ids[~zero]] = False
    at = torch.from_numpy(np.flatnonzero(gone)).cuda()
    for key, w in WIDTH.items():
        assert not bits(o[key][:N * w].view(N, w)[at]).any(), f"{key}: a place without a gradient was written"
    # refusals: before any launch
    assert run_bwd(2, N, dv, radii, t, ws=ws, entry="mtgs_project_bwd_zeroed", zeroed=True, rc=True, **kw) == EINVAL
    assert is_canary(ws)


def test_compact_zeroed_refuses_misaligned_quats(hip_lib):
    sc, dv = R.scene(BIG), dev(BIG)
    N, n_vis = sc.N, 257
    ids, rows, _, _, _ = R.compact_case(n_vis)
    radii, index, vis_ids = compact_device(n_vis, ids)
    t = {k: up(v) for k, v in rows.items()}
    outs = [fzero(N * 3), fzero(N * 4 + 1), fzero(N * 3), fzero(N), fcan(16), fcan(n_vis * 12)]
    keep = [x.clone() for x in outs]
    args = (1, N, ptr(dv["means"]), ptr(dv["quats"]), ptr(dv["scales"]), ptr(dv["vm"]), ptr(dv["K"]), R.W, R.H, R.EPS2D, ptr(radii),
            ptr(dv["conics"]), ptr(dv["comp"]), ptr(dv["opac"]), ptr(t["v_means2d"]), ptr(t["v_depths"]), ptr(t["v_conics"]),
            ptr(t["v_comp"]), ptr(t["v_opac_eff"]), ptr(outs[0]), outs[1].data_ptr() + 4, ptr(outs[2]), ptr(outs[4]), ptr(outs[3]),
            None, ptr(index), None, None, 0, None, None, None, None, ptr(vis_ids), n_vis, ptr(outs[5]), None, None, None, None, None, None, _st())
    assert rc_of("mtgs_project_bwd_zeroed", *args) == EINVAL
    torch.cuda.synchronize()
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(outs, keep)), "refused before any launch"


def test_compact_grid_stride(hip_lib):
    """8192 blocks x 256 + 300 rows: one row beyond the largest n_vis for which mtgs_project_bwd_blocks still grows would do; here blocks
    0 and 1 take a second round and the last one is partly filled.  A gradient in 200 rows of the first round, 150 of block 0's second
    round and all 44 of the last partial block; every other row is zero.  With vm_partials: 8192 x 12 sums in viewmat_from_partials."""
    full = 8192 * 256
    assert hip_blocks(full) == 8192 == hip_blocks(full + 300) and hip_blocks(full - 256) == 8191
    n_vis = N = full + 300
    r = np.random.RandomState(4)
    idx = np.concatenate([np.sort(r.choice(full, 200, replace=False)), full + np.sort(r.choice(256, 150, replace=False)),
                          np.arange(full + 256, N)])
    k = idx.size
    dv, at, rows, ref = _placed(N, idx)
    radii = torch.ones(N, dtype=torch.int32, device="cuda")
    vis_ids = torch.arange(N, dtype=torch.int32, device="cuda")
    g = {}
    for key, v in rows.items():
        t = torch.zeros((N,) + v.shape[1:], device="cuda")
        t[at] = up(v)
        g[key] = t
    ws, partials = fcan(N * 12), fcan(12 * 8192)
    o = run_bwd(1, N, dv, radii, g, row_index=vis_ids, vis_ids=vis_ids, n_vis=n_vis, ws=ws, partials=partials)
    check_placed("grid stride", o, ref, N, at, k)
    assert is_canary(ws[N * 12:]) and is_canary(partials[12 * 8192:])
    rest = bits(ws[:N * 12].view(N, 12)).clone()
    rest[at] = 0
    assert not bool(rest.any()), "workspace rows of zero gradient rows"


# ---- wire rows --------------------------------------------------------------------------------------------------------------------------------
def run_wire(N_, dv, G_, stride_, D_, depth, colors_pre_, mode_, vis_ids, n_vis_, wire_, vm, raw, aa=True, rc=False, **over):
    """mtgs_project_bwd_rows; `over`: arguments replaced by name (the refusals)."""
    a = dict(N=N_, means=ptr(dv["means"]), W=R.W, H=R.H, G=ptr(G_), stride=stride_, D=D_, mode=mode_, colors_pre=ptr(colors_pre_),
             n_vis=n_vis_, wire=ptr(wire_))
    a.update(over)
    args = (a["N"], a["means"], ptr(dv["quats"]), ptr(dv["scales"]), ptr(dv["vm"]), ptr(dv["K"]), a["W"], a["H"], R.EPS2D, ptr(dv["conics"]),
            ptr(dv["comp"]) if aa else None, ptr(dv["opac"]), a["G"], a["stride"], a["D"], depth, a["colors_pre"], a["mode"], ptr(vis_ids),
            a["n_vis"], a["wire"], ptr(vm), raw, _st())
    if rc:
        return rc_of("mtgs_project_bwd_rows", *args)
    _call("mtgs_project_bwd_rows", *args)


@pytest.mark.parametrize("n_vis,D,depth,mode,raw", R.wire_cases())
def test_wire_rows(hip_lib, n_vis, D, depth, mode, raw):
    """Rows [v_xy 2 | |v_xy| 2 | v_conic 3 | v_opacity_eff | D colours | depth | spare columns] -> [v_mean 3 | v_quat 4 | v_scale 3 |
    v_opacity | v_rgb 3 | 0 | index bits].  The depth column sits inside the third float4 for D < 4 and behind it for D >= 4; the row is
    four floats wider than it needs to be and row 1 is non-zero in a spare column only: live, with a zero result."""
    dv, N = dev(BIG), R.scene(BIG).N
    ids, _, zero, d, _ = R.compact_case(n_vis)
    _, _, vis_ids = compact_device(n_vis, ids)
    G, r = R.wire_rows(n_vis, D, depth, bool(raw))
    stride = G.shape[1]
    rows, mags, conv, mag = R.row_gradients(G, ids, bool(raw), depth_col=8 + D if depth else None)
    ref = R.compact_reference(rows, ids, d, vcomp=False, xq=False, xm=False, mags=mags)
    # the colour clamp: x + 0.5 exactly 0 and exactly 1 pass, one ulp outside is blocked (float32 arithmetic, as torch.clamp's)
    colors_pre, passes = None, np.ones((n_vis, 3), bool)
    if mode == 1:
        pre = r.uniform(-1.0, 1.0, (N, D)).astype(F)
        edge = np.array([-0.5, 0.5, np.nextafter(F(-0.5), F(-1)), F(0.5) + F(2.0 ** -23)], F)
        for j in range(min(n_vis, 8)):
            pre[ids[j], :3] = edge[(j + np.arange(3)) % 4]
        x = pre[ids, :3] + F(0.5)
        assert x.dtype == F
        passes = R.clamp_pass(x)
        assert n_vis < 8 or (set(x[:8].reshape(-1).tolist()) >= {0.0, 1.0} and (x[:8] < 0).any() and (x[:8] > 1).any())
        colors_pre = up(pre)
    elif mode == 2:
        mask = r.randint(0, 256, n_vis).astype(np.uint8)
        passes = ((mask[:, None] >> np.arange(3)[None]) & 1).astype(bool)
        colors_pre = torch.cat([up(mask), torch.full((16,), 0xFF, dtype=torch.uint8, device="cuda")])
    buf = torch.cat([up(G).view(-1), can(SL).view(torch.float32)])
    wire, vm = fcan(n_vis * 16), fcan(16)
    run_wire(N, dv, buf, stride, D, depth, colors_pre, mode, vis_ids, n_vis, wire, vm, raw)
    where = f"wire rows n_vis={n_vis} D={D} depth={depth} mode={mode} raw={raw}"
    assert is_canary(wire[n_vis * 16:]) and is_canary(vm[16:]) and is_canary(buf[n_vis * stride:]), where
    got = host(wire[:n_vis * 16]).reshape(n_vis, 16)
    val, terms = R.ws_rows(ref, ids)
    for name, lo, hi in (("means", 0, 3), ("quats", 3, 7), ("scales", 7, 10), ("opacities", 10, 11)):
        w = R.worst_ratio(got[:, lo:hi], val[:, lo:hi], terms[:, lo:hi]) / BOUND[name]
        assert w <= 1.0, f"{where}: {name} {w:.2f} x the bound"
    check(where, dict(viewmat=vm), ref, 1, N, names=("viewmat",))
    # v_rgb: the row's first three colour cotangents where the clamp passes, bit for bit; the index bits in the last float
    live = (G != 0).any(axis=1)
    want = np.zeros((n_vis, 3), F)
    k3 = min(D, 3)
    want[:, :k3] = np.where(passes[:, :k3], G[:, 8:8 + k3], F(0))
    want[~live] = 0
    assert np.array_equal((got[:, 11:14] + F(0)).view(np.int32), (want + F(0)).view(np.int32)), where + ": v_rgb"
    assert not got[:, 14].view(np.int32).any() and np.array_equal(got[:, 15].view(np.int32), ids), where + ": index bits"
    assert not got[~live][:, :14].view(np.int32).any(), where + ": zero rows become zeros plus the index"
    if n_vis > 1:
        assert not got[1, :14].any(), "a row that is live through a spare column only"
    back = host(buf[:n_vis * stride]).reshape(n_vis, stride)
    if raw:
        assert np.array_equal(back[:, 7:].view(np.int32), G[:, 7:].view(np.int32)) and not back[~live].view(np.int32).any()
        w = R.worst_ratio(back[live][:, :7], conv[live][:, :7], mag[live][:, :7]) / R.device_bound(1.0)
        assert w <= 1.0, f"{where}: converted rows {w:.2f} x the bound"
    else:
        assert np.array_equal(back.view(np.int32), G.view(np.int32)), where + ": the rows are inputs"


def test_wire_rows_of_nothing_and_refusals(hip_lib):
    sc, dv = R.scene(BIG), dev(BIG)
    N, n_vis, D, stride = sc.N, 257, 3, 12
    ids, _, _, _, _ = R.compact_case(n_vis)
    _, _, vis_ids = compact_device(n_vis, ids)
    G = torch.zeros(n_vis * stride + 4, device="cuda")
    wire, vm = fcan(n_vis * 16), fcan(16)
    pre = torch.zeros(N * 3, device="cuda")
    base = (N, dv, G, stride, D, 1, None, 0, vis_ids, n_vis, wire, vm, 0)
    run_wire(*base, n_vis=0)                                      # n_vis == 0: the camera's gradient is zeroed, nothing else
    assert not bits(vm[:16]).any() and is_canary(vm[16:]) and is_canary(wire)
    vm = fcan(16)
    base = (N, dv, G, stride, D, 1, None, 0, vis_ids, n_vis, wire, vm, 0)
    bad = [dict(N=-1), dict(n_vis=N + 1), dict(n_vis=-1), dict(W=0), dict(H=0), dict(D=8, stride=20), dict(D=-1), dict(stride=8), dict(stride=14),
           dict(mode=3), dict(mode=-1), dict(mode=1), dict(mode=2), dict(mode=1, D=0, colors_pre=ptr(pre)),
           dict(means=None), dict(G=None), dict(wire=None), dict(G=G.data_ptr() + 4), dict(wire=wire.data_ptr() + 8)]
    for over in bad:
        assert run_wire(*base, rc=True, **over) == EINVAL, over
    torch.cuda.synchronize()
    # (v_viewmats is zeroed by the entry point before the pointers are looked at: only the rows must be untouched)
    assert is_canary(wire)
    assert run_wire(*base, rc=True, mode=1, colors_pre=ptr(pre)) == 0
