"""WildGaussians appearance colours on the GPU (mtgs_amd/appearance.py, csrc/wild.hip).

(a) wild_colors against a float64 evaluation of the formula, written here from config/WildGaussians.py's description:
        rgb = clamp(features_dc * C0 + 0.5, 0, 1);  x = [rgb | features_rest.view(N, -1)[:, :24] | e]
        y = 0.01 * L3(relu(L2(relu(L1(x)))));       colour = rgb * (1 + y[:, 3:6]) + y[:, :3]
(b) wild_color_source through rasterization() against wild_colors + rasterization(): bit-identical render and alpha (every row's
    colour is computed by the same code), gradients within (a)'s bound, and only the visible-row form of the kernels ran.
(c) touch_first on and off, (d) bitwise-reproducible weight gradients, (e) one graph_mode capture + replay equals the eager step."""
import pytest
import torch

from tests.row_refs import edge_dc as _edge_dc, wild_params as _params, wild_reference as _reference  # noqa: F401  (moved there)

pytestmark = pytest.mark.gpu

C0 = 0.28209479177387814
NAMES = ("features_dc", "features_rest", "embedding", "w1", "b1", "w2", "b2", "w3", "b3")


def _grads(ts):
    return [None if t is None or t.grad is None else t.grad.detach().clone() for t in ts]


def _close(a, b, bound=1e-4):
    return float((a.double() - b.double()).abs().max()) <= bound * max(float(b.abs().max()), 1e-30)


@pytest.mark.parametrize("with_emb", [True, False])
@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 4097, 200_000])
def test_wild_colors_against_float64(hip_lib, N, with_emb):
    from mtgs_amd import wild_colors
    ts = _params(N, seed=N + 1, with_emb=with_emb)
    gcot = torch.randn(N, 3, generator=torch.Generator().manual_seed(7)).cuda()
    # rows at a ReLU kink get no cotangent: there fp32 and float64 may take different sides, and the row's gradient -- and every
    # weight gradient it is summed into -- would differ by a whole term although both are right to their precision
    kinks = []
    with torch.no_grad():
        _reference([None if t is None else t.detach() for t in ts], kinks)
    smooth = ~kinks[0]
    assert int((~smooth).sum()) <= max(2, N // 20), int((~smooth).sum())      # (about 1 % of the rows here: 256 units each)
    gcot[~smooth] = 0.0
    out = wild_colors(ts[0], ts[1], ts[2], ts[3:])
    assert out.shape == (N, 3) and out.dtype == torch.float32
    (out * gcot).sum().backward()
    got = _grads(ts)
    ref_ts = [None if t is None else t.detach().clone().requires_grad_(True) for t in ts]
    ref = _reference(ref_ts)
    (ref * gcot.double()).sum().backward()
    if N:
        assert float((out.double() - ref).abs().max()) <= 1e-5
    for name, t, g, r in zip(NAMES, ts, got, ref_ts):
        if t is None:
            continue
        assert g is not None and g.shape == t.shape, name
        if N == 0:
            assert not bool(g.any()), name
            continue
        rg = r.grad
        assert _close(g, rg), (name, float((g.double() - rg).abs().max()), float(rg.abs().max()))
    if N >= 6:      # the columns behind the first 24 floats of features_rest get zeros
        assert not bool(ts[1].grad.reshape(N, 45)[:, 24:].any())


def _scene(N, W, H, seed=5):
    from mtgs_amd.synthetic import make_camera, make_scene
    sc = make_scene(N, seed=seed, extent=(12.0, 4.0, 12.0))
    vm, K = make_camera(W, H)
    g = torch.Generator().manual_seed(seed)
    Gc, Ga = torch.randn(1, H, W, 7, generator=g).cuda(), torch.randn(1, H, W, 1, generator=g).cuda()
    return {k: v.cuda() for k, v in sc.items() if k != "colors"}, vm.cuda(), K.cuda(), Gc, Ga


def _render(form, geo, wild, vm, K, W, H, Gc, Ga, normals, touch_first=False):
    """One forward + backward.  form 'source': wild_color_source; 'dense': wild_colors + rasterization(colors=[N, 3 | 6])."""
    from mtgs_amd import rasterization, wild_color_source, wild_colors, wrapper
    from mtgs_amd.nodes import camera_space_normals
    P = {k: v.clone().requires_grad_(True) for k, v in geo.items()}
    T = [None if t is None else t.detach().clone().requires_grad_(True) for t in wild]
    c2w = torch.inverse(vm)[:, :3, :]
    calls, real = [], wrapper.call
    try:
        wrapper.call = lambda name, *a: (calls.append((name, a[1] if name in ("mtgs_wild_fwd", "mtgs_wild_bwd") else None)),
                                         real(name, *a))[1]
        if form == "source":
            src = wild_color_source(T[0], T[1], T[2], T[3:], camera_normals=c2w[0].contiguous() if normals else None,
                                    touch_first=touch_first)
            cols = None
        else:
            src = None
            cols = wild_colors(T[0], T[1], T[2], T[3:])
            if normals:
                cols = camera_space_normals(P["quats"], P["scales"], P["means"], c2w, cols)
        r, a, info = rasterization(P["means"], P["quats"], P["scales"], P["opacities"], cols, vm, K, W, H, packed=False,
                                   render_mode="RGB+ED", rasterize_mode="antialiased", absgrad=True, color_source=src)
        torch.autograd.backward([r, a], [Gc[..., :r.shape[-1]], Ga])
    finally:
        wrapper.call = real
    grads = {k: p.grad.clone() for k, p in P.items()}
    grads.update({n: t.grad.clone() for n, t in zip(NAMES, T) if t is not None})
    return r.detach(), a.detach(), grads, calls, info


@pytest.mark.parametrize("normals", [False, True])
def test_wild_color_source_equals_dense_colours(hip_lib, normals):
    N, W, H = 300_000, 960, 540
    geo, vm, K, Gc, Ga = _scene(N, W, H)
    wild = _params(N, seed=3)
    r1, a1, g1, c1, info = _render("source", geo, wild, vm, K, W, H, Gc, Ga, normals)
    r2, a2, g2, c2, _ = _render("dense", geo, wild, vm, K, W, H, Gc, Ga, normals)
    assert r1.shape[-1] == (7 if normals else 4)
    n_vis = int((info["radii"] > 0).sum())
    assert 0 < n_vis < N
    assert torch.equal(r1, r2) and torch.equal(a1, a2)
    for k in g2:
        assert _close(g1[k], g2[k]), (k, float((g1[k] - g2[k]).abs().max()), float(g2[k].abs().max()))
    # the source ran the visible-row form of the kernels only (vis_ids given), the dense form the all-N form
    wild_calls = [(n, v) for n, v in c1 if n.startswith("mtgs_wild_")]
    assert {n for n, _ in wild_calls} >= {"mtgs_wild_fwd", "mtgs_wild_bwd", "mtgs_wild_reduce"}
    assert all(v is not None for n, v in wild_calls if n in ("mtgs_wild_fwd", "mtgs_wild_bwd"))
    assert all(v is None for n, v in c2 if n in ("mtgs_wild_fwd", "mtgs_wild_bwd"))
    # the Gaussians outside the frame get no feature gradient from the source
    unseen = info["radii"][0] <= 0
    assert not bool(g1["features_dc"][unseen].any()) and not bool(g1["features_rest"][unseen].any())


def test_wild_color_source_touch_first(hip_lib):
    N, W, H = 300_000, 960, 540
    geo, vm, K, Gc, Ga = _scene(N, W, H, seed=8)
    wild = _params(N, seed=4)
    r0, a0, g0, _, _ = _render("source", geo, wild, vm, K, W, H, Gc, Ga, True, touch_first=False)
    r1, a1, g1, _, _ = _render("source", geo, wild, vm, K, W, H, Gc, Ga, True, touch_first=True)
    assert torch.equal(r0, r1) and torch.equal(a0, a1)
    for k in g0:
        assert _close(g1[k], g0[k]), (k, float((g1[k] - g0[k]).abs().max()))


def test_wild_weight_gradients_are_bitwise_reproducible(hip_lib):
    from mtgs_amd import wild_colors
    N = 200_000
    ts = _params(N, seed=11)
    gcot = torch.randn(N, 3, generator=torch.Generator().manual_seed(3)).cuda()
    runs = []
    for _ in range(2):
        for t in ts:
            t.grad = None
        (wild_colors(ts[0], ts[1], ts[2], ts[3:]) * gcot).sum().backward()
        runs.append(_grads(ts))
    for name, a, b in zip(NAMES, *runs):
        assert torch.equal(a, b), name


def test_wild_color_source_graph_mode_replay_equals_eager(hip_lib):
    import mtgs_amd
    from mtgs_amd import rasterization, wild_color_source
    N, W, H = 60_000, 480, 270
    geo, vm, K, Gc, Ga = _scene(N, W, H, seed=9)
    P = {k: v.clone().requires_grad_(True) for k, v in geo.items()}
    T = [t for t in _params(N, seed=6)]
    c2w = torch.inverse(vm)[:, :3, :]
    leaves = list(P.values()) + T

    def run():
        src = wild_color_source(T[0], T[1], T[2], T[3:], camera_normals=c2w[0].contiguous())
        r, a, info = rasterization(P["means"], P["quats"], P["scales"], P["opacities"], None, vm, K, W, H, packed=False,
                                   render_mode="RGB+ED", rasterize_mode="antialiased", absgrad=True, color_source=src)
        torch.autograd.backward([r, a], [Gc, Ga])
        return r, a, info

    for t in leaves:
        t.grad = None
    r0, a0, info0 = run()
    torch.cuda.synchronize()
    ref = (r0.detach().clone(), a0.detach().clone(), [t.grad.clone() for t in leaves])
    n_vis, M = int((info0["radii"] > 0).sum()), info0["flatten_ids"].numel()
    # the eager step's autograd graph must be gone before the capture: an AccumulateGrad node kept alive from it would accumulate
    # on the default stream inside the capture
    del r0, a0, info0
    for t in leaves:
        t.grad = torch.zeros_like(t)
    grads = [t.grad for t in leaves]
    gm = mtgs_amd.graph_mode(n_vis + 500, M + 5000)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), gm:
        torch._foreach_zero_(grads)
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with gm, torch.cuda.graph(graph):
        torch._foreach_zero_(grads)
        r, a, info = run()
    graph.replay()
    torch.cuda.synchronize()
    assert int(info["n_visible"]) == n_vis and not bool(info["overflow"])
    assert torch.equal(r, ref[0]) and torch.equal(a, ref[1])
    for t, gr in zip(leaves, ref[2]):
        assert _close(t.grad, gr, 2e-4)
