"""mtgs_amd.seed on the device: exact neighbour distances against scikit-learn's (the fixture) and against an fp64 brute force
at size, and the fused seeding kernel against the reference's populate_modules arithmetic (tests/golden/make_seed_golden.py).

Bounds.  A distance is sqrt of a three-term sum of squares of rounded differences, all in fp32: at most about 4 units of 2^-24
relative; the references are correctly rounded fp64 values and a mis-ranked near-tie moves the k-th distance by no more than
that, so rtol = 1e-6 (atol = 0) leaves a factor of four.  exp(scales) adds the three-term mean and one logarithm: 2e-6."""
import time
from pathlib import Path

import numpy as np
import pytest
import torch

from mtgs_amd import seed
from tests.util import REPORT

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
RTOL = 1e-6


@pytest.fixture(scope="module")
def ref():
    return np.load(GOLD / "seed_ref.npz")


def cloud_of(ref, name):
    key = f"{name}_xyz"
    return ref[key] if key in ref.files else ref[str(ref[f"{name}_xyz_from"]) + "_xyz"]


def assert_distances(got, want, name):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, name
    assert np.array_equal(got == 0, want == 0), f"{name}: the exact zeros differ"
    nz = want != 0
    err = float((np.abs(got - want)[nz] / want[nz]).max()) if nz.any() else 0.0
    print(f"{name}: max relative distance error {err:.3e} over {int(nz.sum())} entries, {int((~nz).sum())} exact zeros")
    REPORT.append({"kind": "knn", "case": name, "max_rel_err": err, "zeros": int((~nz).sum())})
    assert np.allclose(got, want, rtol=RTOL, atol=0), f"{name}: max relative error {err:.3e} > {RTOL:.0e}"
    assert (np.diff(got, axis=1) >= 0).all(), f"{name}: rows are not ascending"
    return err


def street_cloud(n, seed_, dev):
    """a thin dense ground strip, two facades and a sparse cluster hundreds of metres away"""
    g = torch.Generator(device=dev).manual_seed(seed_)
    u = lambda m, lo, hi: torch.rand(m, device=dev, generator=g) * (hi - lo) + lo
    nrm = lambda m, s: torch.randn(m, device=dev, generator=g) * s
    n_far = max(n // 40, 8)
    n_fac = n // 3
    n_gr = n - n_far - n_fac
    ground = torch.stack([u(n_gr, 0, 400), u(n_gr, -6, 6), nrm(n_gr, 0.02)], -1)
    side = torch.where(torch.rand(n_fac, device=dev, generator=g) < 0.5, -9.0, 9.0)
    facade = torch.stack([u(n_fac, 0, 400), side + nrm(n_fac, 0.05), u(n_fac, 0, 20)], -1)
    far = torch.tensor([900.0, 400.0, 30.0], device=dev) + torch.randn(n_far, 3, device=dev, generator=g) * 40.0
    x = torch.cat([ground, facade, far])
    return x[torch.randperm(n, device=dev, generator=g)].contiguous()


def sample_brute_force(x, k, n_queries, seed_):
    """fp64 distances from a seeded sample of queries to every other point, the k smallest per query (on the device)"""
    g = torch.Generator(device=x.device).manual_seed(seed_)
    q = torch.randperm(x.shape[0], device=x.device, generator=g)[:n_queries]
    xd = x.double()
    out = []
    for s in range(0, n_queries, 100):
        qi = q[s:s + 100]
        d2 = torch.zeros(qi.numel(), x.shape[0], dtype=torch.float64, device=x.device)
        for a in range(3):
            d2 += (xd[qi, a][:, None] - xd[None, :, a]) ** 2
        d2[torch.arange(qi.numel(), device=x.device), qi] = float("inf")
        out.append(torch.topk(d2, k, dim=1, largest=False).values.sqrt())
    return q, torch.cat(out)


def test_distances_match_the_fixture(ref):
    dev = torch.device("cuda")
    for name in ref["knn_cases"]:
        x, k = cloud_of(ref, name), int(ref[f"{name}_k"])
        d = seed.knn_distances(torch.from_numpy(x).to(dev), k)
        assert d.dtype == torch.float32
        assert_distances(d.cpu().numpy(), ref[f"{name}_dist"], str(name))


def test_indices(ref):
    dev = torch.device("cuda")
    for name in ("street", "duplicates", "outliers", "sky_k8", "n4", "line"):
        x, k = cloud_of(ref, name), int(ref[f"{name}_k"])
        d, idx = seed.knn_distances(torch.from_numpy(x).to(dev), k, return_indices=True)
        d, idx = d.cpu().numpy(), idx.cpu().numpy()
        N = x.shape[0]
        assert idx.dtype == np.int64 and idx.shape == (N, k)
        assert (idx >= 0).all() and (idx < N).all(), name
        assert (idx != np.arange(N)[:, None]).all(), f"{name}: a point is its own neighbour"
        assert all(len(set(row)) == k for row in idx), f"{name}: a neighbour is listed twice"
        back = np.sqrt(((x[:, None, :].astype(np.float64) - x[idx].astype(np.float64)) ** 2).sum(-1))
        assert np.array_equal(back == 0, d == 0) and np.allclose(d, back, rtol=RTOL, atol=0), name
    # ties: equal distances are listed by increasing index, and among the candidates at the k-th distance the smallest indices win
    x = ref["duplicates_xyz"]
    d, idx = seed.knn_distances(torch.from_numpy(x).to(dev), 3, return_indices=True)
    d, idx = d.cpu().numpy(), idx.cpu().numpy()
    same = d[:, 1:] == d[:, :-1]
    assert same.any() and (idx[:, 1:][same] > idx[:, :-1][same]).all()
    full = np.sqrt(((x[:, None, :].astype(np.float64) - x[None, :, :].astype(np.float64)) ** 2).sum(-1))
    np.fill_diagonal(full, np.inf)
    rows = np.nonzero((d == 0).any(axis=1))[0]
    assert rows.size >= 60
    for i in rows:
        zeros = np.nonzero(full[i] == 0)[0]             # exact duplicates of point i, by increasing index
        n0 = int((d[i] == 0).sum())
        assert n0 == min(3, zeros.size) and np.array_equal(idx[i, :n0], zeros[:n0]), i


@pytest.mark.parametrize("kind,n", [("street", 2_000_000), ("sky", 200_000)])
def test_distances_at_size(kind, n):
    dev = torch.device("cuda")
    if kind == "street":
        x = street_cloud(n, 21, dev)
    else:
        x = seed.sky_points(n, 3000.0, 150.0, "spheric", generator=torch.Generator(device=dev).manual_seed(4), device=dev)["xyz"].contiguous()
    seed.knn_distances(x[:4096].contiguous(), 3)      # loads the code objects
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    d = seed.knn_distances(x, 3)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    q, want = sample_brute_force(x, 3, 2000, 77)
    err = assert_distances(d[q].cpu().numpy(), want.cpu().numpy(), f"{kind}_{n}")
    print(f"knn_distances {kind} N={n}: {wall * 1e3:.1f} ms wall")
    REPORT.append({"kind": "knn_time", "case": f"{kind}_{n}", "wall_ms": wall * 1e3, "max_rel_err": err})


def test_cluster_with_outliers_at_size():
    """200 000 points of which 1 000 are isolated far from a dense cluster: the outliers climb many levels before their block
    reaches three neighbours.  It has to finish and to be exact; no time is asserted."""
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(9)
    x = torch.cat([torch.randn(199_000, 3, device=dev, generator=g) * 0.5,
                   (torch.rand(1000, 3, device=dev, generator=g) - 0.5) * 2000.0])
    perm = torch.randperm(x.shape[0], device=dev, generator=g)
    x = x[perm].contiguous()
    d = seed.knn_distances(x, 3)
    q, want = sample_brute_force(x, 3, 2000, 78)
    assert_distances(d[q].cpu().numpy(), want.cpu().numpy(), "cluster_200000")
    out = torch.nonzero(perm >= 199_000).reshape(-1)             # every outlier as a query
    xd = x.double()
    d2 = ((xd[out][:, None, :] - xd[None, :, :]) ** 2).sum(-1)
    d2[torch.arange(out.numel(), device=dev), out] = float("inf")
    assert_distances(d[out].cpu().numpy(), torch.topk(d2, 3, dim=1, largest=False).values.sqrt().cpu().numpy(), "cluster_outliers")


def seed_points(ref, dev, normals=True):
    p = {"xyz": torch.from_numpy(ref["seed_xyz"]).to(dev), "rgb": torch.from_numpy(ref["seed_rgb"].astype(np.float32)).to(dev)}
    if normals:
        p["normals"] = torch.from_numpy(ref["seed_normals"]).to(dev)
    return p


def test_seed_gaussians_match_the_fixture(ref):
    dev = torch.device("cuda")
    out = seed.seed_gaussians(seed_points(ref, dev), 3)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    N = ref["seed_xyz"].shape[0]
    assert np.array_equal(got["means"], ref["seed_xyz"])
    # scales
    want = ref["seed_scales"]
    assert got["scales"].shape == (N, 3)
    assert np.array_equal(np.isneginf(got["scales"]), np.isneginf(want)) and np.isneginf(want).any()
    fin = np.isfinite(want)
    assert np.isfinite(got["scales"][fin]).all()
    e_got, e_want = np.exp(got["scales"].astype(np.float64)), np.exp(want.astype(np.float64))
    err = float((np.abs(e_got - e_want)[fin] / e_want[fin]).max())
    print(f"exp(scales): max relative error {err:.3e}")
    assert np.allclose(e_got[fin], e_want[fin], rtol=2e-6, atol=0), err
    plain = seed.seed_gaussians(seed_points(ref, dev, normals=False), 3, generator=torch.Generator(device=dev).manual_seed(1))
    assert torch.equal(plain["scales"], out["scales"][:, :1].expand(-1, 3))           # log(avg) three times without normals
    iso = seed.seed_gaussians(seed_points(ref, dev), 3, scale_dim=1)
    assert "quats" not in iso and torch.equal(iso["scales"], out["scales"][:, :1])
    qn = plain["quats"].norm(dim=1)
    assert plain["quats"].shape == (N, 4) and torch.allclose(qn, torch.ones_like(qn), atol=1e-5)   # random_quat_tensor: unit
    # colours and opacities
    dc_err = float(np.abs(got["features_dc"] - ref["seed_dc_sh"]).max())
    print(f"features_dc: max abs error {dc_err:.3e}")
    assert np.allclose(got["features_dc"], ref["seed_dc_sh"], rtol=1e-6, atol=1e-7)
    assert got["features_rest"].shape == (N, 15, 3) and not got["features_rest"].any()
    col = seed.seed_gaussians(seed_points(ref, dev), 0)
    assert np.allclose(col["features_dc"].cpu().numpy(), ref["seed_dc_logit"], rtol=1e-6, atol=1e-7)
    assert tuple(col["features_rest"].shape) == (N, 0, 3)
    assert np.array_equal(got["opacities"], ref["seed_opacities"]) and got["opacities"].shape == (N, 1)
    # quaternions
    q, q32, q64 = got["quats"], ref["seed_quats32"], ref["seed_quats64"]
    n_special = int(ref["seed_special_rows"])
    for r in range(n_special):
        nan = np.isnan(q32[r])
        # bit for bit; a NaN has no defined sign or payload (x86 produces 0xffc00000 for 0 / 0, the device 0x7fc00000): NaN where the fixture has NaN
        assert np.array_equal(np.isnan(q[r]), nan), r
        assert np.array_equal(q[r][~nan].view(np.uint32), q32[r][~nan].view(np.uint32)), (r, q[r], q32[r])
    assert np.isnan(q32[n_special - 1]).all()
    c = ref["seed_c64"]
    near_branch = ref["seed_branch_margin"] <= 1e-4
    antipode = (c > -1) & (c < -0.999)
    finite = np.isfinite(q64).all(axis=1)
    loose = finite & (near_branch | antipode)
    assert loose.sum() <= 0.01 * N, f"{int(loose.sum())} of {N} rows are near a branch or the antipode"
    tol = float(ref["seed_gap"]) + 1e-6
    strict = finite & ~loose
    err_q = np.abs(q.astype(np.float64) - q64).max(axis=1)
    print(f"quats: max abs error {err_q[strict].max():.3e} against fp64 over {int(strict.sum())} rows (gap {float(ref['seed_gap']):.2e}), "
          f"{int((finite & near_branch).sum())} near a branch, {int(antipode.sum())} near the antipode")
    assert (err_q[strict] <= tol).all(), float(err_q[strict].max())
    sign = finite & near_branch & ~antipode
    err_s = np.minimum(err_q, np.abs(q.astype(np.float64) + q64).max(axis=1))
    assert (err_s[sign] <= tol).all()


def hand_off_cloud(dev, n=3000):
    g = torch.Generator(device=dev).manual_seed(31)
    xyz = torch.rand(n, 3, device=dev, generator=g) * torch.tensor([6.0, 3.0, 4.0], device=dev) + torch.tensor([-3.0, -1.5, 4.0], device=dev)
    nrm = torch.randn(n, 3, device=dev, generator=g)
    return {"xyz": xyz, "rgb": torch.randint(0, 256, (n, 3), device=dev, generator=g).float(), "normals": nrm}


VARIANTS = {"vanilla": dict(), "multicolor": dict(num_traversals=3), "multicolor_rest": dict(num_traversals=3, multi_feature_rest=True),
            "fourier": dict(features_dc_dim=5), "isotropic": dict(scale_dim=1)}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_shapes_and_hand_off(variant, tmp_path):
    """The seeded dict goes unchanged into the consumers that take its node type: collect_gaussians + a rasterization forward and
    backward (every variant; the Fourier node as a posed rigid node), refine_gaussians with nothing to split or cull and a
    write_ply / read_ply round trip (every variant those two accept: they need scales [N, 3] with quats, and the PLY table holds
    features_dc [N, 3])."""
    from mtgs_amd import checkpoint as ck, rasterization
    from mtgs_amd.densify import RefineConfig, refine_gaussians
    from mtgs_amd.ply import read_ply, write_ply
    from mtgs_amd.synthetic import make_camera
    dev = torch.device("cuda")
    kw = VARIANTS[variant]
    pts = hand_off_cloud(dev)
    N, T, D = pts["xyz"].shape[0], kw.get("num_traversals"), kw.get("features_dc_dim")
    out = seed.seed_gaussians(pts, 3, generator=torch.Generator(device=dev).manual_seed(2), **kw)
    shapes = {"means": (N, 3), "scales": (N, kw.get("scale_dim", 3)), "quats": (N, 4), "features_dc": (N, 3) if D is None else (N, D, 3),
              "features_rest": (N, T, 15, 3) if kw.get("multi_feature_rest") else (N, 15, 3), "opacities": (N, 1)}
    if kw.get("scale_dim") == 1:
        del shapes["quats"]
    if T is not None:
        shapes["features_adapters"] = (N, T, 3)
    assert {k: tuple(v.shape) for k, v in out.items()} == shapes
    assert list(out) == [k for k in ck.GAUSS_PARAM_NAMES if k in out]
    assert all(v.dtype == torch.float32 and v.is_cuda and v.is_contiguous() for v in out.values())
    if D is not None:
        assert not out["features_dc"][:, 1:].any() and bool(out["features_dc"][:, 0].any())

    W, H = 96, 64
    vm, K = make_camera(W, H)
    c2w = torch.inverse(vm)[:, :3].contiguous()
    P = {k: v.clone().requires_grad_(True) for k, v in out.items()}
    node = dict(P)
    extra = {}
    if D is not None:
        node.update(instance_quats=torch.tensor([1.0, 0, 0, 0], device=dev), instance_trans=torch.zeros(3, device=dev))
        extra = dict(fourier={"x": 0.25, "scale": 1.0, "space": "temporal"})
    gs = ck.collect_gaussians({"node": node}, c2w, 3, traversal_index=1 if T is not None else None, **extra)
    render, alpha, _ = rasterization(gs["means"], gs["quats"], gs["scales"], gs["opacities"], gs["rgbs"], vm.to(dev), K.to(dev), W, H,
                                     packed=False, render_mode="RGB", rasterize_mode="antialiased")
    assert float(alpha.detach().sum()) > 0 and bool(torch.isfinite(render).all())
    (render.sum() + alpha.sum()).backward()
    for k in ("means", "scales", "opacities", "features_dc"):
        assert P[k].grad is not None and bool(torch.isfinite(P[k].grad).all()) and bool(P[k].grad.any()), k

    if kw.get("scale_dim", 3) == 3:
        cfg = RefineConfig(densify_grad_thresh=1e9, cull_alpha_thresh=0.0, cull_scale_thresh=1e9, cull_screen_size=1e9, split_screen_size=1e9)
        stats = (torch.zeros(N, device=dev), torch.ones(N, device=dev), torch.zeros(N, device=dev))
        new, _, info = refine_gaussians(out, stats, cfg, step=200, seed=5)
        assert info["n_after"] == N and all(torch.equal(new[k], out[k]) for k in out)
    if kw.get("scale_dim", 3) == 3 and D is None and not kw.get("multi_feature_rest"):
        path = tmp_path / "seeded.ply"
        assert write_ply(path, out) == N
        back = read_ply(path, device=dev)
        for k in ("means", "scales", "quats", "features_dc", "features_rest"):
            assert torch.equal(back[k].reshape(out[k].shape), out[k]), k
        assert torch.equal(back["opacities"].reshape(N, 1), out["opacities"])


def test_reproducible_and_strided():
    dev = torch.device("cuda")
    x = street_cloud(100_000, 3, dev)
    d0, i0 = seed.knn_distances(x, 3, return_indices=True)
    d1, i1 = seed.knn_distances(x, 3, return_indices=True)
    assert torch.equal(d0, d1) and torch.equal(i0, i1)
    wide = torch.cat([x, torch.full((x.shape[0], 1), float("nan"), device=dev)], dim=1)        # [N, 4]: the view skips the NaN column
    view = wide[:, :3]
    assert not view.is_contiguous()
    d2, i2 = seed.knn_distances(view, 3, return_indices=True)
    assert torch.equal(d0, d2) and torch.equal(i0, i2)
    pts = {"xyz": view, "rgb": torch.full((x.shape[0], 3), 128.0, device=dev)}
    a = seed.seed_gaussians(pts, 3, generator=torch.Generator(device=dev).manual_seed(3))
    b = seed.seed_gaussians({"xyz": x, "rgb": pts["rgb"]}, 3, generator=torch.Generator(device=dev).manual_seed(3))
    assert all(torch.equal(a[k], b[k]) for k in a) and a["means"].is_contiguous()


def test_non_finite_coordinates_and_small_clouds_are_refused():
    dev = torch.device("cuda")
    x = torch.rand(1000, 3, device=dev)
    for bad in (float("nan"), float("inf")):
        y = x.clone()
        y[17, 1] = bad
        with pytest.raises(ValueError, match="NaN or infinity"):
            seed.knn_distances(y)
    with pytest.raises(ValueError, match="n_neighbors"):
        seed.knn_distances(x[:3].contiguous(), 3)
    with pytest.raises(ValueError):
        seed.knn_distances(x, 9)
    assert tuple(seed.knn_distances(x[:4].contiguous(), 3).shape) == (4, 3)
    same = torch.ones(50, 3, device=dev) * 2.5                 # no extent at all: every distance is an exact zero
    assert not seed.knn_distances(same, 8).any()
