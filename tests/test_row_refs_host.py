"""tests/row_refs.py without a GPU: every reference against an independent float64 formulation (torch.autograd, finite
differences, torch.nn.Sequential, oracle/normals_oracle.py, tests/golden/normals_ref.npz), the conditioning of every case that
tests/test_gpu_row_colors.py parametrises (so that float32 and float64 must take the same decisions and no row is left out there),
and the measurements behind the constants C_WILD and C_DIR."""
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import normals_oracle as no
from oracle.torch_ref import sh_bases
from tests import row_refs as R

SH_IDS = [c[0] for c in R.SH_CASES]


def _scene(case, edge_rows=False):
    name, n_rows, _, _, degree, k_rest, use_sh, add, _, n_nodes = case
    return R.sh_scene(name, n_rows, degree, k_rest, use_sh, add, n_nodes, edge_rows=edge_rows)


def test_sh_poly_equals_the_oracle_bases_on_the_unit_sphere():
    d = torch.randn(200, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    u = d / d.norm(dim=-1, keepdim=True)
    for degree in range(4):
        nb = (degree + 1) ** 2
        assert float((R.sh_poly(u)[:, :nb] - sh_bases(degree, d)).abs().max()) < 1e-14


@pytest.mark.parametrize("case", R.SH_CASES, ids=SH_IDS)
def test_sh_case_reference_and_conditioning(case):
    """analytic coefficient gradient == autograd; direction gradient (autograd through normalize) == central differences; no clamp
    pre-activation within 1e-5 of an edge; the float32 direction gradient within a quarter of the dir_part bound."""
    sc = _scene(case)
    ref = R.sh_scene_ref(sc)
    n = sc["vis"].numel()
    assert R.sh_margins(sc, ref) >= 1e-5, R.sh_margins(sc, ref)
    assert float((ref["feat"] - ref["feat_autograd"]).abs().max()) <= 1e-13 if n else True
    # columns past the degree and past the node's k_rest are exact zeros in the reference too
    v = sc["vis"].long()
    kk = torch.arange(16)[None]
    off = (kk >= (sc["degree"] + 1) ** 2) | (kk - 1 >= sc["k_rest"][v][:, None]) | ((sc["use_sh"][v] == 0)[:, None] & (kk > 0))
    assert not bool(ref["feat"][off].any())
    if n == 0:
        return
    d0 = (sc["means"] - sc["cam"])[v].double()
    cot = torch.where(sc["cot"].abs() < R.FLUSH, torch.zeros_like(sc["cot"]), sc["cot"]).double()
    fd = torch.zeros(n, 3, dtype=torch.float64)
    h = 1e-5
    for c in range(3):
        e = torch.zeros(3, dtype=torch.float64)
        e[c] = h
        vals = []
        for sgn in (1, -1):
            r = R.sh_rows_ref(sc["degree"], d0 + sgn * e, sc["dc"][v], None if sc["add"] is None else sc["add"][v], sc["rest"][v],
                              sc["k_rest"][v], sc["use_sh"][v], None, sc["exact"][v])
            assert torch.equal(r["mask"], ref["mask"])
            vals.append((r["colour"] * cot).sum(-1))
        fd[:, c] = (vals[0] - vals[1]) / (2 * h)
    assert float((fd - ref["ddir"]).abs().max()) <= 1e-7 * max(1.0, float(ref["ddir"].abs().max()))
    # zero-cotangent rows: exact zeros
    zero = (cot == 0).all(-1)
    assert not bool(ref["feat"][zero].any()) and not bool(ref["ddir"][zero].any())
    # the measurement behind C_DIR: float32, the kernel's formula, rows added in order, per 64-row workgroup
    o32 = R.dir_rows_f32(ref)
    for w0 in range(0, n, 64):
        part32 = torch.zeros(3)
        for r_ in range(w0, min(w0 + 64, n)):
            part32 = part32 + o32[r_]
        want = ref["ddir"][w0:w0 + 64].sum(0)
        bound = R.C_DIR * R.U32 * ref["dterms"][w0:w0 + 64].sum(0)
        assert bool(((part32.double() - want).abs() <= bound / 4).all()), ((part32.double() - want).abs() / (R.U32 * ref["dterms"][w0:w0 + 64].sum(0))).max()


def test_sh_table_and_option_scenes_conditioning():
    """The scenes of the node-table and option tests of the GPU file: the same margins."""
    sc = R.sh_table_scene()
    assert R.sh_margins(sc, R.sh_scene_ref(sc)) >= 1e-5
    assert len(sc["nodes"]) == 129 and len(sc["nodes128"]) == 128
    starts = [s for s, n, _, _ in sc["nodes"] if n]
    assert len(set(sc["vis"].tolist()) & set(starts)) >= 20
    assert len({(k, u) for _, n, k, u in sc["nodes"] if n}) == 5
    for sc in [R.sh_opts_scene(u) for u in R.OPT_USE_SH] + [R.sh_twin_scene(u, K) for u, K in R.TWIN_CASES]:
        assert R.sh_margins(sc, R.sh_scene_ref(sc)) >= 1e-5


def test_sh_edge_rows_decide_in_float32():
    """The deliberate clamp-edge rows: pre-activations exactly 0 and 1 and their float32 neighbours, from the dc term alone."""
    for use_sh in (1, 4):
        sc = R.sh_edge_scene(use_sh)
        ref = R.sh_scene_ref(sc)
        assert R.sh_margins(sc, ref) >= 1e-5
        p = ref["pre32"][:6, 0]
        assert float(p[0]) == 0.0 and float(p[3]) == 1.0 and float(p[1]) > 0 and float(p[2]) < 0 and float(p[5]) <= 1
        # (the float32 neighbours of the dc of 1.0 may still round to 1.0: the sum is coarser than the product there)
        # every bit from the float32 pre-activations of the builder, by the inclusive rule written out here
        x32 = (sc["dc"][sc["vis"][:6].long()].numpy() * np.float32(0.2820947917738781)).astype(np.float32) + np.float32(0.5)
        assert np.array_equal(x32[:, 0], p.numpy())
        want = (x32 >= 0) & (x32 <= 1) if use_sh == 1 else (x32 >= 0)
        got = np.stack([(ref["mask"][:6].numpy() >> c) & 1 for c in range(3)], 1).astype(bool)
        assert np.array_equal(got, want)
        assert want[:, 0].tolist() == [True, True, False, True, True, True] and float(ref["pre32"][0, 2]) > 1
        assert bool(want[0, 2]) == (use_sh == 4)


@pytest.mark.parametrize("with_emb", [True, False])
def test_wild_reference_against_sequential_and_autograd(with_emb):
    ts, cot, kinks = R.wild_case(with_emb)
    n = 600
    sub = [None if t is None else (t[:n] if i < 2 else t) for i, t in enumerate(ts)]
    dc, rest, emb, w1, b1, w2, b2, w3, b3 = sub
    mlp = torch.nn.Sequential(torch.nn.Linear(59, 128), torch.nn.ReLU(), torch.nn.Linear(128, 128), torch.nn.ReLU(), torch.nn.Linear(128, 6)).double()
    with torch.no_grad():
        for lin, w, b in ((mlp[0], w1, b1), (mlp[2], w2, b2), (mlp[4], w3, b3)):
            lin.weight.copy_(w.double())
            lin.bias.copy_(b.double())
    pre32 = dc * torch.tensor(R.C0, dtype=torch.float32) + 0.5
    inside = (pre32 >= 0) & (pre32 <= 1)
    rgb = torch.where(inside, dc.double() * R.C0 + 0.5, pre32.clamp(0, 1).double())
    e = torch.zeros(32, dtype=torch.float64) if emb is None else emb.double()
    y = 0.01 * mlp(torch.cat([rgb, rest.double().reshape(n, 45)[:, :24], e.expand(n, 32)], 1))
    want = rgb * (1 + y[:, 3:]) + y[:, :3]
    assert float((R.wild_reference(sub) - want).abs().max()) < 1e-12
    # the plain-formula backward against autograd through wild_reference
    leaves = [None if t is None else t.clone().requires_grad_(True) for t in sub]
    (R.wild_reference(leaves) * cot[:n].double()).sum().backward()
    grads, _ = R.wild_backward_ref(sub, cot[:n])
    for name, t in zip(R.WILD_NAMES, leaves):
        if t is not None:
            scale = max(1.0, float(t.grad.abs().max()))
            # (the leaves are float32, so autograd rounds their gradients to float32)
            assert float((grads[name].reshape(t.shape) - t.grad).abs().max()) <= 2e-7 * scale, name


@pytest.mark.parametrize("with_emb", [True, False])
def test_wild_case_conditioning_and_float32_measurement(with_emb):
    """No row with a cotangent has a hidden pre-activation within 1e-5 of zero; the edge dc rows are where the builder says; the
    whole backward in float32 stays within a quarter of the C_WILD bound for every weight-gradient case."""
    ts, cot, kinks = R.wild_case(with_emb)
    again = []
    with torch.no_grad():
        R.wild_reference(ts, again)
    assert torch.equal(again[0], kinks) and not bool(cot[kinks].any())
    assert 0 < int(kinks.sum()) < R.WILD_N // 20
    assert torch.equal(ts[0].reshape(-1)[:6], R.edge_dc())
    for rows in R.WILD_GRAD_ROWS:
        v = R.wild_vis_ids(rows).long()
        sub = [None if t is None else (t[v] if i < 2 else t) for i, t in enumerate(ts)]
        g64, terms = R.wild_backward_ref(sub, cot[v])
        g32, _ = R.wild_backward_ref(sub, cot[v], dtype=torch.float32)
        for name in ("w1", "b1", "w2", "b2", "w3", "b3", "embedding"):
            err = (g32[name].double() - g64[name]).abs()
            bound = R.C_WILD * R.U32 * terms[name]
            assert bool((err <= bound / 4).all()), (rows, name, float((err / (R.U32 * terms[name]).clamp_min(1e-300)).max()))


def test_normals_plain_against_oracle_and_golden():
    sc = R.normals_scene(257)
    want = no.normals_fwd(sc["quats"].numpy(), sc["scales"].numpy(), sc["means"].numpy(), sc["c2w"].numpy())
    assert np.abs(R.normals_plain(sc["quats"], sc["scales"], sc["means"], sc["c2w"]) - want).max() < 1e-13
    gold = np.load(Path(__file__).parent / "golden" / "normals_ref.npz")
    for case in "abc":
        g = {k[2:]: torch.from_numpy(gold[k]).float() for k in gold.files if k.startswith(case + "_")}
        got = R.normals_plain(g["quats"], g["scales"], g["means"], g["c2w"].reshape(3, 4))
        assert np.abs(got - g["normals"].numpy()).max() < 2e-6
    # the special rows: the oracle and the plain restatement agree (NaN dot: no flip), everything finite
    sp, k = R.normals_special()
    plain = R.normals_plain(sp["quats"], sp["scales"], sp["means"], sp["c2w"])
    orc = no.normals_fwd(sp["quats"].numpy(), sp["scales"].numpy(), sp["means"].numpy(), sp["c2w"].numpy())
    assert np.isfinite(plain).all() and np.abs(plain - orc).max() < 1e-14
    assert np.argmin(sp["scales"].numpy(), -1).tolist() == k
    assert np.isnan(R.normals_dots(sp["quats"], sp["scales"], sp["means"], sp["c2w"])[3])
    assert not plain[5].any() and abs(np.linalg.norm(plain[4]) - 1) < 1e-14
    # the analytic backward of the oracle against autograd on the smooth rows
    q = sc["quats"].double().requires_grad_(True)
    kmin = sc["scales"].argmin(-1)
    w, x, y, z = q.unbind(-1)
    cols = torch.stack([torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y + w * z), 2 * (x * z - w * y)], -1),
                        torch.stack([2 * (x * y - w * z), 1 - 2 * (x * x + z * z), 2 * (y * z + w * x)], -1),
                        torch.stack([2 * (x * z + w * y), 2 * (y * z - w * x), 1 - 2 * (x * x + y * y)], -1)], 1)
    col = cols[torch.arange(sc["N"]), kmin]
    n0 = col / col.norm(dim=-1, keepdim=True)
    d = sc["c2w"].double()[:, 3][None] - sc["means"].double()
    sign = torch.where((n0.detach() * d / d.norm(dim=-1, keepdim=True)).sum(-1) < 0, -1.0, 1.0)[:, None]
    V = torch.randn(sc["N"], 3, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    (((sign * n0) @ sc["c2w"].double()[:, :3]) * V).sum().backward()
    ref_g = no.normals_bwd(sc["quats"].numpy(), sc["scales"].numpy(), sc["means"].numpy(), sc["c2w"].numpy(), V.numpy())
    assert np.abs(q.grad.numpy() - ref_g).max() < 1e-12 * max(1.0, np.abs(ref_g).max())


@pytest.mark.parametrize("rows", R.NORMAL_ROWS)
def test_normals_case_conditioning(rows):
    """No flip with |dot| < 1e-3 and no scale pair closer than 1e-6 relative, for every Gaussian of the case (cap: zero rows out)."""
    sc = R.normals_scene(rows)
    dots = R.normals_dots(sc["quats"], sc["scales"], sc["means"], sc["c2w"])
    assert np.abs(dots).min() >= 1e-3
    assert float(R.scale_gaps(sc["scales"]).min()) >= 1e-6
    assert sc["vis"].numel() == rows and bool((sc["vis"][1:] > sc["vis"][:-1]).all()) if rows > 1 else True


def test_normals_special_rows_conditioning():
    sp, _ = R.normals_special()
    dots = R.normals_dots(sp["quats"], sp["scales"], sp["means"], sp["c2w"])
    ok = np.isnan(dots) | (np.abs(dots) >= 1e-3) | (np.arange(8) == 5)      # (row 5: a zero normal, its dot is exactly 0 in both precisions)
    assert ok.all(), dots
    assert dots[5] == 0.0
    assert float(R.scale_gaps(sp["scales"]).min()) >= 1e-6


def test_plumbing_helpers():
    assert int(R.totals_word(5)) >> 32 == 5 and int(R.totals_word(0)) >> 32 == 0
    p = R.poisoned((3, 16))
    assert bool(R.is_poison(p).all()) and bool(torch.isnan(p).all())
    v = R.sorted_subset(50, 20, 3, must=(0, 49, 7))
    assert v.dtype == torch.int32 and {0, 7, 49} <= set(v.tolist()) and bool((v[1:] > v[:-1]).all())
    ids = R.padded_ids(v, 50, 40)
    assert ids.numel() == 40 and int(ids.min()) >= 0 and int(ids.max()) < 50 and not (set(ids[20:].tolist()) & set(v.tolist()))
    for n_nodes in (1, 2, 128, 129):
        nodes = R.split_nodes(R.SH_N, n_nodes, 4)
        assert len(nodes) == n_nodes and sum(n for _, n in nodes) == R.SH_N
        assert all(nodes[i + 1][0] == nodes[i][0] + nodes[i][1] for i in range(n_nodes - 1))
        if n_nodes > 2:
            assert nodes[0][1] == 0 and nodes[-1][1] == 0 and nodes[n_nodes // 2][1] == 0 and sum(n == 0 for _, n in nodes) >= 8
