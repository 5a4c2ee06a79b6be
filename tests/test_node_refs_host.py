"""tests/node_refs.py without a GPU: (1) each reference reproduces the golden vectors the reference's own code produced
(pose_fourier_ref.npz, deform_ref.npz) or a hand-written case; (2) the refinement oracle keeps its invariants for every
n_split_samples; (3) the inputs of tests/test_gpu_node_edges.py are conditioned so that a float32 device and a float64 oracle
must take the same decision for every row, and the measured constants that file's tolerances quote are what it quotes."""
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import node_refs as R
from tests import test_gpu_node_edges as E

GOLDEN = Path(__file__).resolve().parent / "golden"


# ---- (1) golden vectors and hand-written cases ------------------------------------------------------------------------------------
def test_fourier_ref_reproduces_the_reference_vectors():
    z = np.load(GOLDEN / "pose_fourier_ref.npz")
    for name in ("t5", "t8", "s6", "s1"):
        fdc, w, G = z[f"four_{name}_fdc"], z[f"four_{name}_w"].reshape(-1), z[f"four_{name}_G"]
        dc, v_f, v_w, abs_w = R.fourier_ref(fdc, w, G)
        assert np.abs(dc - z[f"four_{name}_dc"]).max() <= 1e-12, name
        assert np.abs(v_f - z[f"four_{name}_g_fdc"]).max() <= 1e-12, name
        assert np.abs(v_w - z[f"four_{name}_g_w"].reshape(-1)).max() <= 1e-11, name
        assert abs_w.shape == w.shape and (abs_w >= np.abs(v_w) - 1e-11).all()


def test_deform_embed_ref_layout_on_a_hand_written_case():
    """Two Gaussians, height 2 (so x = means), 2 / 1 frequencies, E = 2: width 3 + 12 + 1 + 2 + 2 = 20, values written out."""
    means = np.array([[0.0, 0.5, -1.0], [2.0, 0.25, 0.0]], dtype=np.float32)
    row = R.deform_embed_ref(means, 2.0, 0.5, [[7.0, -3.0]], 2, 1)
    assert R.deform_embed_width(2, 1, 2) == 20 and row.shape == (2, 20)
    s, c = np.sin, np.cos
    want0 = [0.0, 0.5, -1.0,                                   # x
             0.0, s(0.5), s(-1.0), 1.0, c(0.5), c(-1.0),       # frequency 0: sin(x), cos(x)
             0.0, s(1.0), s(-2.0), 1.0, c(1.0), c(-2.0),       # frequency 1: sin(2 x), cos(2 x)
             0.5, s(0.5), c(0.5),                              # t, sin(t), cos(t)
             7.0, -3.0]                                        # cond
    want1 = [2.0, 0.25, 0.0, s(2.0), s(0.25), 0.0, c(2.0), c(0.25), 1.0, s(4.0), s(0.5), 0.0, c(4.0), c(0.5), 1.0,
             0.5, s(0.5), c(0.5), 7.0, -3.0]
    assert np.abs(row - np.array([want0, want1])).max() <= 1e-15
    # t = 0 and E = 0, no position frequency: [x | t, sin(0), cos(0)]
    row = R.deform_embed_ref(means, 2.0, 0.0, np.zeros((1, 0)), 0, 1)
    assert np.array_equal(row, np.array([[0.0, 0.5, -1.0, 0.0, 0.0, 1.0], [2.0, 0.25, 0.0, 0.0, 0.0, 1.0]]))
    # nothing but x and t
    assert np.array_equal(R.deform_embed_ref(means[:1], 4.0, 1.0, [], 0, 0), np.array([[0.0, 0.25, -0.5, 1.0]]))


def _network64(emb, weights):
    """The layers of mtgs_amd.deform.deform_network behind the embedding, in float64."""
    W = {k: v.astype(np.float64) for k, v in weights.items()}
    h, i, in_ch = emb, 0, emb.shape[1]
    while f"linear.{i}.weight" in W:
        w, b = W[f"linear.{i}.weight"], W[f"linear.{i}.bias"]
        if i > 0 and w.shape[1] == h.shape[1] + in_ch:          # the layer behind the skip connection
            h = np.concatenate([emb, h], -1)
        h = np.maximum(h @ w.T + b, 0.0)
        i += 1
    return tuple(h @ W[f"{k}.weight"].T + W[f"{k}.bias"] for k in ("gaussian_warp", "gaussian_rotation", "gaussian_scaling"))


def test_deform_embed_ref_feeds_the_network_to_the_reference_vectors():
    g = np.load(GOLDEN / "deform_ref.npz")
    emb = R.deform_embed_ref(g["means"], float(g["height"]), float(g["t"]), g["cond"], 10, 10)
    assert emb.shape == (128, 100)
    assert np.abs(emb[:, :63] - g["x_emb"]).max() <= 1e-6 and np.abs(emb[:1, 63:84] - g["t_emb"]).max() <= 1e-6
    outs = _network64(emb, {k[2:]: g[k] for k in g.files if k.startswith("w.")})
    for got, key in zip(outs, ("d_xyz", "d_quat", "d_scale")):
        ref = g[key]
        assert got.shape == ref.shape and np.abs(got - ref).max() / max(1.0, np.abs(ref).max()) < 1e-4, key


def test_stats_ref_rows_equal_the_dense_form():
    """A frame where both are defined: every visible Gaussian has one row, the gradient sits in the row's columns 2-3."""
    g = torch.Generator().manual_seed(3)
    sizes, W, H = [0, 70, 1, 0, 300], 640, 360
    N = sum(sizes) + 20
    starts = (10 + np.cumsum([0] + sizes)[:-1]).tolist()
    radii = (torch.randint(1, 40, (1, N), generator=g) * (torch.rand(1, N, generator=g) < 0.4)).int()
    grad = torch.rand(1, N, 2, generator=g, dtype=torch.float64) * 1e-3
    mk = lambda: [[torch.rand(n, generator=torch.Generator().manual_seed(n), dtype=torch.float64) for _ in range(3)] for n in sizes]
    dense, rows = mk(), mk()
    for s, st in zip(dense, starts):
        mask = torch.zeros(N, dtype=torch.bool)
        mask[st:st + s[0].numel()] = True
        R.stats_ref(s, radii, grad, mask, W, H)
    vis = torch.nonzero(radii[0] > 0).flatten()
    vis = vis[torch.randperm(vis.numel(), generator=g)].int()
    table = torch.zeros(vis.numel(), 16, dtype=torch.float64)
    table[:, 2:4] = grad[0, vis.long()]
    table[:, 0:2] = -7.0
    R.stats_ref_rows(rows, starts, radii, table, vis, W, H, col=2)
    assert any(bool((a[1] != b[1]).any()) for a, b in zip(mk(), dense))
    for a, b in zip(dense, rows):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    # a count below the capacity, the other column pair
    half = mk()
    R.stats_ref_rows(half, starts, radii, table, vis, W, H, col=0, count=vis.numel() // 2)
    seen = torch.zeros(N, dtype=torch.bool)
    seen[vis[:vis.numel() // 2].long()] = True
    for s, s0, st in zip(half, mk(), starts):
        m = seen[st:st + s[0].numel()]
        assert torch.equal(s[1], s0[1] + m.double())
        assert torch.allclose(s[0], s0[0] + m.double() * 3.5 * float(np.hypot(W, H)), rtol=1e-14, atol=0)


# ---- (2) the refinement oracle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clone", [True, False])
@pytest.mark.parametrize("S", [1, 2, 3, 4])
def test_refinement_oracle_invariants(S, clone):
    case = E.REFINE_BY_NAME[f"mixed-S{S}-{'clone' if clone else 'copy'}"]
    (p, stats, moments), (new, new_m, masks) = E.refine_oracle(case)
    cnt = E.refine_counts(case)
    N, n_after = case["N"], new["means"].shape[0]
    kind, src = masks["kind"], masks["src_index"]
    assert n_after == cnt["kept_old"] + cnt["kept_children"] + cnt["kept_dups"] == kind.size == src.size
    assert kind.min() >= 0 and kind.max() <= 1 + S and set(np.unique(kind)) == set(range(2 + S))
    assert (np.diff(kind) >= 0).all()                                                   # [old | children, sample-major | duplicates]
    assert masks["splits"][src[(kind >= 1) & (kind <= S)]].all()                        # every child's parent is a split parent
    assert masks["dups"][src[kind == 1 + S]].all() and not masks["splits"][src[kind == 0]].any()
    assert min(cnt[k] for k in ("splits", "dups", "culled_parents", "culled_children", "culled_old")) > 20, cnt
    for k, (a, b) in new_m.items():
        assert a.shape == new[k].shape and not a[kind > 0].any() and not b[kind > 0].any(), k        # moments of new rows are zero
        assert np.array_equal(a[kind == 0], moments[k][0].numpy().astype(np.float64)[src[kind == 0]]), k
    for k in ("quats", "opacities", "features_dc", "features_rest"):                    # what is not geometry follows its parent
        assert np.array_equal(new[k], p[k].numpy().astype(np.float64)[src]), k
    old = kind == 0
    assert np.array_equal(new["means"][old], p["means"].numpy().astype(np.float64)[src[old]])
    if not clone:                                                                       # a plain copy of the mean
        assert np.array_equal(new["means"][kind == 1 + S], p["means"].numpy().astype(np.float64)[src[kind == 1 + S]])
    else:
        assert (new["means"][kind == 1 + S] != p["means"].numpy().astype(np.float64)[src[kind == 1 + S]]).any(axis=1).all()


# ---- (3) conditioning of the GPU cases and the measured constants -------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in E.REFINE_CASES])
def test_refinement_cases_are_conditioned(name):
    """No statistic within 1e-4 relative of the threshold it is compared with (a condition on the inputs: a seed that
    violates it is replaced)."""
    assert E.refine_margin(E.REFINE_BY_NAME[name]) > 1e-4


def test_refinement_regimes_are_what_their_names_say():
    for S in (2, 3):
        N = 300
        c = E.refine_counts(E.REFINE_BY_NAME[f"same-S{S}"])
        assert (c["splits"], c["dups"], c["kept_old"]) == (0, 0, N)
        c = E.refine_counts(E.REFINE_BY_NAME[f"split-S{S}"])
        assert (c["splits"], c["dups"], c["kept_old"]) == (N, 0, 0) and 0 < c["culled_children"] < S * N
        c = E.refine_counts(E.REFINE_BY_NAME[f"culled-S{S}"])
        assert c["kept_old"] + c["kept_children"] + c["kept_dups"] == 0 and c["splits"] > 20 and c["dups"] > 0
        c = E.refine_counts(E.REFINE_BY_NAME[f"dups-S{S}"])
        assert (c["splits"], c["dups"], c["kept_old"], c["kept_dups"]) == (0, N, N, N)
    want = E.refine_parents(E.REFINE_BY_NAME["mixed-S3-clone"])
    assert 20 < want.sum() < 1000


@pytest.mark.parametrize("name", E.OOB_CASES)
def test_oob_cases_are_conditioned(name):
    nodes, radii, starts = E.oob_inputs(name)
    assert E.oob_margin(nodes) > 1e-4
    val, grads = R.oob_ref(nodes, radii, starts, tolerance=E.OOB_TOL)
    assert (float(val) == 0.0) == (name == "inside")
    assert radii.shape[1] >= starts[-1] + nodes[-1][0].shape[0]


def test_the_measured_constants_are_the_quoted_ones():
    """C_SUM = 4 x the float32 sequential sum of the largest Fourier size (worst over the series lengths); SINCOS_TOL = 4 x float32 np.sin / np.cos over the
    argument grid of the embedding cases, capped at 1e-5."""
    ratios = {(N, F): E.fourier_seq_f32_ratio(N, F) for N in E.FOURIER_NS[1:] for F in E.FOURIER_FS}
    ratio = max(ratios[(max(E.FOURIER_NS), F)] for F in E.FOURIER_FS)
    assert 4 * ratio <= E.C_SUM <= 4 * ratio * 1.1, ratio
    assert max(ratios.values()) <= E.C_SUM / 4, ratios          # every case: the plain float32 sum leaves the device its margin
    err = E.sincos_f32_error()
    assert 4 * err <= E.SINCOS_TOL <= min(1e-5, 4 * err * 1.1), err
