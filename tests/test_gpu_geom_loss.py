"""Geometric loss terms on the GPU (mtgs_amd/loss.py: normals_from_depth, depth_normal_loss, scale_regularizers;
csrc/geomloss.hip).

(1) The target normals, the loss and its gradient against the reference's own functions (tests/golden/depth_normals_ref.npz:
    a plane, a step edge, zero / out-of-range depths, non-finite depths, an odd size, a mask, a 2x5 image);
(2) 960x540 and 1920x1080 against a float64 restatement written here;
(3) NaN normals where nothing was splatted: through output_head -> depth_normal_loss -> combine_losses the term is dropped and
    the render gradient equals the gradient without it; an empty selection gives NaN;
(4) the scale regularisers against float64 autograd, and the documented tie and ratio == max_ratio rules;
(5) bitwise reproducibility, and a torch.cuda.graph capture replayed with new K and depth values equals eager bitwise."""
from pathlib import Path

import numpy as np
import pytest
import torch

from tests.image_refs import normals_from_depth_ref as _normals_f64, scale_reg_rule_grad as _rule_grad, \
    scale_reg_values as _scale_reg_f64, scene_depth as _scene_depth

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "depth_normals_ref.npz"


def _golden():
    z = np.load(GOLDEN)
    return z, [str(c) for c in z["cases"]]


def test_normals_from_depth_matches_the_reference():
    from mtgs_amd.loss import normals_from_depth
    z, cases = _golden()
    for c in cases:
        depth, K = torch.from_numpy(z[f"{c}_depth"]).cuda(), torch.from_numpy(z[f"{c}_K"]).cuda()
        got = normals_from_depth(depth, K).cpu().double()
        want = torch.from_numpy(z[f"{c}_normals64"])
        assert got.shape == want.shape, c
        assert torch.equal(torch.isnan(got), torch.isnan(want)), c
        tol = float(z[f"{c}_gap"]) + 1e-5
        torch.testing.assert_close(got, want, rtol=0, atol=tol, equal_nan=True, msg=lambda m: f"{c}: {m}")
        # border pixels are exactly 0.5
        assert (got[0] == 0.5).all() and (got[-1] == 0.5).all() and (got[:, 0] == 0.5).all() and (got[:, -1] == 0.5).all(), c
    # f16 depth is converted first, as the reference's .float() does; [H, W] depth is accepted as well
    depth, K = torch.from_numpy(z["odd_depth"]).cuda(), torch.from_numpy(z["odd_K"]).cuda()
    half = depth.half()
    assert torch.equal(normals_from_depth(half, K), normals_from_depth(half.float(), K))
    assert torch.equal(normals_from_depth(depth[..., 0], K), normals_from_depth(depth, K))


def test_depth_normal_loss_and_gradient_match_the_reference():
    from mtgs_amd.loss import depth_normal_loss
    z, cases = _golden()
    for c in cases:
        depth, K = torch.from_numpy(z[f"{c}_depth"]).cuda(), torch.from_numpy(z[f"{c}_K"]).cuda()
        mask = torch.from_numpy(z[f"{c}_mask"]).cuda()
        pred = torch.from_numpy(z[f"{c}_pred"]).cuda().requires_grad_(True)
        loss = depth_normal_loss(pred, depth, K, mask)
        (g,) = torch.autograd.grad(loss, pred)
        want = float(z[f"{c}_loss32"])
        if np.isnan(want):
            assert torch.isnan(loss), c
        else:
            assert abs(float(loss) - want) <= 1e-5 * abs(want), (c, float(loss), want)
            assert abs(float(loss) - float(z[f"{c}_loss64"])) <= 1e-5 * abs(want) or c == "zeros_range", c
        g_ref = torch.from_numpy(z[f"{c}_grad32"])
        near = (torch.from_numpy(z[f"{c}_normals32"]) - torch.from_numpy(z[f"{c}_pred"])).abs() < 1e-6
        got = g.cpu()
        assert torch.isfinite(got).all(), c
        torch.testing.assert_close(got[~near], g_ref[~near], rtol=1e-5, atol=1e-10, msg=lambda m: f"{c}: {m}")


@pytest.mark.parametrize("W,H", [(960, 540), (1920, 1080)])
def test_depth_normal_loss_full_size_against_float64(W, H):
    from mtgs_amd.loss import depth_normal_loss, normals_from_depth
    from mtgs_amd.synthetic import make_camera
    _, K = make_camera(W, H)
    K = K[0].cuda()
    depth = _scene_depth(H, W, seed=W).cuda()
    g = torch.Generator().manual_seed(H)
    pred = torch.rand(H, W, 3, generator=g).cuda().requires_grad_(True)
    mask = torch.ones(H, W, 1, dtype=torch.bool, device="cuda")
    mask[: H // 8] = False
    n64 = _normals_f64(depth.cpu(), K.cpu()).cuda()
    got = normals_from_depth(depth, K)
    err = (got.double() - n64).abs().max().item()
    assert err < 2e-4, err
    loss = depth_normal_loss(pred, depth, K, mask)
    (grad,) = torch.autograd.grad(loss, pred)
    p64 = pred.detach().double().requires_grad_(True)
    m = ((depth > 0.1) & (depth < 50) & mask)[..., 0]
    ref = (n64 - p64).abs()[m].mean() + (p64[:, :-1] - p64[:, 1:]).abs().mean() + (p64[:-1] - p64[1:]).abs().mean()
    (g64,) = torch.autograd.grad(ref, p64)
    assert abs(float(loss) - float(ref)) <= 1e-5 * abs(float(ref)), (float(loss), float(ref))
    sure = (n64 - p64.detach()).abs() > 1e-3           # (the sign of |target - pred| is the same in f32 and f64 here)
    torch.testing.assert_close(grad.double()[sure], g64[sure], rtol=1e-5, atol=1e-12)


def test_nan_normals_are_dropped_through_combine_losses():
    from mtgs_amd.loss import combine_losses, depth_normal_loss, masked_l1, output_head
    H, W = 64, 96
    g = torch.Generator().manual_seed(5)
    render = torch.rand(1, H, W, 7, generator=g)
    render[0, 10:20, 30:50, 3:6] = 0.0                 # nothing splatted: the normal is 0 / 0
    render = render.cuda().requires_grad_(True)
    alpha = torch.rand(1, H, W, 1, generator=g).cuda()
    bg = torch.zeros(3, device="cuda")
    gt = torch.rand(H, W, 3, generator=g).cuda()
    depth = _scene_depth(H, W, seed=3).cuda()
    K = torch.tensor([[80.0, 0, 48.0], [0, 80.0, 32.0], [0, 0, 1]], device="cuda")
    mask = torch.ones(H, W, 1, dtype=torch.bool, device="cuda")

    rgb, _, _, normal = output_head(render, alpha, bg, None, depth=True, normal_channel=3)
    assert torch.isnan(normal[15, 40]).all()
    term = depth_normal_loss(normal, depth, K, mask)
    assert torch.isnan(term)
    loss = combine_losses([masked_l1(gt, rgb, mask), term], [0.8, 0.1], drop_if_not_finite=(1,))
    (with_term,) = torch.autograd.grad(loss, render)
    rgb, _, _, normal = output_head(render, alpha, bg, None, depth=True, normal_channel=3)
    loss_b = combine_losses([masked_l1(gt, rgb, mask)], [0.8])
    (without,) = torch.autograd.grad(loss_b, render)
    assert float(loss) == float(loss_b)
    assert torch.isfinite(with_term).all()
    assert torch.equal(with_term, without)
    # a zero cotangent writes exact zeros, also next to NaN pixels
    pred = normal.detach().requires_grad_(True)
    (gz,) = torch.autograd.grad(depth_normal_loss(pred, depth, K, mask), pred, grad_outputs=torch.zeros((), device="cuda"))
    assert torch.equal(gz, torch.zeros_like(gz))


def test_empty_selection_gives_nan():
    from mtgs_amd.loss import depth_normal_loss
    H, W = 32, 40
    pred = torch.rand(H, W, 3, device="cuda")
    depth = torch.full((H, W, 1), 10.0, device="cuda")
    K = torch.tensor([[40.0, 0, 20.0], [0, 40.0, 16.0], [0, 0, 1]], device="cuda")
    assert torch.isnan(depth_normal_loss(pred, depth, K, torch.zeros(H, W, 1, dtype=torch.bool, device="cuda")))
    assert torch.isnan(depth_normal_loss(pred, torch.full_like(depth, 60.0), K))       # everything beyond hi
    assert torch.isfinite(depth_normal_loss(pred, depth, K))
    # without the TV part the result is the L1 mean alone
    l1 = depth_normal_loss(pred, depth, K, tv=False)
    tv = (pred[:, :-1] - pred[:, 1:]).abs().mean() + (pred[:-1] - pred[1:]).abs().mean()
    assert abs(float(depth_normal_loss(pred, depth, K)) - float(l1 + tv)) <= 1e-6


@pytest.mark.parametrize("two_d", [True, False])
def test_scale_regularizers_against_float64_autograd(two_d):
    from mtgs_amd.loss import scale_regularizers
    g = torch.Generator().manual_seed(9)
    N = 200_003
    s = torch.exp(0.8 * torch.randn(N, 3, generator=g))
    s[::3, 0] *= 30.0                                   # a third of the rows above the ratio 10
    sc = s.cuda().requires_grad_(True)
    two, sharp = scale_regularizers(sc, two_d=two_d)
    (grad,) = torch.autograd.grad(0.7 * two + 1.3 * sharp, sc)
    s64 = s.double().requires_grad_(True)
    t64, h64 = _scale_reg_f64(s64, two_d, 10.0)
    (g64,) = torch.autograd.grad(0.7 * t64 + 1.3 * h64, s64)
    assert abs(float(two) - float(t64)) <= 1e-5 * abs(float(t64))
    assert abs(float(sharp) - float(h64)) <= 1e-5 * abs(float(h64))
    # (rows whose ratio is within rounding of max_ratio may take the other branch of maximum in f32: left out)
    srt = torch.sort(s.double(), dim=-1, descending=True)[0]
    ratio = srt[:, 0] / srt[:, 1] if two_d else srt[:, 0] / srt[:, 2]
    clear = (ratio - 10.0).abs() > 1e-4
    assert clear.float().mean() > 0.999
    torch.testing.assert_close(grad.cpu().double()[clear], g64[clear], rtol=2e-5, atol=1e-13)


def test_scale_regularizers_tie_rules():
    from mtgs_amd.loss import scale_regularizers
    rows = torch.tensor([[1.0, 1.0, 0.5], [0.5, 2.0, 2.0], [1.0, 1.0, 1.0], [2.0, 2.0, 0.1], [3.0, 0.2, 0.2],
                         [10.0, 1.0, 0.5], [5.0, 2.0, 0.5], [0.25, 2.5, 0.25], [4.0, 40.0, 4.0]])
    N = rows.shape[0]
    for two_d in (True, False):
        sc = rows.cuda().requires_grad_(True)
        two, sharp = scale_regularizers(sc, two_d=two_d)
        (grad,) = torch.autograd.grad(0.75 * two + 1.5 * sharp, sc)
        want = torch.tensor([_rule_grad(r, two_d, 10.0, N, 0.75, 1.5) for r in rows], dtype=torch.float64)
        torch.testing.assert_close(grad.cpu().double(), want, rtol=1e-6, atol=1e-9, msg=lambda m: f"two_d={two_d}: {m}")
        t64, h64 = _scale_reg_f64(rows.double(), two_d, 10.0)
        assert abs(float(two) - float(t64)) <= 1e-6 and abs(float(sharp) - float(h64)) <= 1e-6 * max(1.0, float(h64))
    # where PyTorch's own choice is defined (amax / amin split evenly, maximum's half at equality), it agrees too
    s64 = rows.double().requires_grad_(True)
    t64, h64 = _scale_reg_f64(s64, False, 10.0)
    (g64,) = torch.autograd.grad(1.5 * h64, s64)
    sc = rows.cuda().requires_grad_(True)
    (grad,) = torch.autograd.grad(1.5 * scale_regularizers(sc, two_d=False)[1], sc)
    torch.testing.assert_close(grad.cpu().double(), g64, rtol=1e-6, atol=1e-9)
    # rows with a NaN give NaN; no rows give NaN (mean of an empty tensor); a zero cotangent gives exact zeros
    bad = rows.clone()
    bad[2, 1] = float("nan")
    two, sharp = scale_regularizers(bad.cuda())
    assert torch.isnan(two) and torch.isnan(sharp)
    two, sharp = scale_regularizers(torch.empty(0, 3, device="cuda"))
    assert torch.isnan(two) and torch.isnan(sharp)
    sc = bad.cuda().requires_grad_(True)
    (gz,) = torch.autograd.grad(scale_regularizers(sc)[1], sc, grad_outputs=torch.zeros((), device="cuda"))
    assert torch.equal(gz, torch.zeros_like(gz))


def test_geom_losses_are_bitwise_reproducible():
    from mtgs_amd.loss import depth_normal_loss, scale_regularizers
    H, W = 540, 960
    depth = _scene_depth(H, W, seed=1).cuda()
    K = torch.tensor([[768.0, 0, 480.0], [0, 768.0, 270.0], [0, 0, 1]], device="cuda")
    pred = torch.rand(H, W, 3, device="cuda", requires_grad=True)
    s = torch.exp(torch.randn(1 << 21, 3, device="cuda")).requires_grad_(True)
    runs = []
    for _ in range(2):
        loss = depth_normal_loss(pred, depth, K)
        two, sharp = scale_regularizers(s)
        gp, gs = torch.autograd.grad(loss + two + sharp, (pred, s))
        runs.append((loss, two, sharp, gp, gs))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_geom_losses_capture_in_a_graph_without_host_reads():
    from mtgs_amd.loss import depth_normal_loss, normals_from_depth, scale_regularizers
    H, W = 135, 240
    K1 = torch.tensor([[190.0, 0, 120.0], [0, 190.0, 67.5], [0, 0, 1]], device="cuda")
    K2 = torch.tensor([[150.0, 0, 101.0], [0, 170.0, 80.0], [0, 0, 1]], device="cuda")
    d1, d2 = _scene_depth(H, W, seed=4).cuda(), (_scene_depth(H, W, seed=5) * 0.7).cuda()
    pred = torch.rand(H, W, 3, device="cuda")
    mask = torch.rand(H, W, 1, device="cuda") > 0.2
    scales = torch.exp(torch.randn(10_000, 3, device="cuda"))
    sK, sd = K1.clone(), d1.clone()
    sp = pred.clone().requires_grad_(True)
    ss = scales.clone().requires_grad_(True)

    def step(K, d, p, s):
        loss = depth_normal_loss(p, d, K, mask)
        two, sharp = scale_regularizers(s)
        gp, gs = torch.autograd.grad(loss + 0.5 * two + sharp, (p, s))
        return loss, two, sharp, gp, gs, normals_from_depth(d, K)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(sK, sd, sp, ss)                  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(sK, sd, sp, ss)
    for K, d in ((K2, d2), (K1, d1)):
        sK.copy_(K)
        sd.copy_(d)
        graph.replay()
        torch.cuda.synchronize()
        eager = step(K, d, sp, ss)
        for a, b in zip(out, eager):
            assert torch.equal(a, b)
    assert not torch.equal(out[5], normals_from_depth(d2, K2))     # the replays did follow K and depth
