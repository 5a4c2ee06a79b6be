"""Image metrics on the GPU (mtgs_amd/metrics.py, csrc/metrics.hip).

(1) color_correct against the reference's own float64 outputs (tests/golden/color_correct_ref.npz), within the reference's
    own f32-vs-f64 gap; (2) color_correct and image_metrics at 960x540 and 1920x1080 against a float64 formulation written
    here (numpy lstsq, gelsd); (3) degenerate inputs: the fallback, empty selections, zero errors, zero depths;
    (4) bitwise reproducibility; (5) a torch.cuda.graph capture + replay equals eager bitwise."""
from pathlib import Path

import numpy as np
import pytest
import torch

from tests.image_refs import color_correct_ref as _cc_f64, depth_metrics_ref as _depth_ref, psnr_ref as _psnr

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "color_correct_ref.npz"


def _structured(H, W, seed):
    """a smooth image with edges and saturated regions, and a target under a per-channel quadratic colour shift"""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    base = torch.stack([0.5 + 0.6 * torch.sin(6 * xx + 2 * yy), 0.5 + 0.5 * torch.cos(5 * yy - 3 * xx * yy),
                        xx * 0.8 + 0.25 * ((xx * 13).floor() % 2)], dim=-1)
    gt = (base + 0.05 * torch.randn(H, W, 3, generator=g)).clamp(0, 1)
    pred = (0.05 + 0.85 * gt + 0.15 * gt * gt - 0.1 * gt[..., [1, 2, 0]] * gt + 0.02 * torch.randn(H, W, 3, generator=g)).clamp(0, 1)
    mask = torch.ones(H, W, 1, dtype=torch.bool)
    mask[: H // 6] = False                                       # a sky band
    mask &= torch.rand(H, W, 1, generator=g) > 0.05
    lidar = torch.where(torch.rand(H, W, 1, generator=g) > 0.7, 1 + 90 * torch.rand(H, W, 1, generator=g), torch.zeros(H, W, 1))
    depth = lidar * (1 + 0.3 * torch.randn(H, W, 1, generator=g)) + 0.5
    return pred, gt, mask, depth, lidar


def test_color_correct_matches_reference_golden():
    from mtgs_amd import color_correct
    z = np.load(GOLDEN)
    names = sorted({k.split("_")[0] for k in z.files})
    assert len(names) >= 5
    for n in names:
        pred, gt = torch.from_numpy(z[f"{n}_pred"]).cuda(), torch.from_numpy(z[f"{n}_gt"]).cuda()
        mask = torch.from_numpy(z[f"{n}_mask"]).cuda() if z[f"{n}_mask"].size else None
        out = color_correct(pred, gt, mask, num_iters=int(z[f"{n}_iters"])).cpu().numpy()
        err = np.abs(out.astype(np.float64) - z[f"{n}_cc_f64"]).max()
        tol = max(2e-6, float(z[f"{n}_gap"]))
        assert err <= tol, f"case {n}: max |device - reference f64| = {err:.3g} > {tol:.3g}"
        assert not np.array_equal(out, pred.cpu().numpy() * (1 if mask is None else mask.cpu().numpy())), n


@pytest.mark.parametrize("H,W", [(540, 960), (1080, 1920)])
def test_metrics_match_float64_at_training_sizes(H, W):
    from mtgs_amd import color_correct, image_metrics
    pred, gt, mask, depth, lidar = _structured(H, W, seed=H)
    cc = color_correct(pred.cuda(), gt.cuda(), mask.cuda())
    m = image_metrics(pred.cuda(), gt.cuda(), mask.cuda(), pred_depth=depth.cuda(), lidar_depth=lidar.cuda())
    assert set(m) == {"psnr", "cc_psnr", "depth_RMSE", "depth_absRel", "depth_delta1"}
    assert all(v.dim() == 0 and v.is_cuda and v.dtype == torch.float32 for v in m.values())
    want = _cc_f64(pred.numpy(), gt.numpy(), mask.numpy())
    got = cc.cpu().numpy().reshape(-1, 3)
    err = np.abs(got - want).max()
    assert err <= 1e-5, f"color_correct differs from float64 by {err:.3g}"
    mk = mask.numpy()
    assert abs(m["psnr"].item() - _psnr(pred.numpy(), gt.numpy(), mk)) <= 1e-4
    assert abs(m["cc_psnr"].item() - _psnr(want, gt.numpy(), mk)) <= 1e-4
    # cc_psnr without the image equals the PSNR of color_correct's output (to f32 rounding)
    cc_direct = _psnr(got, gt.numpy(), mk)
    assert abs(m["cc_psnr"].item() - cc_direct) <= 4 * np.spacing(np.float32(cc_direct))
    assert m["cc_psnr"].item() > m["psnr"].item() + 1.0
    rmse, absrel, d1 = _depth_ref(depth, lidar, mask)
    assert abs(m["depth_RMSE"].item() - rmse) <= 1e-5 * rmse
    assert abs(m["depth_absRel"].item() - absrel) <= 1e-5 * absrel
    assert abs(m["depth_delta1"].item() - d1) <= 1e-6
    plain = image_metrics(pred.cuda(), gt.cuda(), mask.cuda(), color_corrected=False)
    assert set(plain) == {"psnr"} and torch.equal(plain["psnr"], m["psnr"])


def test_degenerate_inputs():
    from mtgs_amd import color_correct, image_metrics
    H, W = 40, 52
    g = torch.Generator().manual_seed(3)
    gt = torch.rand(H, W, 3, generator=g).cuda()
    # a constant image: every fit is singular -> the input comes back unchanged, cc_psnr is psnr
    const = torch.full((H, W, 3), 0.4, device="cuda")
    mask = (torch.rand(H, W, 1, generator=g) > 0.2).cuda()
    assert torch.equal(color_correct(const, gt, mask), const * mask)
    assert torch.equal(color_correct(const, gt), const)
    m = image_metrics(const, gt, mask)
    assert m["cc_psnr"].view(torch.int32).item() == m["psnr"].view(torch.int32).item()
    # an all-false mask: nothing to fit, nothing selected
    none = torch.zeros(H, W, 1, dtype=torch.bool, device="cuda")
    pred = torch.rand(H, W, 3, generator=g).cuda()
    assert torch.equal(color_correct(pred, gt, none), pred * none)
    d = torch.rand(H, W, 1, generator=g).cuda() + 1
    m = image_metrics(pred, gt, none, pred_depth=d, lidar_depth=d)
    assert m["cc_psnr"].view(torch.int32).item() == m["psnr"].view(torch.int32).item()
    assert all(torch.isnan(v).item() for v in m.values())
    # identical images: inf; a lidar without valid depths: nan; a zero predicted depth is a delta1 miss
    lidar = torch.full((H, W, 1), 10.0, device="cuda")
    depth = lidar.clone()
    depth[: H // 4] = 0.0
    m = image_metrics(gt, gt, pred_depth=depth, lidar_depth=lidar)
    assert m["psnr"].item() == float("inf") and m["cc_psnr"].item() > 60
    assert m["depth_delta1"].item() == pytest.approx(1 - (H // 4) / H, abs=1e-7)
    m = image_metrics(pred, gt, pred_depth=depth, lidar_depth=torch.full_like(lidar, 100.0))
    assert all(torch.isnan(m[k]).item() for k in ("depth_RMSE", "depth_absRel", "depth_delta1"))
    assert torch.equal(color_correct(pred, gt, num_iters=0), pred)


def test_metrics_are_bitwise_reproducible():
    from mtgs_amd import color_correct, image_metrics
    pred, gt, mask, depth, lidar = _structured(270, 480, seed=5)
    args = [t.cuda() for t in (pred, gt, mask)]
    a = color_correct(*args)
    b = color_correct(*args)
    assert torch.equal(a, b)
    ma = image_metrics(*args, pred_depth=depth.cuda(), lidar_depth=lidar.cuda())
    mb = image_metrics(*args, pred_depth=depth.cuda(), lidar_depth=lidar.cuda())
    assert all(torch.equal(ma[k], mb[k]) for k in ma)


def test_image_metrics_captures_in_a_graph():
    from mtgs_amd import image_metrics
    H, W = 270, 480
    first = [t.cuda() for t in _structured(H, W, seed=11)]
    second = [t.cuda() for t in _structured(H, W, seed=12)]
    static = [t.clone() for t in first]

    def step():
        p, g, mk, d, l = static
        return image_metrics(p, g, mk, pred_depth=d, lidar_depth=l)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                              # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for src in (second, first):
        for dst, t in zip(static, src):
            dst.copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        eager = image_metrics(src[0], src[1], src[2], pred_depth=src[3], lidar_depth=src[4])
        for k in eager:
            assert out[k].view(torch.int32).item() == eager[k].view(torch.int32).item(), k
