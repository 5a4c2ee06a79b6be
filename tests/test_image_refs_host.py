"""tests/image_refs.py without a GPU: (1) each reference reproduces the golden vectors the reference's own code produced
(ssim_ref.npz, depth_normals_ref.npz, color_correct_ref.npz) and the pinned SSIM oracle; (2) the degenerate sizes behave as the
docstrings say: NaN with a ZERO gradient where the reference's mean runs over an empty tensor, 0 where the reference guards;
(3) the inputs of tests/test_gpu_image_edges.py are chosen so that the float32 and the float64 run of the reference ALONE
disagree on fewer elements than the caps that file allows, and within the tolerances it takes from the existing tests."""
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import image_refs as R
from tests import test_gpu_image_edges as E

GOLDEN = Path(__file__).resolve().parent / "golden"
F32 = torch.float32


# ---- (1) golden vectors ---------------------------------------------------------------------------------------------------------
def test_ssim_ref_reproduces_the_reference_vectors_and_the_oracle():
    from oracle import ssim_oracle
    z = np.load(GOLDEN / "ssim_ref.npz")
    cases = sorted({k.split("_")[0] for k in z.files})
    assert len(cases) >= 4
    for c in cases:
        gt, pred = torch.from_numpy(z[f"{c}_gt"]), torch.from_numpy(z[f"{c}_pred"])
        mask = None if z[f"{c}_mask"].size == 0 else torch.from_numpy(z[f"{c}_mask"])
        val, grad = R.ssim_ref(gt, pred, mask)
        assert abs(float(val) - float(z[f"{c}_ssim_f64"])) <= 1e-12, c
        assert np.abs(grad.numpy() - z[f"{c}_grad_f64"]).max() <= 1e-12, c
        v_o, g_o = ssim_oracle.masked_ssim(gt.numpy(), pred.numpy(), None if mask is None else mask.numpy(), with_grad=True)
        assert abs(float(val) - v_o) <= 1e-12 and np.abs(grad.numpy() - g_o).max() <= 1e-12, c


def test_depth_normal_refs_reproduce_the_reference_vectors():
    z = np.load(GOLDEN / "depth_normals_ref.npz")
    for c in [str(c) for c in z["cases"]]:
        depth, K = torch.from_numpy(z[f"{c}_depth"]), torch.from_numpy(z[f"{c}_K"])
        mask, pred = torch.from_numpy(z[f"{c}_mask"]), torch.from_numpy(z[f"{c}_pred"])
        want = torch.from_numpy(z[f"{c}_normals64"])
        got = R.normals_from_depth_ref(depth, K)
        assert torch.equal(torch.isnan(got), torch.isnan(want)), c
        torch.testing.assert_close(got, want, rtol=0, atol=1e-12, equal_nan=True, msg=lambda m: f"{c}: {m}")
        val, grad, _ = R.depth_normal_loss_ref(pred, depth, K, mask)
        # the golden float64 run also compared the depth with lo and hi in float64, where 0.1f > 0.1: `zeros_range` places depths
        # exactly on lo, which the float32 reference (and so image_refs) leaves out; its float32 run is the witness there
        if c == "zeros_range":
            assert abs(float(val) - float(z[f"{c}_loss32"])) <= 1e-5 * abs(float(z[f"{c}_loss32"])), c
            near = (torch.from_numpy(z[f"{c}_normals32"]) - pred).abs() < 1e-6
            torch.testing.assert_close(grad[~near].float(), torch.from_numpy(z[f"{c}_grad32"])[~near], rtol=1e-5, atol=1e-10)
        elif np.isnan(float(z[f"{c}_loss64"])):
            assert torch.isnan(val), c
        else:
            assert abs(float(val) - float(z[f"{c}_loss64"])) <= 1e-12, c
            torch.testing.assert_close(grad, torch.from_numpy(z[f"{c}_grad64"]), rtol=0, atol=1e-12, msg=lambda m: f"{c}: {m}")


def test_color_correct_ref_reproduces_the_reference_vectors():
    z = np.load(GOLDEN / "color_correct_ref.npz")
    names = sorted({k.split("_")[0] for k in z.files})
    assert len(names) >= 5
    for n in names:
        mask = z[f"{n}_mask"] if z[f"{n}_mask"].size else None
        info = {}
        got = R.color_correct_ref(z[f"{n}_pred"], z[f"{n}_gt"], mask, iters=int(z[f"{n}_iters"]), info=info)
        err = np.abs(got - z[f"{n}_cc_f64"].reshape(-1, 3)).max()
        assert err <= 1e-9, (n, err)          # two float64 least-squares solvers (gelsd here, the reference's torch.linalg.lstsq)
        assert info["min_rank"] == 10, n


# ---- (2) degenerate sizes -------------------------------------------------------------------------------------------------------
def _nan_with_zero_grad(val, grad):
    return bool(torch.isnan(val)) and torch.equal(grad, torch.zeros_like(grad))


@pytest.mark.parametrize("kind", ["margin", "empty"])
def test_ssim_ref_empty_selection_is_nan_with_a_zero_gradient(kind):
    gt, pred, mask = E.ssim_inputs(12, 16, kind)
    assert _nan_with_zero_grad(*R.ssim_ref(gt, pred, mask))
    gt, pred, mask = E.ssim_inputs(11, 11, "corner")           # one output pixel: a mean over three elements
    val, grad = R.ssim_ref(gt, pred, mask)
    assert torch.isfinite(val) and float(grad.abs().max()) > 0


def test_l1_refs_on_empty_selections():
    gt, pred = torch.rand(3, 5, 2), torch.rand(3, 5, 2)
    assert _nan_with_zero_grad(*R.masked_l1_ref(gt, pred, torch.zeros(3, 5, 1, dtype=torch.bool)))
    val, grad = R.masked_l1_ref(gt, gt.clone(), None)            # exact ties: sign(0) = 0
    assert float(val) == 0.0 and torch.equal(grad, torch.zeros_like(grad))
    # the lidar depth term guards an empty selection: 0, zero gradient; lo and hi themselves are outside (strict comparisons)
    depth = torch.full((2, 2, 1), 5.0)
    gt_d = torch.tensor([0.1, 80.0, 0.0, 100.0]).reshape(2, 2, 1)
    val, grad, m = R.inverse_depth_l1_ref(depth, gt_d)
    assert float(val) == 0.0 and torch.equal(grad, torch.zeros_like(grad)) and not m.any()
    gt_d[1, 1] = 79.0
    val, grad, m = R.inverse_depth_l1_ref(depth, gt_d)
    assert int(m.sum()) == 1 and float(val) == pytest.approx(abs(1 / 79.00001 - 1 / 5.00001), rel=1e-6)
    assert float(grad[1, 1]) == pytest.approx(-1 / 5.00001 ** 2, rel=1e-9) and int((grad != 0).sum()) == 1


def test_tv_ref_empty_halves_and_nan_pixels():
    assert _nan_with_zero_grad(*R.tv_ref(torch.rand(1, 1, 3)))
    x = torch.tensor([[[1.0]], [[3.0]]])                          # 2 x 1: the left/right mean is empty, the up/down one is not
    val, grad = R.tv_ref(x)
    assert torch.isnan(val) and grad.flatten().tolist() == [-1.0, 1.0]
    x = torch.tensor([[[1.0], [float("nan")], [2.0]], [[3.0], [4.0], [6.0]]])
    val, grad = R.tv_ref(x)                                       # torch.sign(NaN) = 0: the gradient stays finite
    assert torch.isnan(val) and torch.isfinite(grad).all()
    assert grad.flatten().tolist() == pytest.approx([-1 / 3, 0.0, -1 / 3, 1 / 3 - 1 / 4, 0.0, 1 / 3 + 1 / 4])


def test_ncc_and_oob_refs_on_empty_selections():
    gt, pred, mask = E.ncc_inputs(40, 50, 4, 9, "empty")
    val, grad, n = R.depth_ncc_ref(pred, gt, mask, 4, 9)
    assert n == 0 and _nan_with_zero_grad(val, grad)
    val, grad, n = R.depth_ncc_ref(pred, gt, None, 64, 16)        # a patch larger than the image: no valid patch either
    assert n == 0 and _nan_with_zero_grad(val, grad)
    # the out-of-box term: nothing visible, or nothing out of its box: 0 with zero gradients
    means, ops = torch.tensor([[9.0, 0, 0], [0.1, 0, 0]]), torch.zeros(2, 1)
    for radii, m in ((torch.zeros(1, 2, dtype=torch.int32), means), (torch.ones(1, 2, dtype=torch.int32), means * 0.01)):
        val, grads = R.oob_ref([(m, ops, [1.0, 1.0, 1.0])], radii, [0])
        assert float(val) == 0.0 and torch.equal(grads[0], torch.zeros(2, 1, dtype=torch.float64))
    val, grads = R.oob_ref([(means, ops, [1.0, 1.0, 1.0])], torch.ones(1, 2, dtype=torch.int32), [0])
    assert float(val) == pytest.approx(-np.log(0.5 + 1e-6)) and float(grads[0][1]) == 0.0 and float(grads[0][0]) > 0
    assert float(R.oob_ref([], torch.zeros(1, 4, dtype=torch.int32), [])[0]) == 0.0


@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (7, 1), (2, 2)])
def test_geom_refs_below_the_stencil(H, W):
    pred, depth, K, _ = E.geom_inputs(H, W, "none")
    assert torch.equal(R.normals_from_depth_ref(depth, K), torch.full((H, W, 3), 0.5, dtype=torch.float64))
    val, grad, _ = R.depth_normal_loss_ref(pred, depth, K, None, tv=False)
    assert torch.isfinite(val) or H * W < 3
    val, grad, _ = R.depth_normal_loss_ref(pred, depth, K, None, tv=True)
    assert bool(torch.isnan(val)) == (H == 1 or W == 1 or H * W < 3) and torch.isfinite(grad).all()
    val, grad, _ = R.depth_normal_loss_ref(pred, depth, K, torch.zeros(H, W, 1, dtype=torch.bool), tv=False)
    assert _nan_with_zero_grad(val, grad)


def test_scale_and_metric_refs_on_empty_inputs():
    two, sharp, g = R.scale_reg_ref(torch.empty(0, 3), True)
    assert torch.isnan(two) and torch.isnan(sharp) and g.shape == (0, 3)
    # the documented tie rule agrees with autograd wherever a row has no ties
    s, ties = E.scale_inputs(257)
    for two_d in (True, False):
        _, _, g = R.scale_reg_ref(s, two_d, 10.0, 0.7, 1.3)
        for i in (1, 2, 3, 100, 255):
            want = R.scale_reg_rule_grad(s[i], two_d, 10.0, 257, 0.7, 1.3)
            assert g[i].tolist() == pytest.approx(want, rel=1e-12, abs=1e-18)
    assert ties == [0, 256]
    img, ref = np.random.default_rng(0).random((2, 4, 3), dtype=np.float32), np.random.default_rng(1).random((2, 4, 3), dtype=np.float32)
    info = {}
    out = R.color_correct_ref(img, ref, np.zeros((2, 4, 1), bool), info=info)
    assert np.array_equal(out, np.zeros((8, 3))) and info["min_rank"] == 0
    assert np.isnan(R.psnr_ref(img, ref, np.zeros((2, 4, 1), bool))) and R.psnr_ref(img, img) == float("inf")
    d = torch.full((2, 4, 1), 10.0)
    assert all(np.isnan(v) for v in R.depth_metrics_ref(d, d * 10, None))
    assert R.depth_metrics_ref(d, d, None) == (0.0, 0.0, 1.0)


# ---- (3) the inputs of the GPU edge tests: float32 and float64 runs of the reference alone ----------------------------------------
@pytest.mark.parametrize("alpha_kind", ["mixed", "zero", "positive"])
@pytest.mark.parametrize("H,W", E.HEAD_SIZES)
def test_head_inputs_stay_clear_of_the_clamp_edges(H, W, alpha_kind):
    """Fewer render / alpha gradient elements than the cap differ between the float32 and the float64 run of the reference (a
    value within fp32 rounding of a clamp edge takes the other branch), and the outputs agree to the 3e-6 the GPU test allows."""
    for D, with_exposure, with_depth, normal_ch in E.HEAD_CONFIGS:
        args = E.head_inputs(H, W, D, with_exposure, with_depth, normal_ch, alpha_kind)
        o64, g64 = R.output_head_ref(*args, with_depth, normal_ch)
        o32, g32 = R.output_head_ref(*args, with_depth, normal_ch, dtype=F32)
        for a, b in zip(o32, o64):
            assert a is None or float((a.double() - b).abs().max()) < 3e-6 / 4
        for a, b, name in zip(g32, g64, ("render", "alpha", "background", "exposure")):
            if a is None:
                continue
            scale = float(b.abs().max()) + 1e-12
            diff = (a.double() - b).abs()
            if name in ("render", "alpha"):
                assert float((diff > 2e-5 * scale).double().mean()) < E.HEAD_GRAD_CAP / 4, (name, D)
            else:
                assert float(diff.max()) < 5e-4 * scale / 4, (name, D)


@pytest.mark.parametrize("H,W", E.GEOM_SIZES)
def test_geom_inputs_are_well_conditioned(H, W):
    """The float32 run of the normal reference is within a quarter of the tolerance of the float64 one, and few elements of
    |target - pred| lie inside the band the gradient comparison leaves out."""
    pred, depth, K, _ = E.geom_inputs(H, W, "none")
    n64, n32 = R.normals_from_depth_ref(depth, K), R.normals_from_depth_ref(depth, K, dtype=F32)
    assert float((n32.double() - n64).abs().max()) <= E.NORMAL_TOL / 4
    unsure = ((n64 - pred.double()).abs() <= 1e-3).double().mean()
    assert float(unsure) <= E.GEOM_UNSURE_CAP or H * W < 256


@pytest.mark.parametrize("P", [191, 192, 193])
def test_small_metric_inputs_select_the_same_rows_in_both_precisions(P):
    """Below 200 pixels one row more or less moves the colour fit: no tested value lies within 1e-5 of a clip threshold (fp32
    rounding is 6e-8), and every fit has full rank."""
    pred, gt, _, _ = E.metric_inputs(P)
    info = {}
    R.color_correct_ref(pred.numpy(), gt.numpy(), None, info=info)
    assert info["min_rank"] == 10 and info["margin"] > 1e-5, info


def test_scale_inputs_stay_clear_of_max_ratio():
    s, _ = E.scale_inputs(65537)
    srt = torch.sort(s.double(), dim=-1, descending=True)[0]
    for ratio in (srt[:, 0] / srt[:, 1], srt[:, 0] / srt[:, 2]):
        assert float((ratio - 10.0).abs().min()) > 1.0


def test_measured_tolerances_are_four_times_the_float32_reference_error():
    """GEOM_MEASURED_ATOL holds, per case, 4 x the largest absolute difference between the float32 and the float64 run of the
    reference's gradient (with the GPU test's cotangent 0.9) over the elements that test compares."""
    for (H, W, kind, tv), atol in E.GEOM_MEASURED_ATOL.items():
        pred, depth, K, mask = E.geom_inputs(H, W, kind)
        _, g64, target = R.depth_normal_loss_ref(pred, depth, K, mask, tv=tv)
        _, g32, _ = R.depth_normal_loss_ref(pred, depth, K, mask, tv=tv, dtype=F32)
        sure = (target - pred.double()).abs() > 1e-3
        e32 = float((0.9 * g32.double() - 0.9 * g64)[sure].abs().max())
        assert atol == pytest.approx(4 * e32, rel=0.02), (H, W, kind, tv, e32)
