"""tests/depth_loss_refs.py (the float64 restatement that pins mtgs_amd.loss.pseudo_depth_loss on the GPU) against cases worked
out by hand, and the argument checks of pseudo_depth_loss that need no GPU.

The 2x2 image: pred = [[1, 2], [4, 3]], gt = [[2, 2], [1, 7]], so e = pred - gt = [[-1, 0], [3, -4]], all four selected."""
import enum
import math

import pytest
import torch

from tests import depth_loss_refs as R

PRED = torch.tensor([[1.0, 2.0], [4.0, 3.0]])
GT = torch.tensor([[2.0, 2.0], [1.0, 7.0]])
# mean |colour difference|: (0,0)-(0,1) 0.6, (1,0)-(1,1) 0, (0,0)-(1,0) 0.3, (0,1)-(1,1) 0.3
RGB = torch.tensor([[[0.0, 0.0, 0.0], [0.3, 0.6, 0.9]], [[0.3, 0.3, 0.3], [0.3, 0.3, 0.3]]], dtype=torch.float64)


def _check(kind, value, grad, pred=PRED, gt=GT, **kw):
    val, g = R.pseudo_depth_loss_f64(pred, gt, kind=kind, **kw)
    assert val.dtype == torch.float64 and g.shape == pred.shape
    assert float(val) == pytest.approx(value, rel=1e-7, abs=1e-12), (float(val), value)       # (the inputs are float32 numbers)
    assert torch.allclose(g, torch.tensor(grad, dtype=torch.float64).reshape(pred.shape), rtol=1e-7, atol=1e-12), g


def test_mse_l1_logl1_2x2():
    _check("mse", (1 + 0 + 9 + 16) / 4, [-0.5, 0.0, 1.5, -2.0])
    _check("L1", (1 + 0 + 3 + 4) / 4, [-0.25, 0.0, 0.25, -0.25])                               # abs'(0) = 0
    _check("LogL1", math.log(2 * 1 * 4 * 5) / 4, [-1 / 8, 0.0, 1 / 16, -1 / 20])


def test_inverse_l1_2x2_uses_1e_6():
    eps = 1e-6
    ip = [1 / (p + eps) for p in (1.0, 2.0, 4.0, 3.0)]
    ig = [1 / (g + eps) for g in (2.0, 2.0, 1.0, 7.0)]
    value = sum(abs(a - b) for a, b in zip(ip, ig)) / 4
    # d |ip - ig| / d pred = sgn(ip - ig) * (-ip^2): pred < gt gives ip > ig
    _check("InverseL1", value, [-ip[0] ** 2 / 4, 0.0, ip[2] ** 2 / 4, -ip[3] ** 2 / 4])
    far = sum(abs(1 / (p + 1e-5) - 1 / (g + 1e-5)) for p, g in zip((1.0, 2.0, 4.0, 3.0), (2.0, 2.0, 1.0, 7.0))) / 4
    assert abs(far - value) > 1e-7      # the lidar branch's 1e-5 is another number at this precision


def test_huber_2x2():
    # thresh 0.5: d = 0.5 * 4 = 2.  |e| < d: e = -1 -> (1 + 4) / 4, e = 0 -> 4 / 4; the others keep |e|.
    value = (1.25 + 1.0 + 3.0 + 4.0) / 4
    dl_dd = ((0.5 - 1 / 8) + 0.5) / 4
    _check("HuberL1", value, [(-1 / 2) / 4, 0.0, 0.25, -0.25 - 0.5 * dl_dd], huber_thresh=0.5)
    # the default 0.2: d = 0.8, only e = 0 is quadratic: 0.64 / 1.6 = 0.4, dL/dd = 0.5 / 4
    _check("HuberL1", (0.4 + 1 + 3 + 4) / 4, [-0.25, 0.0, 0.25, -0.25 - 0.2 * 0.125])


def test_huber_tied_maxima_share_the_gradient_of_d():
    pred = torch.tensor([[1.0, 9.0], [4.0, 6.0]])
    gt = torch.tensor([[5.0, 5.0], [3.0, 6.0]])            # e = [[-4, 4], [1, 0]]: two maxima
    dl_dd = ((0.5 - 1 / 8) + 0.5) / 4
    half = 0.5 * dl_dd / 2
    _check("HuberL1", (4 + 4 + 1.25 + 1.0) / 4, [-0.25 - half, 0.25 + half, (1 / 2) / 4, 0.0], pred=pred, gt=gt, huber_thresh=0.5)


def test_huber_d_zero_is_zero_not_nan():
    val, g = R.pseudo_depth_loss_f64(GT.clone(), GT, kind="HuberL1")
    assert float(val) == 0.0 and torch.equal(g, torch.zeros(2, 2, dtype=torch.float64))


def test_edge_aware_2x2():
    ln2, ln4 = math.log(2), math.log(4)
    ex, ey = math.exp(-0.6), math.exp(-0.3)
    # Lx: (0,0) ex ln2, (1,0) 1 * ln4;  Ly: (0,0) ey ln2, (0,1) ey * log(1 + 0) = 0
    g00 = -0.5 * (ex / 2 + ey / 2)
    _check("EdgeAwareLogL1", (ex * ln2 + ln4) / 2 + (ey * ln2) / 2, [g00, 0.0, 0.25 * (1 / 2), 0.0], rgb=RGB)
    # the neighbour's mask is not consulted: masking (0,1) out leaves Lx[0,0] in and only removes Ly[0,1]
    mask = torch.tensor([[True, False], [True, True]])
    _check("EdgeAwareLogL1", (ex * ln2 + ln4) / 2 + ey * ln2, [-0.5 * (ex / 2 + ey), 0.0, 0.125, 0.0], rgb=RGB, mask=mask)
    # a selection confined to the last column: no x difference is selected, 0 / 0
    val, g = R.pseudo_depth_loss_f64(PRED, GT, torch.tensor([[False, True], [False, True]]), "EdgeAwareLogL1", RGB)
    assert math.isnan(float(val)) and torch.isfinite(g).all()


def test_lo_and_hi_are_strict():
    lo, hi = torch.tensor(0.1), torch.tensor(50.0)
    up, down = torch.nextafter(lo, hi), torch.nextafter(hi, lo)
    gt = torch.stack([torch.stack([lo, hi]), torch.stack([up, down])])
    assert R.selection(gt).tolist() == [[False, False], [True, True]]
    pred = gt + 1.0
    val, g = R.pseudo_depth_loss_f64(pred, gt, kind="L1")
    assert float(val) == pytest.approx(1.0, rel=1e-6) and g.tolist() == [[0.0, 0.0], [0.5, 0.5]]
    val, g = R.pseudo_depth_loss_f64(pred[:1], gt[:1], kind="L1")                              # nothing selected
    assert float(val) == 0.0 and torch.equal(g, torch.zeros(1, 2, dtype=torch.float64))


class _Kinds(enum.Enum):          # stands in for the reference's DepthLossType: members are accepted by their .value
    TV = "TV"
    EdgeAwareTV = "EdgeAwareTV"
    L1 = "L1"


def test_argument_checks_need_no_gpu():
    from mtgs_amd.loss import pseudo_depth_loss
    pred, gt = torch.rand(4, 6, 1, requires_grad=True), torch.rand(4, 6, 1) * 10
    rgb = torch.rand(4, 6, 3)
    for kind in ("TV", "EdgeAwareTV", _Kinds.TV, _Kinds.EdgeAwareTV):
        with pytest.raises(NotImplementedError, match="TV"):
            pseudo_depth_loss(pred, gt, kind=kind)
    with pytest.raises(ValueError, match="unknown depth loss kind"):
        pseudo_depth_loss(pred, gt, kind="l1")
    with pytest.raises(ValueError, match="needs rgb"):
        pseudo_depth_loss(pred, gt)                                      # the default kind reads the image
    with pytest.raises(NotImplementedError, match="gt_depth"):
        pseudo_depth_loss(pred, gt.clone().requires_grad_(True), kind="L1")
    with pytest.raises(NotImplementedError, match="rgb"):
        pseudo_depth_loss(pred, gt, rgb=rgb.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="huber_thresh"):
        pseudo_depth_loss(pred, gt, kind="HuberL1", huber_thresh=0.0)
    with pytest.raises(AssertionError):
        pseudo_depth_loss(pred, torch.rand(6, 4, 1), kind="L1")          # depth of another size
    with pytest.raises(AssertionError):
        pseudo_depth_loss(pred, gt, mask=torch.ones(4, 6, 1), kind="L1")  # a float mask
    with pytest.raises(AssertionError):
        pseudo_depth_loss(pred, gt, rgb=torch.rand(4, 6, 4))
    # accepted arguments reach the device check: there is no CPU path
    for kind in ("L1", _Kinds.L1):
        with pytest.raises(RuntimeError, match="HIP device"):
            pseudo_depth_loss(pred, gt, kind=kind)
    with pytest.raises(RuntimeError, match="HIP device"):
        pseudo_depth_loss(pred, gt, torch.ones(4, 6, dtype=torch.uint8), rgb=rgb)
