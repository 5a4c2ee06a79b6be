"""mtgs_amd.loss.pseudo_depth_loss (csrc/depthloss.hip) on the GPU against the float64 restatement of tests/depth_loss_refs.py.

Every case checks the value (2e-6 * max(1, |ref|)) and the gradient with a non-unit cotangent (rtol 2e-5, atol 1e-12): the
tolerances tests/test_gpu_image_edges.py applies to inverse_depth_l1.  A second run must be bit-identical (fixed summation
order).  No kind needs a looser bound: on these inputs the float32 PyTorch composition itself (depth_loss_refs with
dtype=float32, on the CPU) is within 0.07 of the value tolerance and within 1.1e-6 relative on the gradient (largest:
HuberL1 at 513x512), see MEASURED_F32.

Sizes (DL_BLOCK = 256 pixels per block, one block per 256 pixels up to DL_MAX_BLOCKS = 1024, the passes stride beyond):
15x17 = 255, 16x16 = 256, 6x43 = 258 and 1x257 / 257x1 (one pixel into the second block; the x or the y differences of
EdgeAwareLogL1 are empty there, and both at 1x1), 70x100, and 513x512 = 1026 blocks' worth on 1024 blocks."""
import numpy as np
import pytest
import torch

from tests import depth_loss_refs as R

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (15, 17), (16, 16), (6, 43), (1, 257), (257, 1), (70, 100), (513, 512)]
COT = 0.7

# Largest float32-vs-float64 error of the PyTorch composition over SIZES (CPU; value error over its tolerance, gradient relative):
# what a float32 kernel can be asked for.  All far inside the bounds used here, so none is widened.
MEASURED_F32 = {"mse": (0.047, 1.3e-7), "L1": (0.063, 1.8e-8), "InverseL1": (0.0045, 2.8e-7), "LogL1": (0.046, 1.3e-7),
                "HuberL1": (0.043, 1.1e-6), "EdgeAwareLogL1": (0.032, 2.6e-7)}

_REFS = {}


def _ref(key, pred, gt, mask, kind, rgb, **kw):
    """The float64 reference of a case, computed once."""
    if key not in _REFS:
        _REFS[key] = R.pseudo_depth_loss_f64(pred, gt, mask, kind, rgb, **kw)
    return _REFS[key]


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _dev(t):
    return None if t is None else t.cuda()


def _run(pred, gt, mask, kind, rgb, **kw):
    """value, gradient of COT * value; run twice, bit-identical."""
    from mtgs_amd.loss import pseudo_depth_loss
    gt_d, m_d, rgb_d = gt.cuda(), _dev(mask), _dev(rgb)
    res = []
    for _ in range(2):
        p = pred.cuda().requires_grad_(True)
        val = pseudo_depth_loss(p, gt_d, m_d, kind, rgb_d, **kw)
        (COT * val).backward()
        assert val.dtype == torch.float32 and val.dim() == 0 and p.grad.shape == pred.shape
        res.append((val.detach(), p.grad))
    assert _same_bits(res[0][0].reshape(1), res[1][0].reshape(1)) and _same_bits(res[0][1], res[1][1]), "two runs differ"
    return res[0]


def _compare(val, grad, ref, g_ref, where=None):
    val, ref = float(val), float(ref)
    print(f"value {val!r} ref {ref!r}")
    if np.isnan(ref):
        assert np.isnan(val)
    else:
        assert abs(val - ref) <= 2e-6 * max(1.0, abs(ref)), (val, ref)
    got, want = grad.cpu().double(), COT * g_ref
    if where is not None:
        got, want = got[where], want[where]
    print(f"gradient max abs err {float((got - want).abs().max()) if got.numel() else 0.0!r}")
    assert torch.allclose(got, want, rtol=2e-5, atol=1e-12)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("H,W", SIZES)
def test_sizes(H, W, kind):
    pred, gt, mask, rgb = R.depth_inputs(H, W)
    ref, g_ref = _ref(("size", H, W, kind), pred, gt, mask, kind, rgb)
    val, grad = _run(pred, gt, mask, kind, rgb)
    assert int(R.selection(gt, mask).sum()) > 0
    if kind == "EdgeAwareLogL1":
        assert np.isnan(float(ref)) == (H == 1 or W == 1)          # an empty difference image
    _compare(val, grad, ref, g_ref)
    assert torch.isfinite(grad).all()
    assert torch.equal(grad.cpu()[~R.selection(gt, mask)], torch.zeros(int((~R.selection(gt, mask)).sum()), 1))


def _small(seed=3):
    """5x7 inputs with every depth inside (lo, hi)."""
    pred, gt, _, rgb = R.depth_inputs(5, 7, seed)
    gt = gt.clamp(1.0, 45.0)
    pred = (gt + torch.randn(5, 7, 1, generator=torch.Generator().manual_seed(seed))).abs() + 0.05
    return pred, gt, rgb


@pytest.mark.parametrize("kind", R.KINDS)
def test_first_and_last_pixel_only(kind):
    pred, gt, rgb = _small()
    mask = torch.zeros(5, 7, 1, dtype=torch.bool)
    mask[0, 0] = mask[-1, -1] = True          # EdgeAwareLogL1: the last pixel has neither difference, n = 2, n_x = n_y = 1
    ref, g_ref = _ref(("first_last", kind), pred, gt, mask, kind, rgb)
    val, grad = _run(pred, gt, mask, kind, rgb)
    assert np.isfinite(float(ref)) and float(ref) > 0
    _compare(val, grad, ref, g_ref)
    assert int((grad != 0).sum()) == (1 if kind == "EdgeAwareLogL1" else 2)


@pytest.mark.parametrize("kind", R.KINDS)
def test_empty_selection_is_zero_with_a_zero_gradient(kind):
    pred, gt, rgb = _small()
    pred[2, 3] = float("nan")
    for mask, g in ((torch.zeros(5, 7, 1, dtype=torch.bool), gt), (None, gt * 0.0), (None, gt + 50.0)):
        val, grad = _run(pred, g, mask, kind, rgb)
        assert float(val) == 0.0 and torch.equal(grad, torch.zeros_like(grad))


@pytest.mark.parametrize("kind", R.KINDS)
def test_selection_confined_to_the_last_column(kind):
    pred, gt, rgb = _small()
    mask = torch.zeros(5, 7, 1, dtype=torch.bool)
    mask[:, -1] = True
    ref, g_ref = _ref(("last_col", kind), pred, gt, mask, kind, rgb)
    val, grad = _run(pred, gt, mask, kind, rgb)
    assert np.isnan(float(ref)) == (kind == "EdgeAwareLogL1")       # its x term is a mean over nothing
    _compare(val, grad, ref, g_ref)
    assert torch.isfinite(grad).all() and bool((grad[:-1, -1] != 0).all())


@pytest.mark.parametrize("kind", R.KINDS)
def test_gt_exactly_at_lo_and_hi_is_not_selected(kind):
    pred, gt, rgb = _small()
    lo, hi = torch.tensor(0.1), torch.tensor(50.0)
    gt[0, 0], gt[0, 1], gt[1, 0], gt[1, 1] = lo, hi, torch.nextafter(lo, hi), torch.nextafter(hi, lo)
    sel = R.selection(gt)
    assert not sel[0, 0] and not sel[0, 1] and sel[1, 0] and sel[1, 1]
    ref, g_ref = _ref(("lo_hi", kind), pred, gt, None, kind, rgb)
    val, grad = _run(pred, gt, None, kind, rgb)
    _compare(val, grad, ref, g_ref)
    assert float(grad[0, 0]) == 0.0 and float(grad[0, 1]) == 0.0 and float(grad[1, 0]) != 0.0 and float(grad[1, 1]) != 0.0


@pytest.mark.parametrize("kind", R.KINDS)
def test_exact_zero_errors_send_no_gradient(kind):
    pred, gt, rgb = _small()
    pred[0, 0], pred[2, 4], pred[-1, -1] = gt[0, 0], gt[2, 4], gt[-1, -1]
    ref, g_ref = _ref(("zero_err", kind), pred, gt, None, kind, rgb)
    val, grad = _run(pred, gt, None, kind, rgb)
    _compare(val, grad, ref, g_ref)
    assert float(grad[0, 0]) == 0.0 and float(grad[2, 4]) == 0.0 and float(grad[-1, -1]) == 0.0


@pytest.mark.parametrize("kind", R.KINDS)
def test_nan_in_an_unselected_pixel_stays_out(kind):
    pred, gt, rgb = _small()
    mask = torch.ones(5, 7, 1, dtype=torch.bool)
    mask[1, 2] = False
    gt[3, 3] = 55.0                              # unselected by the range
    pred[1, 2] = pred[3, 3] = float("nan")
    sel = R.selection(gt, mask).reshape(5, 7, 1)
    ref, g_ref = _ref(("nan", kind), pred, gt, mask, kind, rgb)
    val, grad = _run(pred, gt, mask, kind, rgb)
    assert np.isfinite(float(ref)) and int((~sel).sum()) == 2
    _compare(val, grad, ref, g_ref, where=sel)
    assert torch.equal(grad.cpu()[~sel], torch.zeros(2))


def test_huber_tied_maxima_and_d_zero():
    pred, gt, rgb = _small()
    assert float((pred - gt).abs().max()) < 8.0
    gt[0, 1], pred[0, 1] = 8.0, 16.0             # e = +8 and -8 exactly: the two maxima
    gt[4, 5], pred[4, 5] = 16.0, 8.0
    ref, g_ref = _ref(("huber_tie",), pred, gt, None, "HuberL1", rgb, huber_thresh=0.5)
    val, grad = _run(pred, gt, None, "HuberL1", rgb, huber_thresh=0.5)
    _compare(val, grad, ref, g_ref)
    assert float(grad[0, 1]) == -float(grad[4, 5]) and float(grad[0, 1]) > COT / 35       # the L1 share plus half of d's
    val, grad = _run(gt.clone(), gt, None, "HuberL1", rgb)                                 # d = 0
    assert float(val) == 0.0 and torch.equal(grad, torch.zeros_like(grad))


@pytest.mark.parametrize("kind", R.KINDS)
def test_layouts_and_mask_types_agree(kind):
    from mtgs_amd.loss import pseudo_depth_loss
    pred, gt, mask, rgb = R.depth_inputs(15, 17)
    rgb_d = rgb.cuda()

    def run(p, g, m):
        p = p.cuda().requires_grad_(True)
        val = pseudo_depth_loss(p, g.cuda(), _dev(m), kind, rgb_d)
        (COT * val).backward()
        return val.detach().reshape(1), p.grad.reshape(15, 17)
    base = run(pred, gt, mask)
    for p, g, m in ((pred[..., 0], gt[..., 0], mask[..., 0]), (pred, gt[..., 0], mask.to(torch.uint8)),
                    (pred[..., 0], gt, (mask[..., 0] * 255).to(torch.uint8))):
        other = run(p, g, m)
        assert _same_bits(base[0], other[0]) and _same_bits(base[1], other[1])
    p = pred[..., 0].cuda().requires_grad_(True)
    pseudo_depth_loss(p, gt.cuda(), None, kind, rgb_d).backward()
    assert p.grad.shape == (15, 17)


def test_forward_and_backward_capture_in_a_graph():
    """One graph holds every kind, forward and backward.  The input VALUES are rewritten and the graph replayed: the results
    equal the eager ones of the new values bit for bit, also when the new selection is empty (decided on the device)."""
    from mtgs_amd.loss import pseudo_depth_loss
    H, W = 33, 47
    a, b = R.depth_inputs(H, W, 1), R.depth_inputs(H, W, 2)
    empty = (b[0], b[1] * 0.0, b[2], b[3])
    s_pred, s_gt, s_mask, s_rgb = (t.cuda().clone() for t in a)
    s_pred.requires_grad_(True)

    def step(pred, gt, mask, rgb):
        out = []
        for kind in R.KINDS:
            val = pseudo_depth_loss(pred, gt, mask, kind, rgb)
            (g,) = torch.autograd.grad(COT * val, pred)
            out += [val.reshape(1), g]
        return out

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(s_pred, s_gt, s_mask, s_rgb)                 # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(s_pred, s_gt, s_mask, s_rgb)
    for case in (b, empty, a):
        pred, gt, mask, rgb = (t.cuda() for t in case)
        with torch.no_grad():
            s_pred.copy_(pred)
        s_gt.copy_(gt)
        s_mask.copy_(mask)
        s_rgb.copy_(rgb)
        graph.replay()
        torch.cuda.synchronize()
        eager = step(pred.requires_grad_(True), gt, mask, rgb)
        for x, y in zip(out, eager):
            assert _same_bits(x, y)
        if case is empty:
            assert all(float(x.detach().abs().max()) == 0.0 for x in out)
        else:
            assert all(float(x.detach().abs().max()) > 0.0 for x in out)
