"""The image-space loss and metric kernels at the sizes where their tiling or their reduction changes behaviour
(csrc/loss.hip, tv.hip, ncc.hip, head.hip, oob.hip, geomloss.hip, metrics.hip), through mtgs_amd.loss / mtgs_amd.metrics.

Every kernel here has a tiled or blocked first pass that writes per-block partials and a single-workgroup finish that walks
them with a stride of 256.  Each case checks (1) the value against the float64 reference of tests/image_refs.py, (2) every
gradient the operator returns against float64 autograd, (3) a second run, which must be bit-identical (fixed summation order).
Sizes sit at extent - 1, extent, extent + 1 of each kernel's per-block extent and at 256 / 257 blocks (the finish loop's second
trip); the comment beside each list names the constant it is derived from.  Contiguous float32 inputs only.

Tolerances are those of the existing test of the same operator (test_gpu_loss.py, test_gpu_geom_loss.py, test_gpu_metrics.py).
The input builders are shared with tests/test_image_refs_host.py, which checks without a GPU that the float32 and the float64
run of the reference alone disagree on fewer elements than the caps used here.

An empty selection: the reference's mean over an empty tensor is NaN and autograd scatters nothing back, so the gradient is
ZERO (masked SSIM, masked L1, depth NCC, the empty half of a one-pixel-wide TV); the lidar depth term and the out-of-box
term guard it and return 0."""
import numpy as np
import pytest
import torch

from tests import image_refs as R
from tests.util import REPORT

pytestmark = pytest.mark.gpu


def _rec(op, case, **errs):
    REPORT.append(dict({"kind": "image_edges", "op": op, "case": str(case)}, **{k: float(v) for k, v in errs.items()}))


def _same_bits(a, b):
    """torch.equal that also holds for NaN results: the two runs must agree bit for bit."""
    if a is None or b is None:
        return a is None and b is None
    if a.dtype == torch.float32:
        return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)


def _twice(fn):
    """fn() -> tuple of tensors; runs it twice, asserts bit identity, returns the first result."""
    a, b = fn(), fn()
    for i, (x, y) in enumerate(zip(a, b)):
        assert _same_bits(x, y), f"output {i} differs between two runs"
    return a


def _value_err(val, ref):
    """|val - ref|, 0 when both are NaN, inf when only one is."""
    val, ref = float(val), float(ref)
    if np.isnan(ref) or np.isnan(val):
        return 0.0 if (np.isnan(ref) and np.isnan(val)) else float("inf")
    return abs(val - ref)


def pixel_mask(kind, H, W, seed=0):
    """[H,W,1] bool or None: none / random / last (the last pixel only) / empty (all false)."""
    if kind == "none":
        return None
    m = torch.zeros(H, W, 1, dtype=torch.bool)
    if kind == "random":
        m = torch.rand(H, W, 1, generator=torch.Generator().manual_seed(seed + 17)) > 0.4
    elif kind == "last":
        m[-1, -1] = True
    else:
        assert kind == "empty", kind
    return m


def _dev(t):
    return None if t is None else t.cuda()


# ---- masked SSIM --------------------------------------------------------------------------------------------------------------
# loss.hip: WIN = 11 (HALO = 10), TILE = 16, IN_TILE = 26; the forward grid tiles the (H-10) x (W-10) map, the backward the image.
# one output pixel; one row / column of outputs; 2 outputs; 6 (a ragged first tile); TILE - 1 + ...; exactly one tile (26);
# one pixel into the next tile (27); two ragged tiles (42 x 43); 266 x 266 = 16 x 16 = 256 forward tiles; 267 x 266 = 17 x 16 = 272.
SSIM_SIZES = [(11, 11), (11, 40), (40, 11), (12, 12), (16, 16), (17, 32), (26, 26), (26, 27), (27, 27), (42, 43), (266, 266),
              (267, 266)]
SSIM_MASKS = ["none", "random", "lastrc", "corner", "margin", "empty"]


def ssim_inputs(H, W, kind):
    g = torch.Generator().manual_seed(H * 1000 + W)
    gt = torch.rand(H, W, 3, generator=g)
    pred = (gt + 0.2 * torch.randn(H, W, 3, generator=g)).clamp(0, 1)
    m = None
    if kind != "none":
        m = torch.zeros(H, W, 1, dtype=torch.bool)
        if kind == "random":
            m = torch.rand(H, W, 1, generator=g) > 0.3
            m[5, 5] = True                # (the first output pixel: the selection is never empty, also at 11 x 11)
        elif kind == "lastrc":            # only the last output row and column: image row H - 6, column W - 6 of the cropped map
            m[H - 6, 5:W - 5] = True
            m[5:H - 5, W - 6] = True
        elif kind == "corner":            # the single output pixel (OH - 1, OW - 1)
            m[H - 6, W - 6] = True
        elif kind == "margin":            # true only inside the 5-pixel margin that the crop removes
            m[:] = True
            m[5:H - 5, 5:W - 5] = False
    return gt, pred, m


@pytest.mark.parametrize("kind", SSIM_MASKS)
@pytest.mark.parametrize("H,W", SSIM_SIZES)
def test_masked_ssim_edges(H, W, kind):
    """Value 5e-6, gradient 2e-5 of its maximum (test_gpu_loss.py).  A mask that selects nothing (all false, or true only in
    the cropped margin): NaN with a zero gradient, as autograd through the reference's ssim_map[mask].mean()."""
    from mtgs_amd.loss import masked_ssim
    gt, pred, mask = ssim_inputs(H, W, kind)
    ref, g_ref = R.ssim_ref(gt, pred, mask)
    gt_d, m_d = gt.cuda(), _dev(mask)

    def run():
        p = pred.cuda().requires_grad_(True)
        val = masked_ssim(gt_d, p, m_d)
        (1.0 - val).backward()               # the loss MTGS forms
        return val.detach(), p.grad
    val, grad = _twice(run)
    ev = _value_err(val, ref)
    eg = float((grad.cpu().double() + g_ref).abs().max())
    _rec("masked_ssim", (H, W, kind), value_err=ev, grad_err=eg, grad_max=float(g_ref.abs().max()))
    assert np.isnan(float(ref)) == (kind in ("margin", "empty"))
    assert ev <= 5e-6, ev
    assert eg <= 2e-5 * float(g_ref.abs().max()), eg


@pytest.mark.parametrize("H,W", [(10, 64), (64, 10), (10, 10), (5, 3)])
def test_masked_ssim_refuses_images_smaller_than_the_window(H, W):
    from mtgs_amd.loss import masked_ssim
    with pytest.raises(ValueError):
        masked_ssim(torch.rand(H, W, 3), torch.rand(H, W, 3))


# ---- masked L1, inverse-depth L1 ------------------------------------------------------------------------------------------------
# loss.hip: L1_PIX = 1024 pixels per forward block, 256 per backward block: 255 / 256 / 257 and 1023 / 1024 / 1025 pixels;
# 512 x 512 = 256 partials, 513 x 512 = 257 (the finish loop's second trip).
L1_SIZES = [(1, 1), (1, 255), (1, 256), (1, 257), (3, 341), (1, 1024), (1, 1025), (512, 512), (513, 512)]
L1_MASKS = ["none", "random", "last", "empty"]


@pytest.mark.parametrize("kind", L1_MASKS)
@pytest.mark.parametrize("ch", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("H,W", L1_SIZES)
def test_masked_l1_edges(H, W, ch, kind):
    """Value 2e-6, gradient rtol 1e-5 (test_gpu_loss.py); exact ties (sign(0) = 0) in the first and the last pixel; an all-false
    mask gives NaN with a zero gradient."""
    from mtgs_amd.loss import masked_l1
    g = torch.Generator().manual_seed(H * 7 + W + ch)
    gt = torch.rand(H, W, ch, generator=g)
    pred = torch.rand(H, W, ch, generator=g)
    pred[0, 0] = gt[0, 0]
    pred[-1, -1] = gt[-1, -1]
    mask = pixel_mask(kind, H, W, seed=H + W)
    ref, g_ref = R.masked_l1_ref(gt, pred, mask)
    gt_d, m_d = gt.cuda(), _dev(mask)

    def run():
        p = pred.cuda().requires_grad_(True)
        val = masked_l1(gt_d, p, m_d)
        (0.8 * val).backward()
        return val.detach(), p.grad
    val, grad = _twice(run)
    ev = _value_err(val, ref)
    _rec("masked_l1", (H, W, ch, kind), value_err=ev, grad_err=float((grad.cpu().double() - 0.8 * g_ref).abs().max()))
    assert np.isnan(float(ref)) == (kind == "empty")
    assert ev <= 2e-6, ev
    assert torch.allclose(grad.cpu().double(), 0.8 * g_ref, rtol=1e-5, atol=1e-12)
    assert torch.equal(grad[0, 0], torch.zeros_like(grad[0, 0])) and torch.equal(grad[-1, -1], torch.zeros_like(grad[-1, -1]))


@pytest.mark.parametrize("kind", L1_MASKS + ["no_return"])
@pytest.mark.parametrize("H,W", L1_SIZES)
def test_inverse_depth_l1_edges(H, W, kind):
    """Value 2e-6 * max(1, |ref|), gradient rtol 2e-5, the mask by-product equal (test_gpu_loss.py).  The comparisons with lo and
    hi are strict: the first pixel holds 0.1f (= lo as the kernel receives it), the last one 80 (= hi), so neither is selected;
    with the last-pixel mask, or a lidar without returns, the selection is empty: 0 with a zero gradient."""
    from mtgs_amd.loss import inverse_depth_l1
    g = torch.Generator().manual_seed(H * 5 + W)
    gt = torch.rand(H, W, 1, generator=g) * 100.0
    gt[torch.rand(H, W, 1, generator=g) < 0.3] = 0.0
    pred = torch.rand(H, W, 1, generator=g) * 60.0 + 0.5
    if H * W > 2:
        pred.view(-1)[1] = gt.view(-1)[1] = 7.25          # an exact tie inside the range
    gt.view(-1)[0] = 0.1
    gt.view(-1)[-1] = 80.0
    if kind == "no_return":
        gt = gt * 0.0
    mask = pixel_mask("none" if kind == "no_return" else kind, H, W, seed=H)
    ref, g_ref, m_ref = R.inverse_depth_l1_ref(pred, gt, mask)
    gt_d, m_d = gt.cuda(), _dev(mask)

    def run():
        p = pred.cuda().requires_grad_(True)
        val, m = inverse_depth_l1(p, gt_d, m_d)
        (0.5 * val).backward()
        return val.detach(), p.grad, m
    val, grad, m = _twice(run)
    ev = _value_err(val, ref)
    _rec("inverse_depth_l1", (H, W, kind), value_err=ev, grad_err=float((grad.cpu().double() - 0.5 * g_ref).abs().max()))
    assert m.dtype == torch.bool and m.shape == (H, W, 1) and torch.equal(m.cpu(), m_ref)
    assert not bool(m_ref.view(-1)[0]) and not bool(m_ref.view(-1)[-1])
    if kind in ("last", "empty", "no_return"):
        assert int(m_ref.sum()) == 0 and float(ref) == 0.0 and float(val) == 0.0
    assert ev <= 2e-6 * max(1.0, abs(float(ref))), ev
    assert torch.allclose(grad.cpu().double(), 0.5 * g_ref, rtol=2e-5, atol=1e-12)


# ---- total variation ------------------------------------------------------------------------------------------------------------
# tv.hip: TV_BLOCK = 256 ELEMENTS (H W C) per block.  1 x 1 and 2 x 1 / 1 x 2: both means, or one, are empty; 255 / 256 / 257 / 258
# elements; 65536 elements = 256 partials, 65712 and 65792 = 257, 66048 = 258.
TV_SIZES = [(1, 1, 1), (1, 1, 3), (2, 1, 3), (1, 2, 4), (2, 2, 1), (2, 2, 3), (2, 2, 4), (5, 17, 3), (16, 16, 1), (8, 8, 4),
            (257, 1, 1), (1, 257, 1), (43, 2, 3), (256, 256, 1), (128, 128, 4), (148, 148, 3), (257, 256, 1), (129, 128, 4)]
TV_CASES = [(h, w, c, False) for h, w, c in TV_SIZES] + [(2, 2, 3, True), (5, 17, 3, True), (16, 16, 1, True), (148, 148, 3, True)]


@pytest.mark.parametrize("H,W,C_,nan_pixel", TV_CASES)
def test_tv_loss_edges(H, W, C_, nan_pixel):
    """Value 2e-6, gradient rtol 1e-5 atol 1e-9 (test_gpu_loss.py).  An empty difference tensor (W = 1 or H = 1) makes the value
    NaN and sends no gradient; a NaN pixel makes the value NaN while the gradient follows torch.sign(NaN) = 0 and stays finite."""
    from mtgs_amd.loss import tv_loss
    g = torch.Generator().manual_seed(H * 3 + W + C_)
    x0 = torch.rand(H, W, C_, generator=g)
    if W > 1:
        x0[0, 0] = x0[0, 1]                       # exact ties: sign(0) = 0
    if nan_pixel:
        x0[H // 2, W // 2, 0] = float("nan")
    ref, g_ref = R.tv_ref(x0)

    def run():
        x = x0.cuda().requires_grad_(True)
        val = tv_loss(x)
        (1.5 * val).backward()
        return val.detach(), x.grad
    val, grad = _twice(run)
    ev = _value_err(val, ref)
    _rec("tv_loss", (H, W, C_, nan_pixel), value_err=ev, grad_err=float((grad.cpu().double() - 1.5 * g_ref).abs().max()))
    assert np.isnan(float(ref)) == (H == 1 or W == 1 or nan_pixel)
    assert ev < 2e-6, ev
    assert torch.isfinite(g_ref).all()
    assert torch.allclose(grad.cpu().double(), 1.5 * g_ref, rtol=1e-5, atol=1e-9)


# ---- depth NCC ------------------------------------------------------------------------------------------------------------------
# ncc.hip: one workgroup (NCC_BLOCK = 256 threads) per patch, the finish walks the patches with a stride of 256.
# (H, W, k, s): k == 1 with one patch along y; s > k; s == 1; k odd with k k = 289 (no multiple of 64, two strided trips);
# 16 x 16 = 256 patches, 16 x 17 = 272, 26 x 26 = 676.
NCC_GEOMS = [(9, 40, 1, 16), (40, 50, 4, 9), (12, 13, 4, 1), (60, 70, 17, 8), (60, 60, 4, 4), (60, 64, 4, 4), (100, 100, 4, 4)]


def ncc_inputs(H, W, k, s, kind):
    g = torch.Generator().manual_seed(H + k)
    gt = torch.rand(H, W, 1, generator=g) * 30 + 1
    pred = gt + torch.randn(H, W, 1, generator=g) * 2
    mask = None
    if kind == "one_pixel":          # the last pixel of the LAST patch that lies inside the image: no other inside patch holds it
        mask = torch.ones(H, W, 1, dtype=torch.bool)
        pad = k // 2
        i = (H - k + pad) // s
        j = (W - k + pad) // s
        mask[i * s - pad + k - 1, j * s - pad + k - 1] = False
    elif kind == "empty":
        mask = torch.zeros(H, W, 1, dtype=torch.bool)
    return gt, pred, mask


@pytest.mark.parametrize("kind", ["none", "one_pixel", "empty"])
@pytest.mark.parametrize("H,W,k,s", NCC_GEOMS)
def test_depth_ncc_edges(H, W, k, s, kind):
    """Value 2e-5, gradient 1e-3 of its maximum (test_gpu_loss.py); every patch invalid: NaN with a zero gradient."""
    from mtgs_amd.loss import depth_ncc_loss
    gt, pred, mask = ncc_inputs(H, W, k, s, kind)
    ref, g_ref, n_valid = R.depth_ncc_ref(pred, gt, mask, k, s)
    _, _, n_all = R.depth_ncc_ref(pred, gt, None, k, s)
    gt_d, m_d = gt.cuda(), _dev(mask)

    def run():
        p = pred.cuda().requires_grad_(True)
        val = depth_ncc_loss(p, gt_d, patch_size=k, stride=s, mask=m_d)
        (2.0 * val).backward()
        return val.detach(), p.grad
    val, grad = _twice(run)
    ev = _value_err(val, ref)
    eg = float((grad.cpu().double() - 2.0 * g_ref).abs().max())
    _rec("depth_ncc", (H, W, k, s, kind), value_err=ev, grad_err=eg, grad_max=float((2.0 * g_ref).abs().max()), valid=n_valid)
    assert n_all > 0 and (n_valid == 0) == (kind == "empty")
    if kind == "one_pixel":
        assert n_all - n_valid == 1
    assert ev <= 2e-5, ev
    assert eg <= 1e-3 * float((2.0 * g_ref).abs().max()), eg


# ---- output head ----------------------------------------------------------------------------------------------------------------
# head.hip: HEAD_BLOCK = 256 pixels per block, head_finish_kernel sums HEAD_RED = 15 columns of per-block partials with a stride of
# 256: 1 / 255 / 256 / 257 pixels, 256 x 256 = 256 blocks, 1 x 65537 = 257 blocks.
HEAD_SIZES = [(1, 1), (1, 255), (1, 256), (1, 257), (256, 256), (1, 65537)]
HEAD_CONFIGS = [(8, True, True, 3), (4, True, True, -1), (3, False, False, -1), (7, False, True, 3)]
HEAD_GRAD_CAP = 1e-3        # share of render / alpha gradient elements that may take the other clamp branch than float64


def head_inputs(H, W, D, with_exposure, with_depth, normal_ch, alpha_kind):
    g = torch.Generator().manual_seed(D * 7 + normal_ch + H + W)
    render = torch.rand(1, H, W, D, generator=g) * 1.4 - 0.2
    if with_depth:
        render[..., -1] = torch.rand(1, H, W, generator=g) * 30
    alpha = torch.rand(1, H, W, 1, generator=g) * 0.98 + 0.01
    if alpha_kind == "zero":
        alpha = torch.zeros(1, H, W, 1)            # nothing hit: depth takes the maximum everywhere
    elif alpha_kind == "mixed":
        alpha[0, :, : (W + 4) // 5] = 0.0
        alpha[0, -1, -1] = 0.5                     # exactly representable: lands ON the clamp edges in fp32 and fp64
        render[0, -1, -1, :3] = torch.tensor([0.0, 1.0, 0.5]) - 0.125
    else:
        assert alpha_kind == "positive"
    bg = torch.full((3,), 0.25)
    E = (torch.eye(3, 4) + 0.1 * torch.randn(3, 4, generator=g)) if with_exposure else None
    cots = [torch.randn(H, W, 3, generator=g), torch.randn(H, W, 3, generator=g), torch.randn(H, W, 1, generator=g),
            torch.randn(H, W, 3, generator=g)]
    return render, alpha, bg, E, cots


@pytest.mark.parametrize("alpha_kind", ["mixed", "zero", "positive"])
@pytest.mark.parametrize("D,with_exposure,with_depth,normal_ch", HEAD_CONFIGS)
@pytest.mark.parametrize("H,W", HEAD_SIZES)
def test_output_head_edges(H, W, D, with_exposure, with_depth, normal_ch, alpha_kind):
    """Values 3e-6; render / alpha gradients 2e-5 of their maximum on all but HEAD_GRAD_CAP of the elements (a pixel within fp32
    rounding of a clamp edge may take the other branch), background / exposure gradients 5e-4 of their maximum
    (test_gpu_loss.py)."""
    from mtgs_amd.loss import output_head
    render, alpha, bg, E, cots = head_inputs(H, W, D, with_exposure, with_depth, normal_ch, alpha_kind)
    ref_out, ref_grad = R.output_head_ref(render, alpha, bg, E, cots, with_depth, normal_ch)
    cots_d = [c.cuda() for c in cots]

    def run():
        P = [None if t is None else t.cuda().requires_grad_(True) for t in (render, alpha, bg, E)]
        outs = output_head(*P, depth=with_depth, normal_channel=normal_ch)
        sum((o * c).sum() for o, c in zip(outs, cots_d) if o is not None).backward()
        return tuple(None if o is None else o.detach() for o in outs) + tuple(None if p is None else p.grad for p in P)
    res = _twice(run)
    out, grad = res[:4], res[4:]
    errs = {}
    for o, r, name in zip(out, ref_out, ("rgb", "rgb_appearance", "depth", "normal")):
        assert (o is None) == (r is None), name
        if o is not None:
            assert o.shape == r.shape, (name, o.shape, r.shape)
            errs[name] = float((o.cpu().double() - r).abs().max())
    if with_depth and alpha_kind == "zero":
        assert torch.equal(out[2], torch.full_like(out[2], float(render[..., -1].max())))
    for gq, gr, name in zip(grad, ref_grad, ("render", "alpha", "background", "exposure")):
        assert (gq is None) == (gr is None), name
        if gq is not None:
            assert gq.shape == gr.shape, name
            scale = float(gr.abs().max()) + 1e-12
            diff = (gq.cpu().double() - gr).abs()
            errs["d_" + name] = float(diff.max()) / scale
            errs["d_" + name + "_share"] = float((diff > 2e-5 * scale).double().mean())
    _rec("output_head", (H, W, D, with_exposure, with_depth, normal_ch, alpha_kind), **errs)
    for name in ("rgb", "rgb_appearance", "depth", "normal"):
        assert errs.get(name, 0.0) < 3e-6, (name, errs[name])
    for name in ("render", "alpha"):
        assert errs["d_" + name + "_share"] < HEAD_GRAD_CAP, (name, errs)
    for name in ("background", "exposure"):
        assert errs.get("d_" + name, 0.0) < 5e-4, (name, errs)


# ---- normals from depth, depth-supervised normal loss ---------------------------------------------------------------------------
# geomloss.hip: GL_BLOCK = 256 pixels per block, the fp64 finish (finish_sums) walks the partials with a stride of 256.
# H or W below 3: the image is all border and the TV neighbours run off it; 255 / 256 / 257 / 258 pixels;
# 256 x 256 = 256 blocks, 257 x 256 = 257.
GEOM_SIZES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 3), (15, 17), (16, 16), (1, 257), (3, 86), (256, 256), (257, 256)]
GEOM_MASKS = ["none", "random", "last", "empty", "beyond_hi"]
NORMAL_TOL = 2e-4           # normals_from_depth against float64 (test_gpu_geom_loss.py)
# The L1 part's sign(pred - target) is compared where |target - pred| > 1e-3 in float64 (test_gpu_geom_loss.py): the fp32 target
# is within NORMAL_TOL of the fp64 one.  pred is uniform on [0, 1], so about 2e-3 of the elements fall inside that band; the
# cap is five times that (small images have few elements).
GEOM_UNSURE_CAP = 1e-2
# A one-row image that is selected almost everywhere has 3 * count (765) next to the TV count (768): where the two parts have
# opposite signs the gradient element is their difference, 4.6e-6 of two terms of 1.2e-3, and fp32 rounds each term.  That is
# conditioning: the float32 run of the reference on the CPU differs from the float64 one by 2.09e-10 (absolute, the largest over
# the compared elements) for this case; 4 x that is allowed as the absolute tolerance (the device measured 9.3e-11).
GEOM_MEASURED_ATOL = {(1, 257, "none", True): 4 * 2.09e-10}


def geom_inputs(H, W, kind):
    g = torch.Generator().manual_seed(H * 11 + W)
    depth = R.scene_depth(H, W, seed=H + W)
    if H * W >= 3:                         # strict comparisons: exactly lo (as the kernel receives it) and exactly hi are out
        depth.view(-1)[0] = 0.1
        depth.view(-1)[1] = 50.0
    if kind == "beyond_hi":
        depth = torch.full_like(depth, 60.0)
    K = torch.tensor([[0.9 * W + 0.25, 0.0, W / 2 - 0.75], [0.0, 0.85 * W + 0.5, H / 2 + 0.5], [0.0, 0.0, 1.0]])
    pred = torch.rand(H, W, 3, generator=g)
    mask = pixel_mask("none" if kind == "beyond_hi" else kind, H, W, seed=W)
    return pred, depth, K, mask


@pytest.mark.parametrize("H,W", GEOM_SIZES)
def test_normals_from_depth_edges(H, W):
    from mtgs_amd.loss import normals_from_depth
    _, depth, K, _ = geom_inputs(H, W, "none")
    want = R.normals_from_depth_ref(depth, K)
    d_d, K_d = depth.cuda(), K.cuda()
    (got,) = _twice(lambda: (normals_from_depth(d_d, K_d),))
    got = got.cpu()
    err = float((got.double() - want).abs().max())
    _rec("normals_from_depth", (H, W), err=err)
    assert got.shape == (H, W, 3) and err < NORMAL_TOL, err
    assert (got[0] == 0.5).all() and (got[-1] == 0.5).all() and (got[:, 0] == 0.5).all() and (got[:, -1] == 0.5).all()


@pytest.mark.parametrize("tv", [True, False])
@pytest.mark.parametrize("kind", GEOM_MASKS)
@pytest.mark.parametrize("H,W", GEOM_SIZES)
def test_depth_normal_loss_edges(H, W, kind, tv):
    """Value 1e-5 relative, gradient rtol 1e-5 where the sign of target - pred is sure (test_gpu_geom_loss.py).  An empty selection
    (a false mask, depth outside [lo, hi]) or, with tv, a one-pixel-wide image gives NaN; the gradient of an empty part is zero."""
    from mtgs_amd.loss import depth_normal_loss
    pred, depth, K, mask = geom_inputs(H, W, kind)
    ref, g_ref, target = R.depth_normal_loss_ref(pred, depth, K, mask, tv=tv)
    d_d, K_d, m_d = depth.cuda(), K.cuda(), _dev(mask)

    def run():
        p = pred.cuda().requires_grad_(True)
        val = depth_normal_loss(p, d_d, K_d, m_d, tv=tv)
        (0.9 * val).backward()
        return val.detach(), p.grad
    val, grad = _twice(run)
    ev = _value_err(val, ref)
    sure = (target - pred.double()).abs() > 1e-3
    eg = float((grad.cpu().double() - 0.9 * g_ref)[sure].abs().max()) if sure.any() else 0.0
    atol = GEOM_MEASURED_ATOL.get((H, W, kind, tv), 1e-12)
    _rec("depth_normal_loss", (H, W, kind, tv), value_err=ev, grad_err=eg, unsure=float((~sure).double().mean()), atol=atol)
    if kind in ("empty", "beyond_hi") or (tv and (H == 1 or W == 1)):
        assert np.isnan(float(ref))
    assert ev <= 1e-5 * abs(float(ref)) or ev == 0.0, (ev, float(ref))
    assert float((~sure).double().mean()) <= GEOM_UNSURE_CAP or H * W < 256
    assert torch.isfinite(grad).all()
    torch.testing.assert_close(grad.cpu().double()[sure], (0.9 * g_ref)[sure], rtol=1e-5, atol=atol)


# ---- scale regularisers ---------------------------------------------------------------------------------------------------------
# geomloss.hip: GL_BLOCK = 256 rows per block: 255 / 256 / 257 rows, 65536 rows = 256 blocks, 65537 = 257; no rows at all.
SCALE_NS = [0, 1, 255, 256, 257, 65536, 65537]


def scale_inputs(n):
    """Rows uniform on [1, 2] (ratios below 2), every third one with its first entry times 30 (ratios 15 .. 60): no ratio within
    rounding of max_ratio = 10, so fp32 and fp64 take the same branch of maximum() in every row.  The first and the last row
    hold ties."""
    s = torch.rand(n, 3, generator=torch.Generator().manual_seed(n + 1)) + 1.0
    s[::3, 0] *= 30.0
    ties = []
    if n:
        s[0] = torch.tensor([2.0, 2.0, 0.125])
        s[-1] = torch.tensor([3.0, 0.25, 0.25]) if n > 1 else s[-1]
        ties = sorted({0, n - 1})
    return s, ties


@pytest.mark.parametrize("two_d", [True, False])
@pytest.mark.parametrize("n", SCALE_NS)
def test_scale_regularizers_edges(n, two_d):
    """Values 1e-5 relative, gradient rtol 2e-5 atol 1e-13 against float64 autograd, the tie rows against the documented rule
    (test_gpu_geom_loss.py); no rows: NaN (the mean of an empty tensor) and an empty gradient."""
    from mtgs_amd.loss import scale_regularizers
    s, ties = scale_inputs(n)
    t64, h64, g64 = R.scale_reg_ref(s, two_d, 10.0, 0.7, 1.3, tie_rows=ties)

    def run():
        sc = s.cuda().requires_grad_(True)
        two, sharp = scale_regularizers(sc, two_d=two_d)
        (0.7 * two + 1.3 * sharp).backward()
        return two.detach(), sharp.detach(), sc.grad
    two, sharp, grad = _twice(run)
    e0, e1 = _value_err(two, t64), _value_err(sharp, h64)
    _rec("scale_regularizers", (n, two_d), two_d_err=e0, sharp_err=e1,
         grad_err=float((grad.cpu().double() - g64).abs().max()) if n else 0.0)
    assert np.isnan(float(t64)) == (n == 0) and grad.shape == (n, 3)
    assert e0 <= 1e-5 * abs(float(t64)) or e0 == 0.0
    assert e1 <= 1e-5 * abs(float(h64)) or e1 == 0.0
    torch.testing.assert_close(grad.cpu().double(), g64, rtol=2e-5, atol=1e-13)


# ---- out-of-box regulariser -----------------------------------------------------------------------------------------------------
# oob.hip: OOB_BLOCK = 256 Gaussians per block, blocks of all nodes in one grid, the finish walks them with a stride of 256.
# 157 + 118 + 2 = 277 blocks in total; a node of exactly 256 Gaussians and a last node of 257.
OOB_CASES = [[40000, 30000, 257], [300, 256, 257], [255, 1, 256]]


@pytest.mark.parametrize("sizes", OOB_CASES, ids=lambda s: "-".join(map(str, s)))
def test_oob_loss_edges(sizes):
    """Value 2e-5 * max(1, |ref|), gradients rtol 2e-4 atol 1e-7 (test_gpu_loss.py)."""
    from mtgs_amd.loss import oob_loss
    g = torch.Generator().manual_seed(sum(sizes))
    starts, s = [], 1000
    for k in sizes:
        starts.append(s)
        s += k
    total = s + 333
    radii = (torch.randint(0, 30, (1, total), generator=g) * (torch.rand(1, total, generator=g) < 0.05)).int()
    radii[0, starts[-1] + sizes[-1] - 1] = 5                   # the last Gaussian of the last node is visible
    nodes = [(torch.randn(k, 3, generator=g) * 2.0, torch.randn(k, 1, generator=g) * 2, [2.5, 1.5, 4.0]) for k in sizes]
    ref, g_ref = R.oob_ref(nodes, radii, starts, tolerance=1.5)
    radii_d, means_d = radii.cuda(), [m.cuda() for m, _, _ in nodes]

    def run():
        P = [o.cuda().requires_grad_(True) for _, o, _ in nodes]
        val = oob_loss([(m, p, size) for m, p, (_, _, size) in zip(means_d, P, nodes)], radii_d, starts, tolerance=1.5)
        (3.0 * val).backward()
        return (val.detach(),) + tuple(p.grad for p in P)
    res = _twice(run)
    ev = _value_err(res[0], ref)
    _rec("oob_loss", sizes, value_err=ev,
         grad_err=max(float((gq.cpu().double() - 3.0 * gr).abs().max()) for gq, gr in zip(res[1:], g_ref)))
    assert float(ref) > 0 and ev <= 2e-5 * max(1.0, abs(float(ref)))
    for gq, gr in zip(res[1:], g_ref):
        assert gq.shape == gr.shape
        assert torch.allclose(gq.cpu().double(), 3.0 * gr, rtol=2e-4, atol=1e-7)


# ---- image metrics --------------------------------------------------------------------------------------------------------------
# metrics.hip: AB = 192 pixels per accumulation workgroup, grid_of(P) = ceil(P / (2 AB)) clamped to MAX_GRID = 1024, which it
# reaches at P = 1024 * 384 = 393216: 392832 pixels use 1023 workgroups, 393216 exactly 1024, 393217 one pixel past the clamp.
METRIC_PS = [1, 191, 192, 193, 392832, 393216, 393217]
METRIC_MASKS = ["none", "last", "empty"]
_metric_cache = {}


def metric_inputs(P):
    g = torch.Generator().manual_seed(P)
    gt = torch.rand(1, P, 3, generator=g)
    pred = (0.05 + 0.85 * gt + 0.15 * gt * gt - 0.1 * gt[..., [1, 2, 0]] * gt + 0.02 * torch.randn(1, P, 3, generator=g)).clamp(0, 1)
    lidar = torch.where(torch.rand(1, P, 1, generator=g) > 0.5, 1 + 90 * torch.rand(1, P, 1, generator=g), torch.zeros(1, P, 1))
    depth = lidar * (1 + 0.3 * torch.randn(1, P, 1, generator=g)) + 0.5
    lidar[0, -1, 0], depth[0, -1, 0] = 10.0, 9.0        # the last pixel always has a return
    return pred, gt, depth, lidar


def metric_reference(P, kind):
    """The float64 references of one case, computed once and shared by the two tests below (never modified)."""
    key = (P, kind)
    if key not in _metric_cache:
        pred, gt, depth, lidar = metric_inputs(P)
        mask = pixel_mask(kind, 1, P)
        info = {}
        mk = None if mask is None else mask.numpy()
        cc = R.color_correct_ref(pred.numpy(), gt.numpy(), mk, info=info)
        _metric_cache[key] = dict(cc=cc, info=info, psnr=R.psnr_ref(pred.numpy(), gt.numpy(), mk),
                                  cc_psnr=R.psnr_ref(cc, gt.numpy(), mk), depth=R.depth_metrics_ref(depth, lidar, mask))
    return _metric_cache[key]


@pytest.mark.parametrize("kind", METRIC_MASKS)
@pytest.mark.parametrize("P", METRIC_PS)
def test_color_correct_edges(P, kind):
    """1e-5 against the float64 formulation (test_gpu_metrics.py) where every fit has full rank.  Where a fit is rank deficient
    (fewer than ten usable rows: one pixel, the last-pixel mask) the reference returns lstsq's minimum-norm solution while the
    device returns img * mask unchanged, as mtgs_amd.metrics.color_correct documents; that fallback is what is asserted then.
    An all-false mask gives zeros in both."""
    from mtgs_amd import color_correct
    pred, gt, _, _ = metric_inputs(P)
    mask = pixel_mask(kind, 1, P)
    ref = metric_reference(P, kind)
    args = (pred.cuda(), gt.cuda(), _dev(mask))
    (out,) = _twice(lambda: (color_correct(*args),))
    masked = pred if mask is None else pred * mask
    if ref["info"]["min_rank"] < 10:
        assert kind != "none" or P < 10
        assert torch.equal(out.cpu(), masked)
        err = 0.0
    else:
        err = float(np.abs(out.cpu().numpy().reshape(-1, 3).astype(np.float64) - ref["cc"]).max())
        assert not torch.equal(out.cpu(), masked)
    _rec("color_correct", (P, kind), err=err, min_rank=ref["info"]["min_rank"])
    assert err <= 1e-5, err
    if kind == "empty":
        assert torch.equal(out, torch.zeros_like(out)) and float(np.abs(ref["cc"]).max()) == 0.0


@pytest.mark.parametrize("kind", METRIC_MASKS)
@pytest.mark.parametrize("P", METRIC_PS)
def test_image_metrics_edges(P, kind):
    """psnr and cc_psnr 1e-4 dB, depth_RMSE and depth_absRel 1e-5 relative, depth_delta1 1e-6 (test_gpu_metrics.py); an empty
    selection gives NaN everywhere; where the colour fit is rank deficient cc_psnr is psnr bit for bit (the documented
    fallback, see test_color_correct_edges)."""
    from mtgs_amd import image_metrics
    pred, gt, depth, lidar = metric_inputs(P)
    mask = pixel_mask(kind, 1, P)
    ref = metric_reference(P, kind)
    args = (pred.cuda(), gt.cuda(), _dev(mask))
    d_d, l_d = depth.cuda(), lidar.cuda()
    keys = ("psnr", "cc_psnr", "depth_RMSE", "depth_absRel", "depth_delta1")

    def run():
        m = image_metrics(*args, pred_depth=d_d, lidar_depth=l_d)
        assert set(m) == set(keys)
        return tuple(m[k].reshape(1) for k in keys)
    m = dict(zip(keys, (float(v) for v in _twice(run))))
    rmse, absrel, d1 = ref["depth"]
    fallback = ref["info"]["min_rank"] < 10
    errs = dict(psnr=_value_err(m["psnr"], ref["psnr"]), cc_psnr=0.0 if fallback else _value_err(m["cc_psnr"], ref["cc_psnr"]),
                rmse=_value_err(m["depth_RMSE"], rmse), absrel=_value_err(m["depth_absRel"], absrel),
                delta1=_value_err(m["depth_delta1"], d1))
    _rec("image_metrics", (P, kind), **errs)
    if kind == "empty":
        assert all(np.isnan(v) for v in m.values()) and np.isnan(ref["psnr"]) and np.isnan(rmse)
    if fallback:
        assert np.float32(m["cc_psnr"]).view(np.int32) == np.float32(m["psnr"]).view(np.int32)
    assert errs["psnr"] <= 1e-4 and errs["cc_psnr"] <= 1e-4, errs
    assert errs["rmse"] <= 1e-5 * abs(rmse) or errs["rmse"] == 0.0, errs
    assert errs["absrel"] <= 1e-5 * abs(absrel) or errs["absrel"] == 0.0, errs
    assert errs["delta1"] <= 1e-6, errs
