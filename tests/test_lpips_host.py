"""LPIPS (mtgs_amd/lpips.py, csrc/lpips.hip, include/mtgs_lpips.h) without a GPU: the header as a group of its own, the fp64
restatement's own properties (tests/lpips_refs.py), the tap-size arithmetic, and the weight handling (order, counts, repack)."""
import ctypes as C

import pytest
import torch

from mtgs_amd import lpips as L
from tests import lpips_refs as R

NAMES = ["mtgs_lpips", "mtgs_lpips_conv", "mtgs_lpips_conv_first", "mtgs_lpips_maxpool", "mtgs_lpips_repack", "mtgs_lpips_weight_floats",
         "mtgs_lpips_workspace_bytes"]


@pytest.fixture(scope="module")
def weights():
    return R.random_weights(seed=5)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_the_header_is_declared_bound_and_exported():
    """include/mtgs_lpips.h is a group of its own (tests/test_abi.py checks every group against its header, its reviewed record
    tests/golden/abi_signatures_lpips.txt and the library): its entry points and its constants."""
    from mtgs_amd import _abi, _lib
    abi = _abi.header_abi("mtgs_lpips.h")
    assert sorted(_lib.GROUPS["mtgs_lpips.h"]) == NAMES
    assert [abi.constants[k] for k in ("MTGS_LPIPS_NORM_SQRT_EPS_INSIDE", "MTGS_LPIPS_NORM_EPS_OUTSIDE")] == [L.NORMS["torchmetrics"], L.NORMS["lpips"]]
    assert abi.constants["MTGS_LPIPS_MIN_SIDE"] == L.MIN_SIDE == 31


def test_the_size_queries_need_no_device(hip_lib):
    """The flat weight array is what LpipsWeights lays out; the workspace holds the two largest activations of each parity and the
    partials; an image below 31 pixels on a side is refused with the reason."""
    n = C.c_size_t(0)
    assert hip_lib.mtgs_lpips_weight_floats(C.byref(n)) == 0
    assert n.value == sum(k * k * cin * cout + 2 * cout for cin, cout, k, *_ in L.LAYERS)
    assert hip_lib.mtgs_lpips_workspace_bytes(31, 31, C.byref(n)) == 0
    assert n.value == 4 * (2 * 7 * 7 * 64 + 2 * 3 * 3 * 64 + 5 * 256)      # conv1's tap, pool1 (> conv4's 2 * 256), partials
    assert hip_lib.mtgs_lpips_workspace_bytes(1080, 1920, C.byref(n)) == 0
    assert n.value == 4 * (2 * 269 * 479 * 64 + 2 * 134 * 239 * 64 + 5 * 256)
    assert hip_lib.mtgs_lpips_workspace_bytes(30, 64, C.byref(n)) != 0
    assert b"second pool" in hip_lib.mtgs_rast_last_error()


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", ["torchmetrics", "lpips"])
def test_identical_images_give_exactly_zero(weights, norm):
    pred, _, mask = R.images(35, 47, seed=1, masked=True)
    assert R.lpips_ref(pred, pred.clone(), mask, *weights, norm=norm) == 0.0
    assert R.lpips_ref(pred, pred.clone(), None, *weights, norm=norm, dtype=torch.float32) == 0.0


def test_symmetric_in_its_two_images(weights):
    pred, gt, mask = R.images(35, 47, seed=2, masked=True)
    a, b = R.lpips_ref(pred, gt, mask, *weights), R.lpips_ref(gt, pred, mask, *weights)
    assert a == b and a > 0


def test_tap_shapes_follow_the_formulas(weights):
    assert L.tap_sizes(31, 31) == [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)]
    assert L.tap_sizes(35, 47) == [(8, 11), (3, 5), (1, 2), (1, 2), (1, 2)]
    assert L.tap_sizes(1080, 1920) == [(269, 479), (134, 239), (66, 119), (66, 119), (66, 119)]
    assert L.tap_sizes(30, 31)[2][0] == 0                                   # no pixel after the second pool
    assert L.LAYERS == R.LAYERS
    for H, W in ((31, 31), (35, 47), (64, 96), (67, 131)):
        got = [tuple(t.shape[2:]) for t in R.taps(torch.zeros(1, 3, H, W, dtype=torch.float64), weights[0])]
        assert got == L.tap_sizes(H, W), (H, W)
        assert [t.shape[1] for t in R.taps(torch.zeros(1, 3, H, W, dtype=torch.float64), weights[0])] == [64, 192, 384, 256, 256]


def test_the_two_norm_forms_differ(weights):
    pred, gt, _ = R.images(35, 47, seed=3)
    a, b = R.lpips_ref(pred, gt, None, *weights, norm="torchmetrics"), R.lpips_ref(pred, gt, None, *weights, norm="lpips")
    assert a != b and abs(a - b) < 1e-3 * a                                 # eps against sums of squares of order 1 and more
    x = torch.full((1, 4, 1, 1), 1e-6, dtype=torch.float64)                 # a near-zero feature vector: the forms part
    assert not torch.allclose(R.unit(x, "torchmetrics"), R.unit(x, "lpips"), rtol=1e-3)
    with pytest.raises(ValueError):
        R.unit(x, "other")


def test_a_mask_of_zeros_is_two_constant_minus_one_images(weights):
    """x = img * mask is 0 BEFORE 2x - 1: every pixel enters the network as (-1 - shift) / scale, the same for both images."""
    pred, gt, _ = R.images(35, 47, seed=4)
    zeros = torch.zeros(35, 47, 1, dtype=torch.bool)
    assert R.lpips_ref(pred, gt, zeros, *weights) == 0.0
    x = R.transform(pred, zeros)
    minus_one = R.transform(torch.full((35, 47, 3), -1.0), None, normalize=False)
    assert torch.equal(x, minus_one)
    assert torch.equal(x[0, :, 0, 0], (-1 - torch.tensor(R.SHIFT, dtype=torch.float64)) / torch.tensor(R.SCALE, dtype=torch.float64))
    assert R.lpips_ref(pred, gt, None, *weights) > 0


# ---- weights ---------------------------------------------------------------------------------------------------------------------
def _module(convs, lins, n_convs=5):
    """A hand-built network in the order a module defines it: the backbone with ReLUs and pools between, a dropout and a bias-free
    1x1 Conv2d per lin layer, and a scaling layer with buffers that is no Conv2d."""
    feats = []
    for (w, b), (cin, cout, k, stride, pad, pool) in list(zip(convs, R.LAYERS))[:n_convs]:
        if pool:
            feats.append(torch.nn.MaxPool2d(3, 2))
        c = torch.nn.Conv2d(cin, cout, k, stride, pad)
        with torch.no_grad():
            c.weight.copy_(w)
            c.bias.copy_(b)
        feats += [c, torch.nn.ReLU()]
    heads = []
    for v in lins:
        c = torch.nn.Conv2d(v.numel(), 1, 1, bias=False)
        with torch.no_grad():
            c.weight.copy_(v.reshape(1, -1, 1, 1))
        heads.append(torch.nn.Sequential(torch.nn.Dropout(), c))
    return torch.nn.Sequential(torch.nn.Sequential(*feats), torch.nn.Identity(), torch.nn.ModuleList(heads))


def test_from_module_orders_the_layers(weights):
    convs, lins = weights
    w = L.LpipsWeights.from_module(_module(convs, lins))
    direct = L.LpipsWeights.from_tensors(convs, lins)
    assert torch.equal(w.flat, direct.flat) and w.flat.dtype == torch.float32 and w.flat.dim() == 1
    for i, ((cw, cb), v, (cin, cout, k, *_)) in enumerate(zip(convs, lins, R.LAYERS)):
        packed, bias, lin = w.layer(i)
        assert packed.shape == (k * k * cin, cout)
        assert torch.equal(L.unpack_conv_weight(packed, cin, k, k), cw) and torch.equal(bias, cb) and torch.equal(lin, v)


def test_from_module_raises_on_four_convolutions(weights):
    convs, lins = weights
    with pytest.raises(ValueError, match=r"found 4 with weights \[\(64, 3, 11, 11\).*and 5 with"):
        L.LpipsWeights.from_module(_module(convs, lins, n_convs=4))
    with pytest.raises(ValueError, match="found 5 .* and 4 with"):
        L.LpipsWeights.from_module(_module(convs, lins[:4]))


def test_from_tensors_checks_shapes(weights):
    convs, lins = weights
    narrow = [(convs[0][0][:48], convs[0][1][:48])] + convs[1:]
    with pytest.raises(NotImplementedError, match="cout = 48 is not a multiple of 32"):
        L.LpipsWeights.from_tensors(narrow, lins)
    with pytest.raises(ValueError, match="convolution 1: weight .* is not AlexNet's"):
        L.LpipsWeights.from_tensors([convs[0], convs[0]] + convs[2:], lins)
    with pytest.raises(ValueError, match="lin 2: 256 elements for 384 channels"):
        L.LpipsWeights.from_tensors(convs, lins[:2] + [lins[3]] + lins[3:])
    with pytest.raises(ValueError, match="bias"):
        L.LpipsWeights.from_tensors([(convs[0][0], None)] + convs[1:], lins)
    with pytest.raises(ValueError, match="got 4 and 5"):
        L.LpipsWeights.from_tensors(convs[:4], lins)


def test_the_weight_repack_round_trips():
    g = torch.Generator().manual_seed(0)
    for cout, cin, kh, kw in ((64, 3, 11, 11), (32, 5, 3, 2), (96, 16, 1, 1)):
        w = torch.randn(cout, cin, kh, kw, generator=g)
        p = L.repack_conv_weight(w)
        assert p.shape == (kh * kw * cin, cout) and p.is_contiguous()
        assert torch.equal(L.unpack_conv_weight(p, cin, kh, kw), w)
        ky, kx, c, o = kh - 1, kw // 2, cin - 1, 7
        assert p[(ky * kw + kx) * cin + c, o] == w[o, c, ky, kx]            # K runs (kh, kw, cin), cin fastest
    with pytest.raises(ValueError):
        L.unpack_conv_weight(p, 16, 3, 3)


def test_the_public_names():
    import mtgs_amd
    from mtgs_amd import metrics
    assert metrics.lpips is L.lpips and metrics.LpipsWeights is L.LpipsWeights
    assert mtgs_amd.LpipsWeights is L.LpipsWeights and mtgs_amd.lpips is L      # the module keeps its name; the function is metrics.lpips
