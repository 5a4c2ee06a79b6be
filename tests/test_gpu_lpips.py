"""LPIPS on the GPU (mtgs_amd/lpips.py, csrc/lpips.hip) against the fp64 restatement of tests/lpips_refs.py.

(1) lpips_conv alone, every layer configuration at the smallest inputs that reach it and at the M edges of its 32-row MFMA tiles,
    per element within the DERIVED bound |out - ref64| <= 1e-6 (sum |a| |w| + |b|): one k-ordered fp32 fma chain measures 3.5e-7 of
    sum |a b| at K = 4096, the largest K here is 3456;
(2) the first layer's fused input transform (mask, no mask, normalize=False, a masked border column) within the same bound;
(3) lpips_maxpool exactly; the device repack exactly;
(4) the whole metric: e = |kernel - fp64| <= 4 e32 + 1e-7 with e32 = |fp32 CPU restatement - fp64| (the factor covers a different
    but equally valid summation order); exactly 0 for identical images; bitwise reproducible; the same number through image_metrics;
(5) a torch.cuda.graph capture + replay equals eager bitwise (a host synchronisation inside the call would fail the capture);
(6) the errors.
All weights are seeded random ones (lpips_refs.random_weights): there are no trained LPIPS weights here."""
import pytest
import torch

from tests import lpips_refs as R
from tests import util

pytestmark = pytest.mark.gpu

_cache = {}


def _weights():
    """(convs, lins) on the CPU and the LpipsWeights on the device, made once"""
    if "w" not in _cache:
        from mtgs_amd.lpips import LpipsWeights
        convs, lins = R.random_weights(seed=5)
        _cache["w"] = (convs, lins, LpipsWeights.from_tensors(convs, lins, device="cuda"))
    return _cache["w"]


def _nchw64(x):
    return x.permute(0, 3, 1, 2).to(torch.float64)


def _assert_conv(got, x64, w, b, stride, pad, what):
    """got [n, oh, ow, cout] from the device; x64 the fp64 NCHW input.  The derived per-element bound."""
    ref = R.conv(x64, w, b, stride, pad).permute(0, 2, 3, 1)
    bound = 1e-6 * R.conv_bound(x64, w, b, stride, pad).permute(0, 2, 3, 1)
    assert tuple(got.shape) == tuple(ref.shape), what
    err = (got.cpu().to(torch.float64) - ref).abs()
    worst = float((err / bound).max())
    print(f"{what}: max |out - ref64| / (sum |a||w| + |b|) = {worst * 1e-6:.3g}")
    assert bool((err <= bound).all()), f"{what}: {worst * 1e-6:.3g} of sum |a||w| + |b| > 1e-6"
    assert float(ref.max()) > 0 and float(ref.min()) == 0, what          # the ReLU cut something, and not everything


# (layer, n images, h, w): the issue's cases, then output width 1, M exactly 32, M = 33
CONV_CASES = [(0, 2, 35, 47), (1, 2, 3, 5), (1, 2, 7, 7), (2, 2, 1, 2), (2, 2, 4, 5), (3, 2, 1, 2), (3, 2, 4, 5), (4, 2, 1, 2), (4, 2, 4, 5),
              (2, 2, 5, 1), (3, 2, 4, 4), (4, 1, 3, 11), (4, 3, 1, 11)]


@pytest.mark.parametrize("layer,n,h,w", CONV_CASES)
def test_conv_alone(layer, n, h, w):
    from mtgs_amd.lpips import conv2d_nhwc
    convs, _, dev = _weights()
    cin, cout, k, stride, pad, _ = R.LAYERS[layer]
    g = torch.Generator().manual_seed(100 * layer + h * 7 + w)
    x = torch.randn(n, h, w, cin, generator=g)
    packed, bias, _ = dev.layer(layer)
    got = conv2d_nhwc(x.cuda(), packed, bias, k, stride, pad)
    M = got.shape[0] * got.shape[1] * got.shape[2]
    if (layer, n, h, w) == (0, 2, 35, 47):
        assert M == 176
    if (layer, n, h, w) == (3, 2, 4, 4):
        assert M == 32
    if (layer, h, w) == (4, 3, 11) or (layer, h, w) == (4, 1, 11):
        assert M == 33
    if (layer, h, w) == (2, 5, 1):
        assert got.shape[2] == 1
    _assert_conv(got, _nchw64(x), *convs[layer], stride, pad, f"conv{layer + 1} on {n} x {h} x {w}")


@pytest.mark.parametrize("cin", [8, 32])
@pytest.mark.parametrize("cout", [32, 96])
def test_conv_with_a_half_empty_last_column_tile(cout, cin):
    """cout is a multiple of 32 only: the last 64-column tile holds 32 columns, which no AlexNet layer reaches (every cout there is a
    multiple of 64).  cin = 8 takes the scalar loader (K = 72: the last K-step is partly zero-filled), cin = 32 the vector loader."""
    from mtgs_amd.lpips import conv2d_nhwc, repack_conv_weight
    g = torch.Generator().manual_seed(1000 * cout + cin)
    w, b = torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5, 0.1 * torch.randn(cout, generator=g)
    x = torch.randn(1, 3, 5, cin, generator=g)
    got = conv2d_nhwc(x.cuda(), repack_conv_weight(w).cuda(), b.cuda(), 3, 1, 1)
    assert got.shape == (1, 3, 5, cout)
    _assert_conv(got, _nchw64(x), w, b, 1, 1, f"3x3 conv {cin} -> {cout} on 1 x 3 x 5")


def test_conv_without_relu_and_misaligned_input():
    """relu=False keeps the negative outputs; an input that is not 16-byte aligned takes the scalar loader and gives the same bits"""
    from mtgs_amd.lpips import conv2d_nhwc
    convs, _, dev = _weights()
    cin, cout, k, stride, pad, _ = R.LAYERS[1]
    x = torch.randn(2, 7, 7, cin, generator=torch.Generator().manual_seed(9))
    packed, bias, _ = dev.layer(1)
    got = conv2d_nhwc(x.cuda(), packed, bias, k, stride, pad, relu=False)
    ref = R.conv(_nchw64(x), *convs[1], stride, pad, relu=False).permute(0, 2, 3, 1)
    bound = 1e-6 * R.conv_bound(_nchw64(x), *convs[1], stride, pad).permute(0, 2, 3, 1)
    assert bool(((got.cpu().double() - ref).abs() <= bound).all()) and float(got.min()) < 0
    shifted = torch.empty(x.numel() + 1, device="cuda")[1:]
    shifted.copy_(x.reshape(-1))
    assert shifted.data_ptr() % 16 == 4
    assert torch.equal(conv2d_nhwc(shifted.view(x.shape), packed, bias, k, stride, pad, relu=False), got)


@pytest.mark.parametrize("case", ["mask", "no_mask", "not_normalized", "border_column"])
def test_first_layer_fuses_the_input_transform(case):
    """Padding taps contribute ZERO (the scaled tensor is what is padded), and a masked pixel is 0 BEFORE 2x - 1, so it enters as
    (-1 - shift) / scale: a masked column at the image border sits next to the padding and tells the two apart."""
    from mtgs_amd.lpips import conv_first
    convs, _, dev = _weights()
    H, W = 35, 47
    pred, gt, mask = R.images(H, W, seed=21, masked=(case == "mask"))
    normalize = case != "not_normalized"
    if case == "not_normalized":
        pred, gt = 2 * pred - 1, 2 * gt - 1
    if case == "border_column":
        mask = torch.ones(H, W, 1, dtype=torch.bool)
        mask[:, 0] = False
    packed, bias, _ = dev.layer(0)
    got = conv_first(pred.cuda(), gt.cuda(), None if mask is None else mask.cuda(), packed, bias, normalize=normalize)
    x64 = torch.cat([R.transform(pred, mask, normalize), R.transform(gt, mask, normalize)])
    _assert_conv(got, x64, *convs[0], 4, 2, f"first layer, {case}")
    if case == "mask":                      # a uint8 mask is read as the bool one
        assert torch.equal(conv_first(pred.cuda(), gt.cuda(), mask.cuda().to(torch.uint8) * 255, packed, bias), got)


@pytest.mark.parametrize("h,w", [(7, 7), (8, 11), (3, 3)])
def test_maxpool_is_exact(h, w):
    from mtgs_amd.lpips import maxpool_nhwc
    x = torch.randn(2, h, w, 64, generator=torch.Generator().manual_seed(h * w))
    ref = torch.nn.functional.max_pool2d(x.permute(0, 3, 1, 2), 3, 2).permute(0, 2, 3, 1)
    assert torch.equal(maxpool_nhwc(x.cuda()).cpu(), ref)


def test_device_repack_equals_the_host_one():
    from mtgs_amd.lpips import repack_conv_weight
    for cout, cin, kh, kw in ((64, 3, 11, 11), (32, 5, 3, 2)):
        w = torch.randn(cout, cin, kh, kw, generator=torch.Generator().manual_seed(cout))
        assert torch.equal(repack_conv_weight(w.cuda()).cpu(), repack_conv_weight(w))


WHOLE = [(31, 31, False), (35, 47, False), (64, 96, False), (67, 131, True), (128, 228, False)]


@pytest.mark.parametrize("norm", ["torchmetrics", "lpips"])
@pytest.mark.parametrize("H,W,masked", WHOLE)
def test_whole_metric(H, W, masked, norm):
    """e <= 4 e32 + 1e-7, both recorded in the parity report."""
    from mtgs_amd.lpips import lpips
    convs, lins, dev = _weights()
    pred, gt, mask = R.images(H, W, seed=H + W, masked=masked)
    key = ("ref", H, W)
    ref64 = R.lpips_ref(pred, gt, mask, convs, lins, norm=norm)
    ref32 = R.lpips_ref(pred, gt, mask, convs, lins, norm=norm, dtype=torch.float32)
    got = lpips(pred.cuda(), gt.cuda(), None if mask is None else mask.cuda(), weights=dev, norm=norm)
    assert got.dim() == 0 and got.dtype == torch.float32 and got.is_cuda, key
    e, e32 = abs(float(got.double()) - ref64), abs(ref32 - ref64)
    print(f"lpips {H}x{W} {norm}: value {ref64:.9g} e = {e:.3g} e32 = {e32:.3g}")
    util.REPORT.append({"kind": "lpips", "case": f"{H}x{W}{'_masked' if masked else ''}_{norm}", "value": ref64, "e": e, "e32": e32})
    assert ref64 > 1e-3
    assert e <= 4 * e32 + 1e-7, f"e = {e:.3g} > 4 * {e32:.3g} + 1e-7"


def test_identical_images_give_exactly_zero_and_calls_repeat_bitwise():
    from mtgs_amd.lpips import lpips
    _, _, dev = _weights()
    pred, gt, mask = (t.cuda() for t in R.images(67, 131, seed=3, masked=True))
    for norm in ("torchmetrics", "lpips"):
        assert lpips(pred, pred.clone(), mask, weights=dev, norm=norm).item() == 0.0
        assert lpips(pred, gt, torch.zeros_like(mask), weights=dev, norm=norm).item() == 0.0     # all masked: two constant images
        a, b = lpips(pred, gt, mask, weights=dev, norm=norm), lpips(pred, gt, mask, weights=dev, norm=norm)
        assert a.view(torch.int32).item() == b.view(torch.int32).item() and a.item() > 0
    assert lpips(pred, gt, mask, weights=dev, norm="torchmetrics").item() != lpips(pred, gt, None, weights=dev).item()
    assert lpips(2 * pred - 1, 2 * gt - 1, None, weights=dev, normalize=False).item() > 0


def test_the_scratch_is_per_stream():
    """The metric on the default stream and on two others, one call at a time: the results are bitwise equal, and each stream has a
    scratch tensor of its own (mtgs_amd._lib.scratch keys on the stream), allocated once."""
    from mtgs_amd import _lib
    from mtgs_amd.lpips import lpips
    _, _, dev = _weights()
    pred, gt, mask = (t.cuda() for t in R.images(31, 31, seed=4, masked=True))
    torch.cuda.synchronize()
    results, scratches = [], []

    def run(stream):
        with torch.cuda.stream(stream):
            out = lpips(pred, gt, mask, weights=dev)
        torch.cuda.synchronize()
        results.append(out.view(torch.int32).item())
        scratches.append(_lib.scratch(("lpips", 31, 31), lambda: pytest.fail("the call left no scratch for its stream"), pred.device, stream.cuda_stream))

    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    for stream in (torch.cuda.current_stream(), a, b):
        run(stream)
    assert results[0] == results[1] == results[2]
    assert len({t.data_ptr() for t in scratches}) == 3 and all(t.numel() > 0 and t.dtype == torch.uint8 for t in scratches)
    entries = len(_lib._scratch)
    run(a)
    assert scratches[3] is scratches[1] and len(_lib._scratch) == entries and results[3] == results[0]


def test_image_metrics_gains_the_key_and_keeps_the_others():
    from mtgs_amd import image_metrics
    from mtgs_amd.metrics import lpips
    _, _, dev = _weights()
    pred, gt, mask = (t.cuda() for t in R.images(64, 96, seed=8, masked=True))
    depth, lidar = 1 + 40 * torch.rand(64, 96, 1, device="cuda"), 1 + 40 * torch.rand(64, 96, 1, device="cuda")
    plain = image_metrics(pred, gt, mask, pred_depth=depth, lidar_depth=lidar)
    more = image_metrics(pred, gt, mask, pred_depth=depth, lidar_depth=lidar, lpips_weights=dev)
    assert "lpips" not in plain and sorted(more) == sorted(list(plain) + ["lpips"])
    for k in plain:
        assert plain[k].view(torch.int32).item() == more[k].view(torch.int32).item(), k
    assert more["lpips"].view(torch.int32).item() == lpips(pred, gt, mask, weights=dev).view(torch.int32).item()


def test_lpips_captures_in_a_graph():
    """One stream, no parallel branches; replayed on rewritten image values the result equals the eager one bitwise."""
    from mtgs_amd.lpips import lpips
    _, _, dev = _weights()
    H, W = 67, 131
    first = [t.cuda() for t in R.images(H, W, seed=11, masked=True)]
    second = [t.cuda() for t in R.images(H, W, seed=12, masked=True)]
    static = [t.clone() for t in first]

    def step():
        return lpips(static[0], static[1], static[2], weights=dev)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                              # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    seen = []
    for src in (second, first):
        for dst, t in zip(static, src):
            dst.copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        eager = lpips(src[0], src[1], src[2], weights=dev)
        assert out.view(torch.int32).item() == eager.view(torch.int32).item()
        seen.append(out.item())
    assert seen[0] != seen[1]


def test_errors():
    from mtgs_amd.lpips import LpipsWeights, conv2d_nhwc, lpips
    convs, lins, dev = _weights()
    img = torch.rand(30, 30, 3, device="cuda")
    with pytest.raises(ValueError, match="30 x 30 image leaves no pixel after the second pool"):
        lpips(img, img, weights=dev)
    with pytest.raises(ValueError, match="second pool"):
        lpips(torch.rand(64, 30, 3, device="cuda"), torch.rand(64, 30, 3, device="cuda"), weights=dev)
    rgba = torch.rand(40, 40, 4, device="cuda")
    with pytest.raises(NotImplementedError, match="4 channels"):
        lpips(rgba, rgba, weights=dev)
    narrow = [(convs[0][0][:48].cuda(), convs[0][1][:48].cuda())] + [(w.cuda(), b.cuda()) for w, b in convs[1:]]
    with pytest.raises(NotImplementedError, match="cout = 48"):
        LpipsWeights.from_tensors(narrow, lins)
    with pytest.raises(NotImplementedError, match="cout = 48"):
        conv2d_nhwc(torch.rand(2, 4, 4, 16, device="cuda"), torch.rand(9 * 16, 48, device="cuda"), torch.rand(48, device="cuda"), 3, 1, 1)
    good = torch.rand(40, 40, 3, device="cuda")
    needs = torch.rand(40, 40, 3, device="cuda").requires_grad_(True)
    with pytest.raises(RuntimeError, match="requires grad"):
        lpips(needs, good, weights=dev)
    with torch.no_grad():
        assert lpips(needs, good, weights=dev).item() > 0
    with pytest.raises(ValueError, match="norm must be"):
        lpips(good, good, weights=dev, norm="l2")
    with pytest.raises(RuntimeError, match="weights are on cpu"):
        lpips(good, good, weights=LpipsWeights.from_tensors(convs, lins))
    with pytest.raises(ValueError, match="same shape"):
        lpips(good, torch.rand(40, 41, 3, device="cuda"), weights=dev)
