"""The LPIPS metric with the AlexNet backbone on the device (include/mtgs_lpips.h, csrc/lpips.hip): what
LearnedPerceptualImagePatchSimilarity(normalize=True) computes on `gt * mask` and `pred * mask` in mtgs_scene_graph.py's
get_metrics_dict on every training step and for every evaluation image.

    w = LpipsWeights.from_module(torchmetrics_lpips_module)          # or from_tensors(convs=[(w, b)] * 5, lins=[v] * 5); once
    d = lpips(pred, gt, mask, weights=w)                             # 0-dim fp32 device tensor; float(d) is the caller's choice
    image_metrics(pred, gt, mask, lpips_weights=w)["lpips"]          # the same number under MTGS's key

Forward only, no host read (graph-capturable), no atomics (bitwise reproducible).  Five convolutions as implicit GEMMs on exact-f32
MFMA with bias and ReLU in the epilogue (the first reads the images and the mask and applies the input transform on load), two
max-pools, one fused launch per tap for the channel norms, the weighted squared difference and the spatial sum, one launch for the
result.

[RECALL] The definition is recalled (include/mtgs_lpips.h states it; tests/lpips_refs.py restates it in fp64): neither torchmetrics
nor the lpips package was available to check it against.  In particular the DEFAULT normalisation, norm="torchmetrics"
(x / sqrt(1e-8 + sum x^2)), is recalled as torchmetrics' form and could not be checked; norm="lpips" is the original package's
x / (sqrt(sum x^2) + 1e-10).  The two differ (by about 1e-8 relative on ordinary features, more on near-zero ones).
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch
from torch import Tensor

from ._inputs import as_f32, image_pair
from ._lib import call, ptr, require_gpu, scratch, size_query, stream_of

# (cin, cout, kernel, stride, pad, a 3x3 stride-2 max-pool before it): AlexNet's features, every convolution followed by a ReLU and a tap
LAYERS = ((3, 64, 11, 4, 2, False), (64, 192, 5, 1, 2, True), (192, 384, 3, 1, 1, True), (384, 256, 3, 1, 1, False), (256, 256, 3, 1, 1, False))
MIN_SIDE = 31
NORMS = {"torchmetrics": 0, "lpips": 1}


def _conv_out(n: int, k: int, stride: int, pad: int) -> int:
    return (n + 2 * pad - k) // stride + 1 if n + 2 * pad >= k else 0


def _pool_out(n: int) -> int:
    return (n - 3) // 2 + 1 if n >= 3 else 0


def tap_sizes(H: int, W: int) -> List[Tuple[int, int]]:
    """(h, w) of the five taps of an H x W image; a side of 0 means the image is too small."""
    h, w, out = H, W, []
    for _, _, k, stride, pad, pool in LAYERS:
        if pool:
            h, w = _pool_out(h), _pool_out(w)
        h, w = _conv_out(h, k, stride, pad), _conv_out(w, k, stride, pad)
        out.append((h, w))
    return out


def repack_conv_weight(w: Tensor) -> Tensor:
    """torch's [cout, cin, kh, kw] as the [K, cout] array the convolution reads, K = kh * kw * cin in the order (kh, kw, cin)."""
    cout, cin, kh, kw = w.shape
    if w.is_cuda:
        src = as_f32(w)
        out = torch.empty(kh * kw * cin, cout, dtype=torch.float32, device=w.device)
        call("mtgs_lpips_repack", cout, cin, kh, kw, ptr(src), ptr(out), stream_of(src))
        return out
    return w.detach().to(torch.float32).permute(2, 3, 1, 0).reshape(kh * kw * cin, cout).contiguous()


def unpack_conv_weight(packed: Tensor, cin: int, kh: int, kw: int) -> Tensor:
    """The inverse of repack_conv_weight."""
    K, cout = packed.shape
    if K != kh * kw * cin:
        raise ValueError(f"packed weights have K = {K}, not {kh} * {kw} * {cin}")
    return packed.reshape(kh, kw, cin, cout).permute(3, 2, 0, 1).contiguous()


class LpipsWeights:
    """One weight set, repacked once: `flat` is the array mtgs_lpips reads (per layer: packed weights [K, cout], bias, lin)."""

    def __init__(self, flat: Tensor):
        self.flat = flat

    @property
    def device(self):
        return self.flat.device

    def to(self, device) -> "LpipsWeights":
        return LpipsWeights(self.flat.to(device))

    def layer(self, i: int) -> Tuple[Tensor, Tensor, Tensor]:
        """(packed [K, cout], bias [cout], lin [cout]) of layer i, as views of `flat`."""
        o = 0
        for cin, cout, k, *_ in LAYERS[:i]:
            o += k * k * cin * cout + 2 * cout
        cin, cout, k, *_ = LAYERS[i]
        K = k * k * cin
        return self.flat[o:o + K * cout].view(K, cout), self.flat[o + K * cout:o + (K + 1) * cout], self.flat[o + (K + 1) * cout:o + (K + 2) * cout]

    @classmethod
    def from_tensors(cls, convs: Sequence[Tuple[Tensor, Tensor]], lins: Sequence[Tensor], device=None) -> "LpipsWeights":
        """convs: five (weight [cout, cin, kh, kw], bias [cout]) in network order; lins: five vectors of cout elements (any shape
        with that many elements, as a 1x1 convolution's [1, cout, 1, 1])."""
        convs, lins = list(convs), list(lins)
        if len(convs) != len(LAYERS) or len(lins) != len(LAYERS):
            raise ValueError(f"LPIPS (AlexNet) takes {len(LAYERS)} convolutions and {len(LAYERS)} lin vectors, got {len(convs)} and {len(lins)}")
        parts = []
        for i, ((w, b), v, (cin, cout, k, *_)) in enumerate(zip(convs, lins, LAYERS)):
            if w.dim() != 4:
                raise ValueError(f"convolution {i}: weight must be [cout, cin, kh, kw], got {tuple(w.shape)}")
            if w.shape[0] % 32 != 0:
                raise NotImplementedError(f"convolution {i}: cout = {w.shape[0]} is not a multiple of 32")
            if tuple(w.shape) != (cout, cin, k, k):
                raise ValueError(f"convolution {i}: weight {tuple(w.shape)} is not AlexNet's {(cout, cin, k, k)}")
            if b is None or tuple(b.shape) != (cout,):
                raise ValueError(f"convolution {i}: bias must be [{cout}], got {None if b is None else tuple(b.shape)}")
            if v.numel() != cout:
                raise ValueError(f"lin {i}: {v.numel()} elements for {cout} channels (shape {tuple(v.shape)})")
            parts += [repack_conv_weight(w).reshape(-1), b.detach().to(torch.float32).reshape(-1), v.detach().to(torch.float32).reshape(-1)]
        flat = torch.cat([p.to(parts[0].device) for p in parts]).contiguous()
        return cls(flat if device is None else flat.to(device))

    @classmethod
    def from_module(cls, module: torch.nn.Module, device=None) -> "LpipsWeights":
        """Walks `module` in definition order: the Conv2d with a bias are the backbone, the bias-free 1x1 Conv2d the lin layers.
        No checkpoint key names are assumed, so a torchmetrics or lpips module is handed over as it is."""
        convs, lins = [], []
        for m in module.modules():
            if isinstance(m, torch.nn.Conv2d):
                if m.bias is None and tuple(m.kernel_size) == (1, 1):
                    lins.append(m.weight)
                else:
                    convs.append((m.weight, m.bias))
        if len(convs) != len(LAYERS) or len(lins) != len(LAYERS):
            raise ValueError(f"expected {len(LAYERS)} biased Conv2d and {len(LAYERS)} bias-free 1x1 Conv2d, found {len(convs)} with weights "
                             f"{[tuple(w.shape) for w, _ in convs]} and {len(lins)} with weights {[tuple(v.shape) for v in lins]}")
        return cls.from_tensors(convs, lins, device=device)


def _check_nhwc(x: Tensor) -> Tensor:
    if x.dim() != 4 or x.shape[0] < 1:
        raise ValueError(f"activations must be [n, h, w, c], got {tuple(x.shape)}")
    require_gpu(x)
    return as_f32(x)


def conv2d_nhwc(x: Tensor, packed: Tensor, bias: Tensor, kernel: int, stride: int, pad: int, relu: bool = True) -> Tensor:
    """lpips_conv alone: x [n, h, w, cin], packed [kernel * kernel * cin, cout] -> [n, oh, ow, cout] (n = 2 inside the metric)."""
    x = _check_nhwc(x)
    n, h, w, cin = x.shape
    cout = packed.shape[1]
    if cout % 32 != 0:
        raise NotImplementedError(f"cout = {cout} is not a multiple of 32")
    if packed.shape[0] != kernel * kernel * cin:
        raise ValueError(f"packed weights have K = {packed.shape[0]}, not {kernel} * {kernel} * {cin}")
    require_gpu(packed, bias)
    out = torch.empty(n, _conv_out(h, kernel, stride, pad), _conv_out(w, kernel, stride, pad), cout, dtype=torch.float32, device=x.device)
    call("mtgs_lpips_conv", n, h, w, cin, cout, kernel, kernel, stride, pad, ptr(x), ptr(packed.contiguous()), ptr(bias.contiguous()),
         int(relu), ptr(out), stream_of(x))
    return out


def conv_first(pred: Tensor, gt: Tensor, mask: Optional[Tensor], packed: Tensor, bias: Tensor, *, normalize: bool = True,
               kernel: int = 11, stride: int = 4, pad: int = 2, relu: bool = True) -> Tensor:
    """The first layer's form of lpips_conv alone: the input transform applied on load."""
    pred_c, gt_c, mask_c = image_pair(pred, gt, mask, metric="lpips")
    H, W = pred_c.shape[:2]
    cout = packed.shape[1]
    if cout % 32 != 0:
        raise NotImplementedError(f"cout = {cout} is not a multiple of 32")
    require_gpu(packed, bias)
    out = torch.empty(2, _conv_out(H, kernel, stride, pad), _conv_out(W, kernel, stride, pad), cout, dtype=torch.float32, device=pred_c.device)
    call("mtgs_lpips_conv_first", H, W, ptr(pred_c), ptr(gt_c), ptr(mask_c), int(normalize), cout, kernel, kernel, stride, pad,
         ptr(packed.contiguous()), ptr(bias.contiguous()), int(relu), ptr(out), stream_of(pred_c))
    return out


def maxpool_nhwc(x: Tensor) -> Tensor:
    """lpips_maxpool alone: 3x3, stride 2, no padding, on [n, h, w, c]."""
    x = _check_nhwc(x)
    n, h, w, c = x.shape
    out = torch.empty(n, _pool_out(h), _pool_out(w), c, dtype=torch.float32, device=x.device)
    call("mtgs_lpips_maxpool", n, h, w, c, ptr(x), ptr(out), stream_of(x))
    return out


def lpips(pred: Tensor, gt: Tensor, mask: Optional[Tensor] = None, *, weights: LpipsWeights, normalize: bool = True,
          norm: str = "torchmetrics") -> Tensor:
    """LPIPS (AlexNet) of pred * mask and gt * mask, [H, W, 3] images in [0, 1] (normalize=True) or [-1, 1] (False), the mask
    [H, W, 1] or [H, W] bool or uint8 (non-zero keeps the pixel).  Returns a 0-dim fp32 tensor on the images' device.
    [RECALL] norm: "torchmetrics" (the default; x / sqrt(1e-8 + sum x^2), recalled, not checked against torchmetrics here) or
    "lpips" (x / (sqrt(sum x^2) + 1e-10), the original package's).  The workspace is kept per (device, stream, H, W)."""
    if norm not in NORMS:
        raise ValueError(f"norm must be one of {sorted(NORMS)}, got {norm!r}")
    pred_c, gt_c, mask_c = image_pair(pred, gt, mask, metric="lpips")
    H, W = pred_c.shape[:2]
    if H < MIN_SIDE or W < MIN_SIDE:
        raise ValueError(f"a {H} x {W} image leaves no pixel after the second pool: both sides must be >= {MIN_SIDE}")
    if weights.device != pred_c.device:
        raise RuntimeError(f"weights are on {weights.device}, the images on {pred_c.device}: move them once with weights.to(device)")
    stream = stream_of(pred_c)
    ws = scratch(("lpips", H, W), lambda: size_query("mtgs_lpips_workspace_bytes", H, W), pred_c.device, stream)
    out = torch.empty((), dtype=torch.float32, device=pred_c.device)
    call("mtgs_lpips", H, W, ptr(pred_c), ptr(gt_c), ptr(mask_c), ptr(weights.flat), int(normalize), NORMS[norm], ptr(out), ptr(ws),
         ws.numel(), stream)
    return out


__all__ = ["LpipsWeights", "lpips", "tap_sizes", "repack_conv_weight", "unpack_conv_weight", "LAYERS", "MIN_SIDE"]
