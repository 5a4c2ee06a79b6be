"""A restatement of LPIPS with the AlexNet backbone in torch.nn.functional, on the CPU, in fp64 (or any dtype given): the reference of
tests/test_lpips_host.py and tests/test_gpu_lpips.py.

[RECALL] Every line of the definition is recalled -- torchmetrics, torchvision and the lpips package were not available to run:
the scaling layer's constants, AlexNet's five convolutions and two pools, one tap after each ReLU, the unit normalisation of each
pixel's channel vector, the squared difference weighted by a learned non-negative `lin` vector, the spatial mean and the sum over
the taps.  The normalisation has two published forms: norm="torchmetrics" x / sqrt(1e-8 + sum x^2) (recalled as torchmetrics' form,
NOT checked) and norm="lpips" x / (sqrt(sum x^2) + 1e-10) (the original package's).

There are no trained weights here: random_weights() draws seeded ones, convolutions scaled by 1 / sqrt(K) so that activations
neither die nor explode, and non-negative lin vectors as in the trained metric.
"""
import math

import torch
import torch.nn.functional as F

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .449, .450)
# (cin, cout, kernel, stride, pad, max-pool 3x3 stride 2 before it)
LAYERS = ((3, 64, 11, 4, 2, False), (64, 192, 5, 1, 2, True), (192, 384, 3, 1, 1, True), (384, 256, 3, 1, 1, False), (256, 256, 3, 1, 1, False))
EPS = {"torchmetrics": 1e-8, "lpips": 1e-10}


def random_weights(seed=0, layers=LAYERS):
    """(convs, lins): fp32 CPU tensors, [(w [cout, cin, k, k], b [cout])] and [v [cout] >= 0]"""
    g = torch.Generator().manual_seed(seed)
    convs, lins = [], []
    for cin, cout, k, *_ in layers:
        K = cin * k * k
        convs.append((torch.randn(cout, cin, k, k, generator=g) / math.sqrt(K), 0.1 * torch.randn(cout, generator=g)))
        lins.append(torch.rand(cout, generator=g))
    return convs, lins


def transform(img, mask=None, normalize=True, dtype=torch.float64):
    """[RECALL] steps 1-2: [H, W, 3] -> the scaled [1, 3, H, W] tensor the first convolution pads with zeros.  A masked pixel is 0
    BEFORE 2x - 1."""
    x = img.to(dtype)
    if mask is not None:
        x = x * (mask.reshape(img.shape[0], img.shape[1], 1) != 0).to(dtype)
    if normalize:
        x = 2 * x - 1
    x = (x - torch.tensor(SHIFT, dtype=dtype)) / torch.tensor(SCALE, dtype=dtype)
    return x.permute(2, 0, 1)[None]


def conv(x, w, b, stride, pad, relu=True):
    y = F.conv2d(x, w.to(x.dtype), None if b is None else b.to(x.dtype), stride=stride, padding=pad)
    return F.relu(y) if relu else y


def conv_bound(x, w, b, stride, pad):
    """sum |a| |w| + |b| per output element: the scale of the derived error bound of one k-ordered fp32 fma chain"""
    return F.conv2d(x.abs(), w.to(x.dtype).abs(), b.to(x.dtype).abs(), stride=stride, padding=pad)


def taps(x, convs, layers=LAYERS):
    """[RECALL] step 3: the five activations, each after its ReLU; x is [N, 3, H, W]"""
    out = []
    for (w, b), (_, _, _, stride, pad, pool) in zip(convs, layers):
        if pool:
            x = F.max_pool2d(x, 3, 2)
        x = conv(x, w, b, stride, pad)
        out.append(x)
    return out


def unit(x, norm):
    """[RECALL] the two published forms of the channel normalisation of [N, C, h, w]"""
    s = (x * x).sum(dim=1, keepdim=True)
    if norm == "torchmetrics":
        return x / torch.sqrt(EPS[norm] + s)
    if norm == "lpips":
        return x / (torch.sqrt(s) + EPS[norm])
    raise ValueError(norm)


def lpips_ref(pred, gt, mask, convs, lins, normalize=True, norm="torchmetrics", dtype=torch.float64):
    """[RECALL] the whole metric, as a Python float"""
    t0 = taps(transform(pred, mask, normalize, dtype), convs)
    t1 = taps(transform(gt, mask, normalize, dtype), convs)
    total = 0.0
    for a, b, v in zip(t0, t1, lins):
        d = (unit(a, norm) - unit(b, norm)) ** 2
        total = total + (d * v.to(dtype).reshape(1, -1, 1, 1)).sum(dim=1).mean()
    return float(total)


def images(H, W, seed, masked=False):
    """two related fp32 images in [0, 1] and, if asked, a random bool mask [H, W, 1]"""
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(H, W, 3, generator=g)
    pred = (gt + 0.2 * torch.randn(H, W, 3, generator=g)).clamp(0, 1)
    mask = (torch.rand(H, W, 1, generator=g) > 0.3) if masked else None
    return pred, gt, mask
