#!/usr/bin/env python3
"""The pseudo-depth loss family, forward + backward: the reference's composition as PyTorch runs it on the GPU
(mtgs_scene_graph.py:847-873: the selection, `mask.sum() == 0` on the host, pred[mask] / gt[mask] by boolean indexing, then the
member of mtgs/utils/geometric_loss.py) against mtgs_amd.loss.pseudo_depth_loss, for every kind at 960x540 and 1920x1080.
Alternating rounds, the median of each; one line per size and kind."""
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from mtgs_amd.loss import pseudo_depth_loss  # noqa: E402

dev = torch.device("cuda")
KINDS = ("mse", "L1", "InverseL1", "LogL1", "HuberL1", "EdgeAwareLogL1")


def composition(pred, gt, mask, kind, rgb, thresh=0.2):
    m = (gt > 0.1) & (gt < 50) & mask
    if m.sum() == 0:                                   # (the reference's host read)
        return pred.sum() * 0.0
    if kind == "EdgeAwareLogL1":
        logl1 = torch.log(1 + torch.abs(pred - gt))
        lam_x = torch.exp(-torch.mean(torch.abs(rgb[:, :-1] - rgb[:, 1:]), -1, keepdim=True))
        lam_y = torch.exp(-torch.mean(torch.abs(rgb[:-1] - rgb[1:]), -1, keepdim=True))
        return (lam_x * logl1[:, :-1])[m[:, :-1]].mean() + (lam_y * logl1[:-1])[m[:-1]].mean()
    p, g = pred[m], gt[m]
    if kind == "mse":
        return torch.nn.functional.mse_loss(p, g)
    if kind == "L1":
        return torch.abs(p - g).mean()
    if kind == "InverseL1":
        return torch.abs(1 / (p + 1e-6) - 1 / (g + 1e-6)).mean()
    if kind == "LogL1":
        return torch.log(1 + torch.abs(p - g)).mean()
    l1 = torch.abs(p - g)                              # HuberL1 (its gt != 0 mask is all true inside gt > 0.1)
    d = thresh * torch.max(l1)
    return torch.where(l1 < d, ((p - g) ** 2 + d ** 2) / (2 * d), l1).mean()


def t(fn, reps=50):
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


for H, W in ((540, 960), (1080, 1920)):
    g = torch.Generator().manual_seed(0)
    gt = (torch.rand(H, W, 1, generator=g) * 60.0).to(dev)
    pred = ((gt.cpu() + 2.0 * torch.randn(H, W, 1, generator=g)).abs() + 0.05).to(dev).requires_grad_(True)
    mask = (torch.rand(H, W, 1, generator=g) > 0.2).to(dev)
    rgb = torch.rand(H, W, 3, generator=g).to(dev)
    for kind in KINDS:
        def run(fn):
            pred.grad = None
            fn(pred, gt, mask, kind, rgb).backward()

        torch_step, hip_step = (lambda: run(composition)), (lambda: run(pseudo_depth_loss))
        for _ in range(3):
            torch_step(), hip_step()
        a, b = [], []
        for _ in range(5):
            a.append(t(torch_step))
            b.append(t(hip_step))
        a, b = sorted(a)[2], sorted(b)[2]
        d = abs(float(composition(pred, gt, mask, kind, rgb).detach()) - float(pseudo_depth_loss(pred, gt, mask, kind, rgb).detach()))
        print(f"{W}x{H} {kind:>14}: PyTorch composition {a:.0f} us, pseudo_depth_loss {b:.0f} us ({a / b:.1f}x), "
              f"|difference| {d:.1e}", flush=True)
