#!/usr/bin/env python3
"""The geometric loss terms of the shipped configs, forward + backward per call, on one device:

    normal  MTGS's depth-supervised "Normal Loss" (mtgs_scene_graph.py:912-935) at 960x540 and 1920x1080
    scale   the "2D reg" and "Sharp Shape Reg" terms (:937-940, :969-981, two_d_gaussians) at 2M Gaussians

each in four forms:

    torch        the reference's expressions restated in PyTorch for this script: the target normal from the depth through
                 the back-projection, the cross product, normalize, the flip and (1 + n) / 2 with the intrinsics read by .item()
                 and the loss over a boolean-mask selection; torch.min / torch.sort / torch.maximum for the scale terms
    torch_graph  the same in a torch.cuda.graph: the intrinsics and the flip made before the capture and the boolean selection written
                 as a masked sum over the selected count (the reference's form cannot be captured)
    eager        mtgs_amd.loss.depth_normal_loss / scale_regularizers
    graph        the same captured once and replayed

Device events around each call, median of --steps after --warmup; for the device ops the forward alone is timed too.
Prints one JSON line per term, size and form (--out FILE also writes them).

--kernel-stats CSV (the kernel_stats.csv of `rocprofv3 --kernel-trace --stats -- python scripts/geom_loss_bench.py --sizes WxH`,
one size per run) prints, per kernel, the HBM bytes it moves divided by its mean time: normal 17 B/px forward (pred 12, depth 4,
mask 1) and 29 B/px backward (+ the 12 B/px gradient); scale 12 B/row forward and 24 B/row backward."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def normal_inputs(H, W, seed=0, dev="cuda"):
    g = torch.Generator().manual_seed(seed)
    v = torch.arange(H, dtype=torch.float64)[:, None] + 0.5
    u = torch.arange(W, dtype=torch.float64)[None, :] + 0.5
    ground = 1.28 * W / torch.clamp(v - H / 2, min=1e-3)
    facade = 12.0 + 4.0 * torch.sin(u / W * 9.0) + 2.0 * ((u / W * 7).floor() % 2)
    depth = torch.where(v > H / 2 + 2, torch.minimum(ground, facade + 50), facade)
    depth = (depth + 0.002 * torch.rand(H, W, generator=g, dtype=torch.float64)).float()[..., None]
    K = torch.tensor([[0.8 * W, 0.0, W / 2.0], [0.0, 0.8 * W, H / 2.0], [0.0, 0.0, 1.0]])
    pred = torch.rand(H, W, 3, generator=g)
    mask = torch.ones(H, W, 1, dtype=torch.bool)
    mask[: H // 8] = False
    return depth.to(dev), K.to(dev), pred.to(dev).requires_grad_(True), mask.to(dev)


def torch_target(depth, fx, fy, cx, cy, flip=None):
    H, W = depth.shape[:2]
    d = depth.float().reshape(H, W)
    u = torch.arange(W, device=d.device, dtype=torch.float32)[None, :] + 0.5
    v = torch.arange(H, device=d.device, dtype=torch.float32)[:, None] + 0.5
    P = torch.stack([(u - cx) * d / fx, (v - cy) * d / fy, d], dim=-1)
    a = P[1:-1, 2:] - P[1:-1, :-2]
    b = P[:-2, 1:-1] - P[2:, 1:-1]
    n = torch.nn.functional.normalize(torch.cross(a, b, dim=-1), p=2, dim=-1)
    n = torch.nn.functional.pad(n.permute(2, 0, 1), (1, 1, 1, 1), mode="constant").permute(1, 2, 0)
    n = n @ torch.diag(n.new_tensor([1, -1, -1]) if flip is None else flip)
    return (1 + n) / 2


def tv(pred):
    return torch.mean(torch.abs(pred[:, :-1] - pred[:, 1:])) + torch.mean(torch.abs(pred[:-1] - pred[1:]))


def torch_normal_loss(pred, depth, K, mask):
    """the reference's form: host reads of the intrinsics, boolean-mask selection"""
    fx, fy, cx, cy = K[0, 0].item(), K[1, 1].item(), K[0, 2].item(), K[1, 2].item()
    gt = torch_target(depth.detach(), fx, fy, cx, cy)
    m = ((depth > 0.1) & (depth < 50) & mask).squeeze(-1)
    return torch.abs(gt - pred)[m].mean() + tv(pred)


def torch_normal_loss_capturable(pred, depth, intr, mask, flip):
    gt = torch_target(depth.detach(), *intr, flip=flip)
    m = ((depth > 0.1) & (depth < 50) & mask).float()
    return (torch.abs(gt - pred) * m).sum() / (3 * m.sum()) + tv(pred)


def torch_scale_terms(s):
    two = torch.min(s, dim=1, keepdim=True)[0].mean()
    srt, _ = torch.sort(s, dim=-1, descending=True)
    sharp = (torch.maximum(srt[..., 0] / srt[..., 1], torch.tensor(10.0)) - 10.0).mean()
    return two + sharp


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    dev_ms, wall_ms = [], []
    for _ in range(steps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        wall_ms.append((time.perf_counter() - t0) * 1e3)
        dev_ms.append(s.elapsed_time(e))
    return {"ms_median": round(statistics.median(dev_ms), 4), "ms_min": round(min(dev_ms), 4), "ms_max": round(max(dev_ms), 4),
            "wall_ms_median": round(statistics.median(wall_ms), 4)}


def graphed(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    return g, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="960x540,1920x1080")
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--forms", default="torch,torch_graph,eager,graph")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
    if a.kernel_stats:
        return kernel_bandwidth(a)
    from mtgs_amd.loss import depth_normal_loss, scale_regularizers
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    for size in a.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        depth, K, pred, mask = normal_inputs(H, W)
        intr = (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))
        flip = torch.tensor([1.0, -1.0, -1.0], device=depth.device)      # (a host-to-device copy cannot be captured)
        for form in a.forms.split(","):
            rec = {"term": "normal", "form": form, "width": W, "height": H, "steps": a.steps}
            if form == "torch":
                step = lambda: torch.autograd.grad(torch_normal_loss(pred, depth, K, mask), pred)        # noqa: E731
            elif form == "torch_graph":
                step = graphed(lambda: torch.autograd.grad(torch_normal_loss_capturable(pred, depth, intr, mask, flip), pred))[0].replay
            elif form == "eager":
                step = lambda: torch.autograd.grad(depth_normal_loss(pred, depth, K, mask), pred)       # noqa: E731
                fwd = timed(lambda: depth_normal_loss(pred, depth, K, mask), a.steps, a.warmup)
                rec["fwd_ms_median"] = fwd["ms_median"]
            else:
                step = graphed(lambda: torch.autograd.grad(depth_normal_loss(pred, depth, K, mask), pred))[0].replay
                gf = graphed(lambda: depth_normal_loss(pred, depth, K, mask))[0]
                rec["fwd_ms_median"] = timed(gf.replay, a.steps, a.warmup)["ms_median"]
            rec.update(timed(step, a.steps, a.warmup))
            emit(rec)
        loss = float(depth_normal_loss(pred, depth, K, mask).detach())
        ref = float(torch_normal_loss(pred, depth, K, mask))
        emit({"term": "normal", "check": True, "width": W, "height": H, "device": loss, "torch": ref})

    N = a.rows
    g = torch.Generator().manual_seed(1)
    s = torch.exp(0.8 * torch.randn(N, 3, generator=g))
    s[::3, 0] *= 30.0
    s = s.cuda().requires_grad_(True)

    def ops():
        two, sharp = scale_regularizers(s)
        return two + sharp
    for form in a.forms.split(","):
        rec = {"term": "scale", "form": form, "rows": N, "steps": a.steps}
        if form == "torch":
            step = lambda: torch.autograd.grad(torch_scale_terms(s), s)      # noqa: E731
        elif form == "torch_graph":
            step = graphed(lambda: torch.autograd.grad(torch_scale_terms(s), s))[0].replay
        elif form == "eager":
            step = lambda: torch.autograd.grad(ops(), s)                     # noqa: E731
            rec["fwd_ms_median"] = timed(lambda: scale_regularizers(s), a.steps, a.warmup)["ms_median"]
        else:
            step = graphed(lambda: torch.autograd.grad(ops(), s))[0].replay
            rec["fwd_ms_median"] = timed(graphed(lambda: scale_regularizers(s))[0].replay, a.steps, a.warmup)["ms_median"]
        rec.update(timed(step, a.steps, a.warmup))
        emit(rec)
    emit({"term": "scale", "check": True, "rows": N, "device": float(ops()), "torch": float(torch_scale_terms(s))})
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


def kernel_bandwidth(a):
    import csv
    (W, H), N = (int(v) for v in a.sizes.split("x")), a.rows
    per_call = {"normal_loss_fwd_kernel": 17 * W * H, "normal_loss_bwd_kernel": 29 * W * H, "depth_normals_kernel": 16 * W * H,
                "scale_reg_fwd_kernel": 12 * N, "scale_reg_bwd_kernel": 24 * N}
    lines = []
    with open(a.kernel_stats) as f:
        for row in csv.DictReader(f):
            name = row["Name"].replace("(anonymous namespace)::", "").split("(")[0].strip()
            rec = {"kernel": name, "calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 2)}
            if name in per_call:
                rec.update(bytes=per_call[name], GBps=round(per_call[name] / float(row["AverageNs"]), 1),
                           **({"rows": N} if name.startswith("scale") else {"width": W, "height": H}))
            elif "finish" not in name:
                continue
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    if a.out:
        with open(a.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
