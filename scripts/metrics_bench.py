#!/usr/bin/env python3
"""get_metrics_dict's device metrics (psnr, cc_psnr, depth_RMSE / absRel / delta1) per call, on one device, at 960x540 and
1920x1080, for three forms:

    torch   a PyTorch formulation of the same metrics on the device, written for this script from the algorithm (per channel
            torch.linalg.lstsq of the masked quadratic features, one torch.isfinite(w) host read per fit, boolean-mask gathers
            for the PSNRs and the depth errors).  If lstsq raises on the device, the error is recorded instead of a time.
    eager   mtgs_amd.image_metrics
    graph   mtgs_amd.image_metrics captured once in torch.cuda.graph and replayed

Device events around each call, median of --steps after --warmup; `wall_ms` is the host time per call including a synchronize.
Prints one JSON line per form and size (--out FILE also writes them)."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

EPS = 0.5 / 255


def inputs(H, W, seed=0, dev="cuda"):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    gt = torch.stack([0.5 + 0.6 * torch.sin(6 * xx + 2 * yy), 0.5 + 0.5 * torch.cos(5 * yy - 3 * xx * yy), 0.8 * xx], dim=-1)
    gt = (gt + 0.05 * torch.randn(H, W, 3, generator=g)).clamp(0, 1)
    pred = (0.05 + 0.85 * gt + 0.15 * gt * gt + 0.02 * torch.randn(H, W, 3, generator=g)).clamp(0, 1)
    mask = torch.rand(H, W, 1, generator=g) > 0.05
    lidar = torch.where(torch.rand(H, W, 1, generator=g) > 0.7, 1 + 90 * torch.rand(H, W, 1, generator=g), torch.zeros(H, W, 1))
    depth = lidar * (1 + 0.3 * torch.randn(H, W, 1, generator=g)) + 0.5
    return [t.to(dev) for t in (pred, gt, mask, depth, lidar)]


def torch_metrics(pred, gt, mask, depth, lidar, iters=5):
    """The metrics in plain PyTorch ops on the device (not the reference's code; same algorithm)."""
    x = (pred * mask).reshape(-1, 3)
    y = (gt * mask).reshape(-1, 3)
    ok = lambda z: (z >= EPS) & (z <= 1 - EPS)                     # noqa: E731
    keep0 = ok(x)
    for _ in range(iters):
        feats = torch.cat([x[:, :1] * x, x[:, 1:2] * x[:, 1:], x[:, 2:] * x[:, 2:], x, torch.ones_like(x[:, :1])], dim=1)
        ws = []
        for c in range(3):
            rows = (keep0[:, c] & ok(x[:, c]) & ok(y[:, c])).unsqueeze(1)
            w = torch.linalg.lstsq(feats * rows, (y[:, c:c + 1] * rows)).solution
            if not bool(torch.isfinite(w).all()):                   # host read, as the reference's assert
                raise FloatingPointError("non-finite warp")
            ws.append(w)
        x = (feats @ torch.cat(ws, dim=1)).clamp(0, 1)
    sel = mask.expand_as(pred)
    psnr = lambda a, b: 10 * torch.log10(a.numel() / ((a - b) ** 2).sum())   # noqa: E731
    out = {"psnr": psnr(pred[sel], gt[sel]), "cc_psnr": psnr(x.reshape(pred.shape)[sel], gt[sel])}
    dsel = (lidar > 0.1) & (lidar < 80) & mask
    p, g = depth[dsel], lidar[dsel]
    e = g - p
    out.update(depth_RMSE=torch.sqrt((e * e).mean()), depth_absRel=(e.abs() / g).mean(),
               depth_delta1=(torch.max(p / g, g / p) < 1.25).float().mean())
    return out


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="960x540,1920x1080")
    ap.add_argument("--forms", default="torch,eager,graph")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from mtgs_amd import image_metrics
    lines = []
    for size in a.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        args = inputs(H, W)
        kw = dict(pred_depth=args[3], lidar_depth=args[4])
        ref_vals = {k: float(v) for k, v in image_metrics(*args[:3], **kw).items()}
        for form in a.forms.split(","):
            rec = {"form": form, "width": W, "height": H, "steps": a.steps}
            if form == "torch":
                try:
                    vals = {k: float(v) for k, v in torch_metrics(*args).items()}
                    rec.update(timed(lambda: torch_metrics(*args), max(3, a.steps // 5), 2), measured=True, lstsq_ran=True,
                               lstsq_driver="gels (the only driver on a GPU)", values=vals)
                except Exception as ex:                            # noqa: BLE001 -- recorded, not hidden
                    rec.update(measured=False, lstsq_ran=False, error=f"{type(ex).__name__}: {ex}"[:400])
            elif form == "eager":
                rec.update(timed(lambda: image_metrics(*args[:3], **kw), a.steps, a.warmup), measured=True, values=ref_vals)
            else:
                static = [t.clone() for t in args]
                s = torch.cuda.Stream()
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):
                    image_metrics(*static[:3], pred_depth=static[3], lidar_depth=static[4])
                torch.cuda.current_stream().wait_stream(s)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    out = image_metrics(*static[:3], pred_depth=static[3], lidar_depth=static[4])
                rec.update(timed(graph.replay, a.steps, a.warmup), measured=True,
                           values={k: float(v) for k, v in out.items()})
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
