#!/usr/bin/env python
"""Times mtgs_amd.lpips against the torch.nn.functional chain of the same definition on the same GPU, and each convolution layer
against the library's convolution.

    whole metric   1920 x 1080, 910 x 512, 228 x 128; one call on two images and a mask, eager and as a replayed HIP graph, ours
                   and the fp32 torch chain (mask multiply, 2x - 1, scaling layer, five convolutions with ReLUs and two pools, and
                   per tap two channel norms, a squared difference, a 1x1 convolution and a spatial mean)
    per layer      lpips_conv alone on the activations of the layer before: time, and achieved TFLOP/s = 2 M K cout / time with
                   M = 2 oh ow (the operations the layer needs, padding taps counted, as the usual convention has it); beside it
                   F.conv2d + bias + ReLU of the same layer (NCHW fp32, the library's choice of algorithm)
    accuracy       e = |ours - fp64|, e32 = |fp32 CPU restatement - fp64| on the shapes of tests/test_gpu_lpips.py

Device events around one call on the current stream, `--reps` calls after `--warmup` untimed ones; median (min .. max).  Weights are
seeded random ones: there are no trained LPIPS weights here, and the time does not depend on them.  Writes profiles/lpips.txt.

    python scripts/lpips_bench.py [--reps 30] [--warmup 5] [--out profiles/lpips.txt]
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from mtgs_amd import lpips as L  # noqa: E402
from tests import lpips_refs as R  # noqa: E402

SIZES = ((1080, 1920), (512, 910), (128, 228))
ACCURACY = ((31, 31, False), (35, 47, False), (64, 96, False), (67, 131, True), (128, 228, False))


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ms.append(s.elapsed_time(e))
    return ms


def fmt(ms):
    return f"{statistics.median(ms) * 1e3:9.1f} us  ({min(ms) * 1e3:.1f} .. {max(ms) * 1e3:.1f})"


def graphed(fn):
    """fn captured once on a side stream (after a warm-up there); returns the replay"""
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        fn()
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        fn()
    return graph.replay


class TorchChain:
    """The definition in torch.nn.functional on the device, fp32, NCHW, as the module it replaces runs it; returns a 0-dim tensor."""

    def __init__(self, convs, lins):
        self.convs = [(w.cuda(), b.cuda()) for w, b in convs]
        self.lins = [v.cuda().reshape(1, -1, 1, 1) for v in lins]
        self.shift = torch.tensor(R.SHIFT, device="cuda").reshape(1, 3, 1, 1)
        self.scale = torch.tensor(R.SCALE, device="cuda").reshape(1, 3, 1, 1)

    def __call__(self, pred, gt, mask):
        x = torch.stack([pred * mask, gt * mask]).permute(0, 3, 1, 2)
        x = (2 * x - 1 - self.shift) / self.scale
        total = None
        for (w, b), v, (_, _, _, stride, pad, pool) in zip(self.convs, self.lins, R.LAYERS):
            if pool:
                x = F.max_pool2d(x, 3, 2)
            x = F.relu(F.conv2d(x, w, b, stride=stride, padding=pad))
            u = x / torch.sqrt(1e-8 + (x * x).sum(dim=1, keepdim=True))
            d = F.conv2d((u[0:1] - u[1:2]) ** 2, v).mean()
            total = d if total is None else total + d
        return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "lpips.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "lpips_bench.py measures on the device: there is no CPU timing"
    convs, lins = R.random_weights(seed=5)
    dev = L.LpipsWeights.from_tensors(convs, lins, device="cuda")
    chain = TorchChain(convs, lins)
    lines = [f"mtgs_amd.lpips against the torch.nn.functional chain of the same definition, {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"device events around one call, median (min .. max) of {a.reps} after {a.warmup} warm-ups; seeded random weights", ""]

    def say(*new):
        lines.extend(new)
        print("\n".join(new), flush=True)

    for H, W in SIZES:
        pred, gt, mask = (t.cuda() for t in R.images(H, W, seed=H, masked=True))
        ours = lambda: L.lpips(pred, gt, mask, weights=dev)                     # noqa: E731
        theirs = lambda: chain(pred, gt, mask)                                  # noqa: E731
        vo, vt = ours().item(), theirs().item()
        say(f"whole metric, {W} x {H}: ours {vo:.7g}, torch chain {vt:.7g}, |difference| {abs(vo - vt):.3g}")
        t_e = timed(ours, a.reps, a.warmup)
        say(f"  ours, eager (13 launches)       {fmt(t_e)}")
        t_g = timed(graphed(ours), a.reps, a.warmup)
        say(f"  ours, replayed graph            {fmt(t_g)}")
        c_e = timed(theirs, a.reps, a.warmup)
        say(f"  torch chain, eager              {fmt(c_e)}")
        try:
            c_g = timed(graphed(theirs), a.reps, a.warmup)
            say(f"  torch chain, replayed graph     {fmt(c_g)}")
            ratio_g = f"{statistics.median(c_g) / statistics.median(t_g):.2f}x"
        except Exception as exc:        # the library's convolution may refuse a capture; that is a finding, not a failure of this script
            say(f"  torch chain, replayed graph     not captured: {type(exc).__name__}: {str(exc).splitlines()[0][:120]}")
            ratio_g = "n/a"
        say(f"  ratio torch chain / ours: eager {statistics.median(c_e) / statistics.median(t_e):.2f}x, graph {ratio_g}")

        # per layer, on our own activations
        x = None
        total_ms = 0.0
        for i, (cin, cout, k, stride, pad, pool) in enumerate(R.LAYERS):
            packed, bias, _ = dev.layer(i)
            if pool:
                x = L.maxpool_nhwc(x)
            if i == 0:
                fn = lambda: L.conv_first(pred, gt, mask, packed, bias)         # noqa: E731
                x_nchw = torch.cat([R.transform(pred.cpu(), mask.cpu(), True, torch.float32), R.transform(gt.cpu(), mask.cpu(), True, torch.float32)]).cuda()
            else:
                xin = x
                fn = lambda: L.conv2d_nhwc(xin, packed, bias, k, stride, pad)   # noqa: E731
                x_nchw = x.permute(0, 3, 1, 2).contiguous()
            w_t, b_t = chain.convs[i]
            lib = lambda: F.relu(F.conv2d(x_nchw, w_t, b_t, stride=stride, padding=pad))    # noqa: E731
            y = fn()
            diff = float((y.permute(0, 3, 1, 2) - lib()).abs().max())
            t_o, t_l = timed(fn, a.reps, a.warmup), timed(lib, a.reps, a.warmup)
            flop = 2.0 * y.shape[0] * y.shape[1] * y.shape[2] * (k * k * cin) * cout
            mo, ml = statistics.median(t_o), statistics.median(t_l)
            total_ms += mo
            say(f"  conv{i + 1} {cin:3d} -> {cout:3d} {k}x{k}, out {y.shape[2]} x {y.shape[1]}, {flop / 1e9:6.2f} GFLOP: ours {fmt(t_o)} = {flop / mo / 1e9:6.1f} TFLOP/s;"
                f"  library conv + ReLU {fmt(t_l)} = {flop / ml / 1e9:6.1f} TFLOP/s;  max |difference| {diff:.3g}")
            x = y
        say(f"  the five convolutions: {total_ms * 1e3:.1f} us of ours", "")

    say("accuracy on the test shapes (e = |ours - fp64|, e32 = |fp32 CPU restatement - fp64|; the test asserts e <= 4 e32 + 1e-7):")
    for H, W, masked in ACCURACY:
        pred, gt, mask = R.images(H, W, seed=H + W, masked=masked)
        for norm in ("torchmetrics", "lpips"):
            ref64 = R.lpips_ref(pred, gt, mask, convs, lins, norm=norm)
            ref32 = R.lpips_ref(pred, gt, mask, convs, lins, norm=norm, dtype=torch.float32)
            got = L.lpips(pred.cuda(), gt.cuda(), None if mask is None else mask.cuda(), weights=dev, norm=norm).item()
            say(f"  {H:3d} x {W:3d}{' masked' if masked else '       '} {norm:12s} value {ref64:.9g}  e {abs(got - ref64):.3g}  e32 {abs(ref32 - ref64):.3g}")

    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
