#!/usr/bin/env python
"""Times the JPEG encode of a presented frame: mtgs_amd.jpeg on the device against what it replaces, the download of the raw uint8
frame followed by Pillow's encode on the host at the same settings (the evaluation dump's path; the render tool's mediapy goes
through Pillow as well).  The viewer's own encoder inside viser (recalled to be OpenCV or imageio) is not installed here and is not
measured.

    228 x 128  quality 40      the viewer while moving        910 x 512  quality 40 and 75     the viewer, static
    1920 x 1080 quality 75     the render tool, one output

Both paths end with the file in host memory, and are timed with the host clock around one frame ending there (the device path
ends in the copy of `nbytes` bytes, which synchronises): the median and the spread of `--reps` frames after `--warmup`.  The device
path is run eagerly and as a replayed HIP graph; the encode alone is also timed with device events.  The two files are compared
before timing.  The per-kernel split is torch.profiler's device time per kernel name over `--reps` eager encodes.  Writes
profiles/jpeg.txt.

    python scripts/jpeg_bench.py [--reps 50] [--warmup 10] [--out profiles/jpeg.txt]
"""
import argparse
import io
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from mtgs_amd import jpeg as J  # noqa: E402

CASES = [(128, 228, 40), (512, 910, 40), (512, 910, 75), (1080, 1920, 75)]


def frame(h, w, seed):
    """uint8 [h, w, 3]: smooth structure, edges and mild noise -- neither the flat nor the incompressible extreme"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    base = np.stack([np.sin(xx / 37.0) * np.cos(yy / 23.0), np.sin((xx + yy) / 51.0), np.cos(xx / 11.0 - yy / 71.0)], -1) * 0.35 + 0.5
    base += ((xx // 64 + yy // 48) % 2)[..., None] * 0.12
    base += rng.normal(0, 0.02, (h, w, 3))
    return (np.clip(base, 0, 1) * 255).astype(np.uint8)


def host_clock(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return ms


def device_events(fn, reps, warmup):
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


def kernel_split(fn, reps):
    """[(kernel name, mean device us per encode)] by torch.profiler; None if it reports nothing"""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        rows = []
        for ev in prof.key_averages():
            total = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0)
            if str(ev.device_type).endswith("CUDA") and total:
                rows.append((ev.key, total / reps, ev.count / reps))
        return sorted(rows, key=lambda r: -r[1]) or None
    except Exception as exc:                    # the split is a report, not a result
        print(f"torch.profiler: {exc!r}", file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "jpeg.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "jpeg_bench.py measures on the device: there is no CPU timing"
    try:
        import PIL
        from PIL import Image, features
        pillow = f"Pillow {PIL.__version__}, libjpeg-turbo {features.version('jpg')}" if features.check_feature("libjpeg_turbo") else f"Pillow {PIL.__version__}"
    except ImportError:
        Image, pillow = None, "Pillow is not installed: the host path is not measured"
    lines = [f"mtgs_amd.jpeg against the download of the raw frame + the host encode ({pillow}), {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"host clock around one frame that ends with the file in host memory, median (min .. max) of {a.reps} after {a.warmup} warm-ups;",
             "viser's own encoder (OpenCV or imageio, as recalled) is not installed here: not measured", ""]
    for h, w, q in CASES:
        pixels = frame(h, w, h + q)
        image = torch.from_numpy(pixels).cuda()
        out = J.encode_jpeg(image, q)
        ours = out.tobytes()
        encode = lambda: J.encode_jpeg(image, q, out=out)
        replay = graphed(encode)
        lines.append(f"{w} x {h}, quality {q}, 4:2:0: raw frame {pixels.nbytes} bytes, file {len(ours)} bytes ({pixels.nbytes / len(ours):.1f}x fewer over PCIe, "
                     f"+ 16 bytes of length and flag); buffer capacity {out.data.numel()} bytes, workspace {J.sizes(h, w)[0]} bytes")
        t_host = None
        if Image is not None:
            def host():
                buf = io.BytesIO()
                Image.fromarray(image.cpu().numpy()).save(buf, "JPEG", quality=q, subsampling="4:2:0")
                return buf.getvalue()
            lines.append(f"  files identical to the host encoder's: {host() == ours}")
            t_host = host_clock(host, a.reps, a.warmup)
            t_copy = host_clock(lambda: image.cpu(), a.reps, a.warmup)
            lines.append(f"  host: .cpu() of the raw frame + Pillow's encode        {fmt(t_host)}     of which the download {fmt(t_copy)}")
        t_eager = host_clock(lambda: (encode(), out.tobytes()), a.reps, a.warmup)
        t_graph = host_clock(lambda: (replay(), out.tobytes()), a.reps, a.warmup)
        lines.append(f"  device, eager: encode + length read + copy of nbytes   {fmt(t_eager)}")
        lines.append(f"  device, replayed graph + length read + copy of nbytes  {fmt(t_graph)}")
        lines.append(f"  device, the encode alone (device events): eager        {fmt(device_events(encode, a.reps, a.warmup))}")
        lines.append(f"  device, the encode alone (device events): graph        {fmt(device_events(replay, a.reps, a.warmup))}")
        if t_host is not None:
            lines.append(f"  ratio host / device: eager {statistics.median(t_host) / statistics.median(t_eager):.1f}x, graph "
                         f"{statistics.median(t_host) / statistics.median(t_graph):.1f}x")
        split = kernel_split(encode, a.reps)
        if split:
            lines.append("  per kernel (torch.profiler, device us per encode, launches per encode):")
            lines += [f"    {us:8.1f} us  x{count:.0f}  {name[:140]}" for name, us, count in split]
        else:
            lines.append("  per kernel: torch.profiler reported no device events")
        lines.append("")
        print("\n".join(lines[-(len(split or []) + 10):]), flush=True)
    out_path = Path(a.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text("\n".join(lines) + "\n")
    print(f"wrote {out_path}")


if __name__ == "__main__":
    main()
