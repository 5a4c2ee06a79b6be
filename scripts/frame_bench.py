#!/usr/bin/env python
"""Times mtgs_amd.frame on a whole training frame -- image uint8 [H, W, 3], mask bool, semantic_map uint8, instance_map int32 and
depth float32, each [H, W, 1] -- at the two training scales of a 1920 x 1080 camera (-> 960 x 540 and -> 1440 x 810) and at one small
frame (240 x 135 -> 120 x 67, where launch cost is expected to decide).  Per shape:

    one launch    resize_frame as shipped: the two passes of a bilinear plane in ONE launch, the horizontal result of a tile kept in LDS
    two launches  the same kernel twice per bilinear plane through an [H, w] intermediate image in global memory (frame._bilinear's
                  two_pass); the bytes are the same.  The two forms are timed alternately in the same process
    each eager and as a replayed HIP graph captured on one stream
    host          the path it replaces: Pillow's Image.resize per plane on the CPU plus the upload of the five results
    torch         torch.nn.functional.interpolate on device tensors (bilinear with antialias for image and depth, nearest for the
                  rest).  Timed only: it is NOT bit-identical to Pillow

Device times are HIP events around windows of repeated calls (median of the windows); host times are a wall clock around work that
ends in a device synchronise.  A kernel's rate is the bytes the plane needs (input once + output once) over its event time.
Writes profiles/frame.txt.

    python scripts/frame_bench.py [--out profiles/frame.txt] [--windows 5]
    rocprofv3 --kernel-trace --stats -d DIR -o frame -- python scripts/frame_bench.py --trace-calls 20     # kernel times, a run of its own
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as TF

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from mtgs_amd import frame as F  # noqa: E402

HBM_PEAK = 8.0e12          # bytes per second, the specification
SHAPES = (((1080, 1920), (540, 960)), ((1080, 1920), (810, 1440)), ((135, 240), (67, 120)))
NEAREST = ("mask", "semantic_map", "instance_map")


def make_frame(rng, h, w):
    return {"image": rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "mask": rng.random((h, w, 1)) < 0.7,
            "semantic_map": rng.integers(0, 20, (h, w, 1), dtype=np.uint8), "instance_map": rng.integers(0, 70000, (h, w, 1), dtype=np.int32),
            "depth": np.where(rng.random((h, w, 1)) < 0.2, 0.0, rng.uniform(0.0, 6e4, (h, w, 1))).astype(np.float32)}


def two_launches(data, size):
    out = F.resize_frame({k: data[k] for k in NEAREST}, size)
    out["image"] = F._bilinear(data["image"], *size, two_pass=True)
    out["depth"] = F._bilinear(data["depth"], *size, two_pass=True)
    return out


def pillow_frame(frame, size):
    from PIL import Image
    out = {}
    for key, x in frame.items():
        flat = x if key == "image" else x[:, :, 0]
        resample = Image.Resampling.BILINEAR if F.RESAMPLE_MAP[key] == "bilinear" else Image.Resampling.NEAREST
        r = np.array(Image.fromarray(flat).resize((size[1], size[0]), resample=resample), dtype=x.dtype)
        out[key] = r if key == "image" else r[:, :, None]
    return out


def torch_frame(data, size):
    out = {}
    for key, x in data.items():
        planes = x.permute(2, 0, 1)[None].to(torch.float32)
        if F.RESAMPLE_MAP[key] == "bilinear":
            r = TF.interpolate(planes, size=size, mode="bilinear", antialias=True, align_corners=False)
            r = r.round().clamp(0, 255).to(torch.uint8) if key == "image" else r
        else:
            r = TF.interpolate(planes, size=size, mode="nearest").to(x.dtype)
        out[key] = r[0].permute(1, 2, 0)
    return out


def captured(fn):
    """fn as a HIP graph on one stream: (replay, the outputs)"""
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        fn()
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        outs = fn()
    return graph.replay, outs


def device_ms(fn, windows):
    """milliseconds per call: HIP events around windows of at least 0.2 s (or 3 calls), (median, min, max) of the windows"""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    calls = max(3, int(0.2 / max(time.perf_counter() - t0, 1e-6)))
    times = []
    for _ in range(windows):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(calls):
            fn()
        end.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(end) / calls)
    return float(np.median(times)), min(times), max(times)


def alternately(fns, windows, rounds=3):
    """the candidates timed in turn, `rounds` times over: per candidate the (median, min, max) over all its windows' medians"""
    seen = [[] for _ in fns]
    for _ in range(rounds):
        for times, fn in zip(seen, fns):
            times.append(device_ms(fn, windows)[0])
    return [(float(np.median(t)), min(t), max(t)) for t in seen]


def wall_ms(fn, reps):
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), min(times), max(times)


def fmt(t):
    return f"{t[0] * 1e3:9.1f} us (min {t[1] * 1e3:.1f}, max {t[2] * 1e3:.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "frame.txt"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--trace-calls", type=int, default=0, help="no timing: this many resize_frame calls per shape, for a kernel trace")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "frame_bench needs a HIP device"
    dev = torch.device("cuda")
    rng = np.random.default_rng(7)
    if a.trace_calls:
        for (h, w), size in SHAPES[:2]:
            data = {k: torch.from_numpy(v).to(dev) for k, v in make_frame(rng, h, w).items()}
            for _ in range(a.trace_calls):
                F.resize_frame(data, size)
            torch.cuda.synchronize()
        return
    try:
        import PIL
        pillow = PIL.__version__
    except ImportError:
        pillow = None
    lines = [f"frame_bench: {torch.cuda.get_device_name(0)}; device times are HIP events, median of {a.windows} windows of >= 0.2 s (the two kernel "
             "forms alternately, 3 rounds: median, min and max of the rounds); host times are wall clocks that end in a synchronise",
             f"tile {F.TILE_W} x {F.TILE_H} output pixels per workgroup, {F.CHUNK_ROWS} source rows per LDS chunk; Pillow "
             f"{pillow or 'is not installed: the host baseline is not measured'}",
             "torch.nn.functional.interpolate is timed only: it is not bit-identical to Pillow"]

    def say(line):
        print(line, flush=True)
        lines.append(line)

    losses, ratios = [], []
    for (h, w), size in SHAPES:
        frame = make_frame(rng, h, w)
        data = {k: torch.from_numpy(v).to(dev) for k, v in frame.items()}
        ours, split = F.resize_frame(data, size), two_launches(data, size)
        same_forms = all(torch.equal(ours[k], split[k]) for k in ours)
        say(f"frame {w}x{h} -> {size[1]}x{size[0]}: one launch and two launches give the same bytes: {same_forms}")
        if pillow:
            want = pillow_frame(frame, size)
            wrong = {k: int((ours[k].cpu().numpy().view(np.uint8) != want[k].view(np.uint8)).sum()) for k in want if k != "mask"}
            wrong["mask"] = int((ours["mask"].cpu().numpy() != (want["mask"].view(np.uint8) != 0)).sum())
            say(f"    bytes that differ from Pillow {pillow}: {wrong}")
        one_eager, two_eager = alternately([lambda: F.resize_frame(data, size), lambda: two_launches(data, size)], a.windows)
        replay_one, keep_one = captured(lambda: F.resize_frame(data, size))
        replay_two, keep_two = captured(lambda: two_launches(data, size))
        one_graph, two_graph = alternately([replay_one, replay_two], a.windows)
        as_float = device_ms(lambda: F.resize_frame(data, size, image_float=True), a.windows)
        say(f"    one launch per plane, eager         {fmt(one_eager)}   replayed graph {fmt(one_graph)}   (image_float=True, eager: {fmt(as_float)})")
        say(f"    two launches per plane, eager       {fmt(two_eager)}   replayed graph {fmt(two_graph)}   = {two_eager[0] / one_eager[0]:.2f} x / "
            f"{two_graph[0] / one_graph[0]:.2f} x the one-launch form")
        ratios.append((two_eager[0] / one_eager[0], two_graph[0] / one_graph[0]))
        parts = {"image (uint8 x 3, bilinear)": (lambda: F.resize_plane(data["image"], size), h * w * 3 + size[0] * size[1] * 3),
                 "depth (float32, bilinear)": (lambda: F.resize_plane(data["depth"], size), 4 * (h * w + size[0] * size[1])),
                 "mask + semantic + instance (nearest)": (lambda: F.resize_frame({k: data[k] for k in NEAREST}, size), 6 * size[0] * size[1] * 2)}
        for name, (fn, nbytes) in parts.items():
            t = device_ms(fn, a.windows)
            say(f"        {name:38s} {fmt(t)}   {nbytes / 1e6:6.2f} MB in + out -> {nbytes / (t[0] * 1e-3) / 1e9:7.1f} GB/s = "
                f"{100 * nbytes / (t[0] * 1e-3) / HBM_PEAK:.2f} % of the 8.0 TB/s HBM peak (eager: launch cost included)")
        t_torch = device_ms(lambda: torch_frame(data, size), a.windows)
        say(f"    torch interpolate on the device     {fmt(t_torch)}   = {t_torch[0] / one_eager[0]:.1f} x resize_frame (eager)")
        if t_torch[0] < one_eager[0]:
            losses.append(f"{w}x{h} -> {size[1]}x{size[0]}: eager resize_frame {one_eager[0] * 1e3:.1f} us loses to torch interpolate {t_torch[0] * 1e3:.1f} us")
        if pillow:
            t_host = wall_ms(lambda: {k: torch.from_numpy(v).to(dev) for k, v in pillow_frame(frame, size).items()}, 10)
            t_ours = wall_ms(lambda: F.resize_frame(data, size), 50)
            say(f"    host: Pillow + upload of the results {fmt(t_host)}   resize_frame by the same wall clock {fmt(t_ours)}   = {t_host[0] / t_ours[0]:.1f} x")
            if t_host[0] < t_ours[0]:
                losses.append(f"{w}x{h} -> {size[1]}x{size[0]}: resize_frame {t_ours[0] * 1e3:.1f} us by the wall clock loses to the host path {t_host[0] * 1e3:.1f} us")
        else:
            say("    host: Pillow + upload of the results: not measured (Pillow is not installed)")
        del keep_one, keep_two
    say("kernel form kept: ONE launch per bilinear plane, the horizontal result of a tile staged in LDS.  The two-launch form through an "
        f"[H, w] intermediate image takes {min(r[0] for r in ratios):.2f} - {max(r[0] for r in ratios):.2f} x its time eager and "
        f"{min(r[1] for r in ratios):.2f} - {max(r[1] for r in ratios):.2f} x replayed (rows above); it stays reachable as "
        "frame._bilinear(two_pass=True) for this comparison only.  Kernel times without launch cost: profiles/frame_kernel_stats.csv")
    say("shapes where the device path loses: " + ("; ".join(losses) if losses else "none among the shapes timed"))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
