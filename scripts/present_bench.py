#!/usr/bin/env python
"""Times the presentation of a rendered frame: mtgs_amd.present against the torch transcription of what the viewer thread and the
render tool do today (tests/present_refs.py: nerfstudio's colormaps with their host reads and the per-call upload of the colour
table, torch.cat / the column fill, the uint8 cast, `.cpu().numpy()`, np.pad / np.concatenate, F.interpolate of the depth).

    render tool   1920 x 1080, `rgb | depth` concatenated, near / far from the data          render_frame_torch  vs  render_frame
    viewer        512 x 910 and 128 x 228, depth shown with `normalize`, with and without    viewer_frame_torch + viewer_depth_torch
                  the split against rgb, depth compositing on                                 vs  viewer_frame + viewer_depth

Each side is timed with device events around one frame on the current stream, `--reps` frames after `--warmup` untimed ones; the
median and the spread (min .. max) are printed.  Ours is timed three ways: eager with `out=`, the same as a replayed HIP graph, and
eager followed by the download of the uint8 frame (and of the resized depth), which is what the transcription's time contains as
well.  The transcription cannot be captured: it reads the device from the host.  Launch counts: ours counted at the C ABI, the
transcription's device kernels and copies counted by torch.profiler over one frame.  The frames of the two sides are compared
before timing.  Writes profiles/present.txt.

    python scripts/present_bench.py [--reps 50] [--warmup 10] [--out profiles/present.txt]
"""
import argparse
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from mtgs_amd import _lib, present as P  # noqa: E402
from tests import present_refs as R  # noqa: E402

SCALE_RATIO = 10.0        # viser_scale_ratio: any value, one multiplication


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
    return f"{statistics.median(ms) * 1e3:8.1f} us  ({min(ms) * 1e3:.1f} .. {max(ms) * 1e3:.1f})"


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


def count_ours(fn):
    calls = []
    original = _lib.call

    def counting(name, *args):
        calls.append(name)
        return original(name, *args)
    P.call = counting
    try:
        fn()
    finally:
        P.call = original
    return len(calls)


def count_device_activities(fn):
    """device kernels and memory copies of one call of fn, by torch.profiler; None if the profiler gives nothing"""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        kernels = copies = 0
        for ev in prof.events():
            if str(ev.device_type).endswith("CUDA"):
                if "memcpy" in ev.name.lower() or "copy" in ev.name.lower() and "kernel" not in ev.name.lower():
                    copies += 1
                else:
                    kernels += 1
        return (kernels, copies) if kernels else None
    except Exception as exc:                    # the count is a report, not a result
        print(f"torch.profiler: {exc!r}", file=sys.stderr)
        return None


def scene(H, W, seed):
    g = torch.Generator().manual_seed(seed)
    rgb = torch.rand((H, W, 3), generator=g)
    depth = torch.rand((H, W, 1), generator=g) * 78.0 + 2.0
    acc = torch.rand((H, W, 1), generator=g)
    return {k: v.cuda() for k, v in (("rgb", rgb), ("depth", depth), ("accumulation", acc))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "present.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "present_bench.py measures on the device: there is no CPU timing"
    for name, table in R.tables().items():
        P.register_colormap(name, table)
    lines = [f"mtgs_amd.present against the torch transcription (tests/present_refs.py), {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"device events around one frame, median (min .. max) of {a.reps} after {a.warmup} warm-ups", ""]

    def report(title, theirs, ours, ours_download, differing):
        t = timed(theirs, a.reps, a.warmup)
        e = timed(ours, a.reps, a.warmup)
        d = timed(ours_download, a.reps, a.warmup)
        g = timed(graphed(ours), a.reps, a.warmup)
        counted = count_device_activities(theirs)
        lines.append(title)
        lines.append(f"  transcription (host reads, table upload, download)   {fmt(t)}   "
                     + (f"{counted[0]} kernels + {counted[1]} copies" if counted else "launches not counted"))
        lines.append(f"  ours, eager, out=                                     {fmt(e)}   {count_ours(ours)} launches")
        lines.append(f"  ours, replayed graph                                  {fmt(g)}")
        lines.append(f"  ours, eager + download of the frame                   {fmt(d)}")
        lines.append(f"  ratio transcription / ours: eager {statistics.median(t) / statistics.median(e):.1f}x, graph "
                     f"{statistics.median(t) / statistics.median(g):.1f}x, with the download {statistics.median(t) / statistics.median(d):.1f}x;  "
                     f"pixels that differ between the two frames: {differing}")
        lines.append("")
        print("\n".join(lines[-7:]), flush=True)

    # ---- the render tool: rgb | depth at 1920 x 1080 ----
    H, W = 1080, 1920
    outputs = scene(H, W, 0)
    o, ns = P.ColormapOptions(), R.NSColormapOptions()
    frame = torch.empty((H, 2 * W, 3), dtype=torch.uint8, device="cuda")
    names = ["rgb", "depth"]
    theirs = lambda: R.render_frame_torch(outputs, names, None, None, ns)
    ours = lambda: P.render_frame(outputs, names, None, None, o, out=frame)
    differing = int((ours().cpu().numpy() != theirs()[1]).any(axis=-1).sum())
    report(f"render tool, {W} x {H}, rgb | depth (near / far from the data), frame {2 * W} x {H}", theirs, ours, lambda: ours().cpu(), differing)

    # ---- the viewer: depth with normalize, with and without the split against rgb, depth compositing on ----
    for (H, W), state in (((512, 910), "high"), ((128, 228), "low_move")):
        outputs = scene(H, W, 1)
        h, w = P.depth_size(H, W, state)
        for split in (None, "rgb"):
            o, ns = P.ColormapOptions("turbo", normalize=True), R.NSColormapOptions("turbo", True)
            so, sns = (None, None) if split is None else (P.ColormapOptions(), R.NSColormapOptions())
            frame = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
            small = torch.empty((h, w, 1), device="cuda")

            def theirs():
                f = R.viewer_frame_torch(outputs, "depth", ns, split, sns, 0.5, W / H)
                return f, R.viewer_depth_torch(outputs["depth"], state).cpu().numpy() * SCALE_RATIO

            def ours():
                P.viewer_frame(outputs, "depth", o, split, so, 0.5, W / H, out=frame)
                P.viewer_depth(outputs["depth"], state, SCALE_RATIO, out=small)
                return frame

            differing = int((ours().cpu().numpy() != theirs()[0]).any(axis=-1).sum())
            report(f"viewer, {W} x {H} ({state}), depth normalized{'' if split is None else ', split against rgb'}, gl_z_buf_depth {w} x {h}",
                   theirs, ours, lambda: (ours().cpu(), small.cpu()), differing)

    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
