#!/usr/bin/env python
"""Times mtgs_amd.undistort on a whole training frame -- image uint8 [H, W, 3], the valid mask with the ego rule (ego mask uint8
[H, W]), panoptic uint8 [H, W, 3] and semantic uint8 [H, W, 1] -- through a nuPlan-like lens in mode "optimal", at 1920 x 1080 and at
960 x 540.  Per shape:

    one launch     undistort_frame as shipped: every thread evaluates its map entry in fp64 and serves the four planes from it
    map in memory  the same launch reading a precomputed float32 [H, W, 2] map (the kernel's `map` argument) instead of evaluating
                   the closed form: 8 more bytes per pixel read, about 30 fp64 operations per pixel saved.  OpenCV's own fixed-point
                   form (CV_16SC2 + CV_16UC1) would be 6 bytes per pixel.  The two forms are timed alternately in the same process
    each eager and as a replayed HIP graph captured on one stream
    torch          the same formulas with torch.nn.functional.grid_sample on device tensors, from a precomputed grid (bilinear for
                   the image with the uint8 <-> float32 conversions, nearest for the rest).  Timed only: it is NOT bit-identical
    host           cv2 is not installed here: the host path (initUndistortRectifyMap + five cv2.remap + upload) is NOT measured

Device times are HIP events around windows of repeated calls (median of the windows).  The rate is the bytes the frame needs (every
source plane once + every destination plane once) over the event time.  Writes profiles/undistort.txt.

    python scripts/undistort_bench.py [--out profiles/undistort.txt] [--windows 5]
"""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as TF

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

from frame_bench import alternately, captured, device_ms, fmt  # noqa: E402
from mtgs_amd import undistort as U  # noqa: E402

HBM_PEAK = 8.0e12          # bytes per second, the specification
SHAPES = ((1080, 1920), (540, 960))
D = (-0.356123, 0.172545, -0.00213, 0.000464, -0.05231)


def lens(h, w):
    s = w / 1920.0
    return (1545.0 * s, 1545.0 * s, 960.0 * s, 560.0 * s)


def make_frame(rng, h, w):
    return {"image": rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "ego": (rng.random((h, w)) < 0.1).astype(np.uint8) * 255,
            "panoptic": rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "semantic": rng.integers(0, 20, (h, w, 1), dtype=np.uint8)}


def frame_bytes(h, w):
    return 2 * (3 + 1 + 3 + 1) * h * w                  # every source plane once, every destination plane once


def with_map(cam, data, m):
    """undistort_frame's launch with a map read from memory"""
    dev = cam.device
    out = {"image": torch.empty(cam.size + (3,), dtype=torch.uint8, device=dev), "valid_mask": torch.empty(cam.size + (1,), dtype=torch.uint8, device=dev),
           "panoptic": torch.empty(cam.size + (3,), dtype=torch.uint8, device=dev), "semantic": torch.empty(cam.size + (1,), dtype=torch.uint8, device=dev)}
    records = [U._record(data["ego"][:, :, None], out["valid_mask"], U._VALID), U._record(data["image"], out["image"], U._LINEAR, 3),
               U._record(data["panoptic"], out["panoptic"], U._NEAREST, 3), U._record(data["semantic"], out["semantic"], U._NEAREST, 1)]
    U._launch(cam, records, torch.cuda.current_stream(dev).cuda_stream, map=m)
    return out


def torch_frame(data, grid, ones):
    """grid_sample from a precomputed normalised grid [1, H, W, 2]"""
    planes = lambda x: x.permute(2, 0, 1)[None].to(torch.float32)
    image = TF.grid_sample(planes(data["image"]), grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    near = torch.cat([ones, 255.0 - planes(data["ego"][:, :, None]), planes(data["panoptic"]), planes(data["semantic"])], dim=1)
    near = TF.grid_sample(near, grid, mode="nearest", padding_mode="zeros", align_corners=True)[0].permute(1, 2, 0)
    return {"image": image[0].permute(1, 2, 0).round().to(torch.uint8), "valid_mask": (near[:, :, 0:1] != 0) & (near[:, :, 1:2] != 0),
            "panoptic": near[:, :, 2:5].to(torch.uint8), "semantic": near[:, :, 5:6].to(torch.uint8)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "undistort.txt"))
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "undistort_bench needs a HIP device"
    dev = torch.device("cuda")
    rng = np.random.default_rng(7)
    lines = [f"undistort_bench: {torch.cuda.get_device_name(0)}; device times are HIP events, median of {a.windows} windows of >= 0.2 s (the two "
             "kernel forms alternately, 3 rounds: median, min and max of the rounds)",
             f"tile {U.TILE_W} x {U.TILE_H} destination pixels per workgroup, one thread per pixel; planes: image (linear, uint8 x 3), valid "
             "mask with the ego rule, panoptic (nearest, uint8 x 3), semantic (nearest, uint8); lens: nuPlan-like, mode 'optimal'",
             "torch.nn.functional.grid_sample is timed only: it is not bit-identical.  A host OpenCV baseline is NOT measured: cv2 is not installed"]

    def say(line):
        print(line, flush=True)
        lines.append(line)

    verdicts = []
    for h, w in SHAPES:
        cam = U.undistort_camera(lens(h, w), D, (h, w), mode="optimal")
        frame = make_frame(rng, h, w)
        data = {k: torch.from_numpy(v).to(dev) for k, v in frame.items()}
        run = lambda: U.undistort_frame(cam, image=data["image"], ego_mask=data["ego"], panoptic=data["panoptic"], semantic=data["semantic"])
        m = U.undistort_map(cam)
        mapped = lambda: with_map(cam, data, m)
        ours, theirs = run(), mapped()
        same = all(torch.equal(ours[k].view(torch.uint8), theirs[k]) for k in ours)
        valid = float(ours["valid_mask"].float().mean())
        say(f"frame {w}x{h}: new camera fx' {cam.new_K[0, 0]:.3f} fy' {cam.new_K[1, 1]:.3f} cx' {cam.new_K[0, 2]:.3f} cy' {cam.new_K[1, 2]:.3f}, roi {cam.roi}; "
            f"{100 * valid:.1f} % of the pixels valid (ego rule included); the map in memory gives the same bytes: {same}")
        eager, eager_map = alternately([run, mapped], a.windows)
        replay, keep = captured(run)
        replay_map, keep_map = captured(mapped)
        graph, graph_map = alternately([replay, replay_map], a.windows)
        nbytes = frame_bytes(h, w)
        rate = lambda t, extra=0: (f"{(nbytes + extra) / 1e6:6.2f} MB -> {(nbytes + extra) / (t[0] * 1e-3) / 1e9:7.1f} GB/s = "
                                   f"{100 * (nbytes + extra) / (t[0] * 1e-3) / HBM_PEAK:.2f} % of the 8.0 TB/s HBM peak")
        say(f"    map evaluated per pixel, eager      {fmt(eager)}   replayed graph {fmt(graph)}   {rate(graph)} (replayed)")
        say(f"    map read from memory, eager         {fmt(eager_map)}   replayed graph {fmt(graph_map)}   {rate(graph_map, 8 * h * w)} (replayed)"
            f"   = {eager_map[0] / eager[0]:.2f} x / {graph_map[0] / graph[0]:.2f} x the evaluated form")
        verdicts.append((f"{w}x{h}", eager_map[0] / eager[0], graph_map[0] / graph[0]))
        image_only = device_ms(lambda: U.undistort_plane(data["image"], cam), a.windows)
        say(f"        image alone (linear, uint8 x 3)  {fmt(image_only)}   {6 * h * w / 1e6:6.2f} MB in + out -> {6 * h * w / (image_only[0] * 1e-3) / 1e9:7.1f} GB/s "
            "(eager: launch cost included)")
        t_map = device_ms(lambda: U.undistort_map(cam), a.windows)
        say(f"        the map alone (undistort_map)    {fmt(t_map)}   {8 * h * w / 1e6:6.2f} MB written")
        gx, gy = 2.0 * m[..., 0] / (w - 1) - 1.0, 2.0 * m[..., 1] / (h - 1) - 1.0
        grid = torch.stack([gx, gy], dim=-1)[None].contiguous()
        ones = torch.ones((1, 1, h, w), dtype=torch.float32, device=dev)
        theirs = torch_frame(data, grid, ones)
        off = {k: float((ours[k].to(torch.float32) - theirs[k].to(torch.float32)).abs().ne(0).float().mean()) for k in ours}
        t_torch = device_ms(lambda: torch_frame(data, grid, ones), a.windows)
        say(f"    torch grid_sample on the device     {fmt(t_torch)}   = {t_torch[0] / eager[0]:.1f} x undistort_frame (eager); share of elements that differ: "
            + ", ".join(f"{k} {100 * v:.2f} %" for k, v in off.items()))
        del keep, keep_map
    say("kernel form: " + "; ".join(f"{name}: reading the map takes {e:.2f} x (eager) / {g:.2f} x (replayed) the time of evaluating it" for name, e, g in verdicts)
        + ".  Shipped: the map evaluated per pixel, nothing stored; the `map` argument stays for a caller that brings a map of its own")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
