#!/usr/bin/env python
"""Times the evaluation dump's way back into the raw camera -- mtgs_amd.undistort.redistort_image and mtgs_amd.evaldump -- on a rendered
float32 [H, W, 3] frame through a nuPlan-like lens in mode "optimal", at 1920 x 1080 and at 960 x 540, with 5 and with 20 iterations
of the inverse lens model.  Per shape and iteration count:

    evaluated      redistort_image as shipped: every thread iterates its map entry in fp64 inside the launch
    map in memory  the same launch reading a precomputed float32 [H, W, 2] map (8 more bytes per pixel read, the iteration saved); the
                   two forms are timed alternately in the same process, eager and as a replayed HIP graph
    the map alone  redistort_map, what a per-camera map costs once
    eval_dump      the whole "nuplan" dump with the file in host memory: redistort_image, encode_jpeg, tobytes (a wall clock that ends
                   in the host copy); beside it encode_jpeg of the uint8 frame alone and of the float32 frame alone -- what the
                   intermediate uint8 frame costs is the launch that writes it, the encoder reads a quarter of the float frame's bytes
    torch          torch.nn.functional.grid_sample from a precomputed grid on the device, then * 255 and the cast.  Timed only: it
                   is NOT bit-identical
    host           the NumPy restatement (tests/redistort_refs.py) between the two transfers (.cpu() and the upload).  NOT OpenCV: cv2
                   is not installed, so the host path the reference runs cannot be measured here

With --lib the library of another build is loaded instead (scripts/build_variant.py) and only the two kernel forms are timed: an A/B
is a second run, appended with --append.  profiles/redistort.txt keeps the one made so far: four pixels per thread with dword stores.

Device times are HIP events around windows of repeated calls (median of the windows).  The rate is the bytes the frame needs (the
float32 source once + the uint8 destination once, + the map when it is read) over the event time.  Writes profiles/redistort.txt.

    python scripts/redistort_bench.py [--out profiles/redistort.txt] [--windows 5] [--lib PATH --append]
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

HBM_PEAK = 8.0e12          # bytes per second, the specification
SHAPES = ((1080, 1920), (540, 960))
ITERATIONS = (5, 20)
D = (-0.356, 0.173, -0.0002, 0.0003, -0.052)


def lens(h, w):
    s = w / 1920.0
    return (1545.0 * s, 1545.0 * s, 960.0 * s, 560.0 * s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "redistort.txt"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--lib", default=None, help="another build of the library (A/B): only the kernel forms are timed")
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()
    if a.lib:
        from mtgs_amd import _lib
        _lib.use_library(a.lib)
    from frame_bench import alternately, captured, device_ms, fmt, wall_ms
    from mtgs_amd import evaldump as E
    from mtgs_amd import jpeg as J
    from mtgs_amd import undistort as U
    from tests import redistort_refs as R
    assert torch.cuda.is_available(), "redistort_bench needs a HIP device"
    dev = torch.device("cuda")
    rng = np.random.default_rng(7)
    what = f"library {a.lib}" if a.lib else "the shipped library"
    lines = [f"redistort_bench ({what}): {torch.cuda.get_device_name(0)}; device times are HIP events, median of {a.windows} windows of >= 0.2 s "
             "(the two kernel forms alternately, 3 rounds: median, min and max of the rounds); host and eval_dump times are wall clocks",
             f"tile {U.TILE_W} x {U.TILE_H} destination pixels per workgroup, one thread per pixel; source float32 [H, W, 3], conversion "
             "'truncate'; lens: nuPlan-like, mode 'optimal'",
             "torch.nn.functional.grid_sample is timed only: it is not bit-identical.  The host baseline is the NumPy restatement between "
             "the two transfers, NOT OpenCV: cv2 is not installed"]

    def say(line):
        print(line, flush=True)
        lines.append(line)

    losses, verdicts = [], []
    for h, w in SHAPES:
        cam = U.undistort_camera(lens(h, w), D, (h, w), mode="optimal")
        frame = rng.random((h, w, 3), dtype=np.float32)
        x = torch.from_numpy(frame).to(dev)
        nbytes = (12 + 3) * h * w
        rate = lambda t, extra=0: (f"{(nbytes + extra) / 1e6:6.2f} MB -> {(nbytes + extra) / (t[0] * 1e-3) / 1e9:7.1f} GB/s = "
                                   f"{100 * (nbytes + extra) / (t[0] * 1e-3) / HBM_PEAK:.2f} % of the 8.0 TB/s HBM peak")
        say(f"frame {w}x{h}: new camera fx' {cam.new_K[0, 0]:.3f} fy' {cam.new_K[1, 1]:.3f} cx' {cam.new_K[0, 2]:.3f} cy' {cam.new_K[1, 2]:.3f}")
        graphs = {}
        for n in ITERATIONS:
            m = U.redistort_map(cam, n)
            out = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
            run = lambda: U.redistort_image(x, cam, n, out=out)
            mapped = lambda: U.redistort_image(x, cam, n, map=m, out=out)
            same = torch.equal(run().clone(), mapped())
            eager, eager_map = alternately([run, mapped], a.windows)
            replay, keep = captured(run)
            replay_map, keep_map = captured(mapped)
            graph, graph_map = alternately([replay, replay_map], a.windows)
            graphs[n] = (graph, graph_map)
            say(f"  {n:2d} iterations; the map in memory gives the same bytes: {same}")
            say(f"    map evaluated in the launch, eager  {fmt(eager)}   replayed graph {fmt(graph)}   {rate(graph)} (replayed)")
            say(f"    map read from memory, eager         {fmt(eager_map)}   replayed graph {fmt(graph_map)}   {rate(graph_map, 8 * h * w)} (replayed)"
                f"   = {eager_map[0] / eager[0]:.2f} x / {graph_map[0] / graph[0]:.2f} x the evaluated form")
            verdicts.append((f"{w}x{h}, {n} iterations", eager_map[0] / eager[0], graph_map[0] / graph[0]))
            if a.lib:
                del keep, keep_map
                continue
            t_map = device_ms(lambda: U.redistort_map(cam, n), a.windows)
            say(f"        the map alone (redistort_map)     {fmt(t_map)}   {8 * h * w / 1e6:6.2f} MB written")
            dump = wall_ms(lambda: E.eval_dump(x, "nuplan", cam=cam, iterations=n)["rendered"].tobytes(), 20)
            dump_map = wall_ms(lambda: E.eval_dump(x, "nuplan", cam=cam, iterations=n, map=m)["rendered"].tobytes(), 20)
            size = len(E.eval_dump(x, "nuplan", cam=cam, iterations=n)["rendered"].tobytes())
            say(f"    eval_dump('nuplan') to host bytes   {fmt(dump)}   with the map in memory {fmt(dump_map)}   the file: {size} bytes (noise: the worst case)")
            del keep, keep_map
        if a.lib:
            continue
        # fp64 issue or bytes: the cost of 15 more iterations against the whole launch with no iteration at all (the map read)
        (g5, gm5), (g20, _) = graphs[5], graphs[20]
        per_iteration = (g20[0] - g5[0]) / 15
        say(f"  what binds: one iteration costs {per_iteration * 1e3:.2f} us per frame ({per_iteration * 1e6 / (h * w) * 1e3:.3f} ps per pixel); the launch without any "
            f"({gm5[0] * 1e3:.1f} us, the map read) runs at {100 * (nbytes + 8 * h * w) / (gm5[0] * 1e-3) / HBM_PEAK:.1f} % of the HBM peak -- "
            + ("fp64 issue binds the evaluated form at 20 iterations" if g20[0] > 1.5 * gm5[0] else "neither fp64 issue nor HBM traffic binds: the launch is latency-bound")
            + f"; at 5 iterations the iteration is {100 * 5 * per_iteration / g5[0]:.0f} % of the launch")
        raw = U.redistort_image(x, cam, 5)
        enc_u8 = device_ms(lambda: J.encode_jpeg(raw), a.windows)
        enc_f32 = device_ms(lambda: J.encode_jpeg(x), a.windows)
        say(f"  the intermediate uint8 frame: encode_jpeg of it {fmt(enc_u8)}, of a float32 frame {fmt(enc_f32)}; it is written once and read once, "
            f"{2 * 3 * h * w / 1e6:.2f} MB = {100 * 2 * 3 * h * w / (nbytes + 3 * h * w):.0f} % of the two launches' bytes -- a fused first stage would save at most that")
        # torch on the device
        m = U.redistort_map(cam, 5)
        grid = torch.stack([2.0 * m[..., 0] / (w - 1) - 1.0, 2.0 * m[..., 1] / (h - 1) - 1.0], dim=-1)[None].contiguous()
        planes = x.permute(2, 0, 1)[None]
        torch_way = lambda: (TF.grid_sample(planes, grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0].permute(1, 2, 0).clamp(0, 1) * 255.0).to(torch.uint8)
        differ = float((torch_way().to(torch.int16) - raw.to(torch.int16)).ne(0).float().mean())
        t_torch = device_ms(torch_way, a.windows)
        ours = device_ms(lambda: U.redistort_image(x, cam, 5), a.windows)
        say(f"  torch grid_sample on the device       {fmt(t_torch)}   = {t_torch[0] / ours[0]:.1f} x redistort_image (eager, 5 iterations, {fmt(ours).strip()}); "
            f"{100 * differ:.2f} % of its bytes differ")
        if t_torch[0] < ours[0]:
            losses.append(f"{w}x{h}: torch grid_sample {t_torch[0] * 1e3:.1f} us < redistort_image {ours[0] * 1e3:.1f} us")
        # the host: NumPy between the two transfers
        K, Dm, new_K = tuple(cam.params[:4].tolist()), tuple(cam.params[8:13].tolist()), tuple(cam.params[4:8].tolist())
        host_way = lambda: torch.from_numpy(R.redistort_image(x.cpu().numpy(), K, Dm, new_K, (h, w), 5)).to(dev)
        agree = torch.equal(host_way(), raw)
        t_host = wall_ms(host_way, 3)
        ours_wall = wall_ms(lambda: U.redistort_image(x, cam, 5), 20)
        say(f"  host: NumPy restatement + transfers   {fmt(t_host)}   = {t_host[0] / ours_wall[0]:.0f} x redistort_image (wall, {fmt(ours_wall).strip()}); same bytes: {agree}")
        if t_host[0] < ours_wall[0]:
            losses.append(f"{w}x{h}: the host path {t_host[0]:.2f} ms < redistort_image {ours_wall[0]:.2f} ms")
    say("kernel form: " + "; ".join(f"{name}: reading the map takes {e:.2f} x (eager) / {g:.2f} x (replayed) the time of evaluating it" for name, e, g in verdicts))
    if not a.lib:
        say("shapes where the device path loses: " + ("; ".join(losses) if losses else "none"))
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    text = "\n".join(lines) + "\n"
    out.write_text(out.read_text() + "\n" + text if a.append and out.exists() else text)


if __name__ == "__main__":
    main()
