#!/usr/bin/env python
"""Times mtgs_amd.brightness: adjust_brightness at 1920 x 1080 and 960 x 540 for C = 1 and C = 8 images, and
estimate_brightness_factors with 8 cameras of 1920 x 1080 and 120 000 points.

    adjust, shipped     one launch, 4 pixels per thread through dwords (the images are contiguous), eager and as a replayed HIP graph
    adjust, strided     the byte-by-byte kernel forced onto the same contiguous images, timed alternately with the shipped one
    torch on the device the same definition as a chain of torch ops on device tensors (integer tables gathered, float32 chain):
                        timed, and its bytes compared with ours for the record.  It is the device baseline because no OpenCV exists
                        here: a host OpenCV baseline (cv2.cvtColor twice + upload) is NOT measured
    host restatement    tests/brightness_refs.adjust_brightness in NumPy plus the upload of its result: a host baseline of this
                        project's own making, NOT OpenCV's speed
    estimate            three launches, eager and replayed; against the reference's formulation (matmul, grid_sample in fp64, masks,
                        the chain on the host with its host reads) in torch on the device and on the host

Device times are HIP events around windows of repeated calls (median of the windows); host times are wall clocks that end in a
synchronise.  The rate is the bytes the operator needs (every source byte once, every result byte once) over the event time, as a
share of the 8.0 TB/s HBM peak.  Writes profiles/brightness.txt.

    python scripts/brightness_bench.py [--out profiles/brightness.txt] [--windows 5]
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
sys.path.insert(0, str(ROOT / "scripts"))

from frame_bench import alternately, captured, device_ms, fmt, wall_ms  # noqa: E402
from mtgs_amd import brightness as M  # noqa: E402
from tests import brightness_refs as B  # noqa: E402
from tests import lidar_refs  # noqa: E402

HBM_PEAK = 8.0e12          # bytes per second, the specification
SHAPES = ((1080, 1920), (540, 960))
FACTORS = (1.0, 0.8, 1.25, 0.9, 1.1, 0.7, 1.4, 1.05)


def torch_adjust(images, factors, sdiv, hdiv):
    """the header's definition as torch ops on [C, h, w, 3] uint8 (rgb) and factors float64 [C]"""
    c = images.to(torch.int32)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    v, vmin = torch.maximum(r, torch.maximum(g, b)), torch.minimum(r, torch.minimum(g, b))
    d = v - vmin
    s = (d * sdiv[v.long()] + 2048) >> 12
    h = torch.where(v == r, g - b, torch.where(v == g, b - r + 2 * d, r - g + 4 * d))
    h = (h * hdiv[d.long()] + 2048) >> 12
    h = torch.where(h < 0, h + 180, h)
    v2 = torch.nan_to_num(v.to(torch.float64) * factors[:, None, None], nan=0.0).clamp(0.0, 255.0).trunc().to(torch.float32)
    hf, sf, vf = h.to(torch.float32) * np.float32(6.0 / 180.0), s.to(torch.float32) * (1.0 / 255.0), v2 * (1.0 / 255.0)
    fl = torch.floor(hf)
    f, sector = hf - fl, fl.long()
    tab = torch.stack([vf, vf * (1.0 - sf), vf * (1.0 - sf * f), vf * (1.0 - sf * (1.0 - f))], dim=-1)
    order = torch.tensor([[0, 3, 1], [2, 0, 1], [1, 0, 3], [1, 2, 0], [3, 1, 0], [0, 1, 2]], device=images.device)      # (r, g, b) per sector
    rgb = torch.gather(tab, -1, order[sector.clamp(0, 5)])
    rgb = torch.where((s == 0)[..., None], vf[..., None], rgb)
    return torch.round(rgb * 255.0).clamp(0, 255).to(torch.uint8)


def torch_estimate(points, mats, images, pairs, strip=100, min_overlap=10):
    """adjust_brightness_single_frame's formulation in torch fp64 on the tensors' device; the chain runs on the host as the
    reference's does, with one host read per pair"""
    C, h, w = images.shape[:3]
    xyz1 = torch.cat([points, torch.ones_like(points[:, :1])], dim=-1)
    p = (mats @ xyz1.T).transpose(1, 2)
    fov = p[..., 2] > 0.1
    uv = p[..., :2] / p[..., 2:3].clamp(1e-5, 99999) / torch.tensor([w, h], dtype=torch.float64, device=points.device)
    fov = fov & (uv[..., 0] < 1) & (uv[..., 0] >= 0) & (uv[..., 1] < 1) & (uv[..., 1] >= 0)
    imgs = images.to(torch.float64).permute(0, 3, 1, 2) / 255.0
    rgb = TF.grid_sample(imgs, (uv * 2 - 1).unsqueeze(2), align_corners=True, padding_mode="zeros").squeeze(3).permute(0, 2, 1)
    V = (rgb * 255).to(torch.uint8).amax(dim=-1).to(torch.float64)
    factor = {0: 1.0}
    for a, b, side in pairs:
        both = fov[a] & fov[b]
        if int(both.sum()) < min_overlap:
            sa, sb = (slice(None, strip), slice(-strip, None)) if side == 0 else (slice(-strip, None), slice(None, strip))
            ratio = float(images[a][:, sa].amax(dim=-1).double().mean() / images[b][:, sb].amax(dim=-1).double().mean())
        else:
            ratio = float(V[a][both].mean() / V[b][both].mean())
        ratio *= factor.get(a, 1.0)
        factor[b] = (factor[b] + ratio) / 2 if b in factor else ratio
    out = np.array([factor.get(c, 1.0) for c in range(C)])
    return out / np.mean(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "brightness.txt"))
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "brightness_bench needs a HIP device"
    dev = torch.device("cuda")
    rng = np.random.default_rng(7)
    lines = [f"brightness_bench: {torch.cuda.get_device_name(0)}; device times are HIP events, median of {a.windows} windows of >= 0.2 s (two "
             "forms timed alternately, 3 rounds: median, min and max of the rounds); host times are wall clocks that end in a synchronise",
             "the torch chain is the device baseline because no OpenCV exists here; a host OpenCV baseline is NOT measured.  The host "
             "restatement is this project's NumPy code, not OpenCV"]

    def say(line):
        print(line, flush=True)
        lines.append(line)

    sdiv, hdiv = (torch.from_numpy(t.astype(np.int32)).to(dev) for t in B.tables())
    for h, w in SHAPES:
        for C in (1, 8):
            host_images = rng.integers(0, 256, (C, h, w, 3), dtype=np.uint8)
            images, factors = torch.from_numpy(host_images).to(dev), torch.tensor(FACTORS[:C], dtype=torch.float64, device=dev)
            run = lambda: M.adjust_brightness(images, factors)
            strided = lambda: M.adjust_brightness(images, factors, _force_strided=True)
            as_float = lambda: M.adjust_brightness(images, factors, image_float=True)
            ours = run()
            assert torch.equal(ours, strided())
            nbytes = 6 * C * h * w
            rate = lambda t, n=nbytes: f"{n / 1e6:7.2f} MB -> {n / (t[0] * 1e-3) / 1e9:7.1f} GB/s = {100 * n / (t[0] * 1e-3) / HBM_PEAK:5.2f} % of the 8.0 TB/s HBM peak"
            eager, eager_strided = alternately([run, strided], a.windows)
            replay, keep = captured(run)
            replay_strided, keep_strided = captured(strided)
            graph, graph_strided = alternately([replay, replay_strided], a.windows)
            say(f"adjust {w}x{h} C={C}:")
            say(f"    dword path (shipped), eager   {fmt(eager)}   replayed graph {fmt(graph)}   {rate(graph)} (replayed)")
            say(f"    strided path forced, eager    {fmt(eager_strided)}   replayed graph {fmt(graph_strided)}   {rate(graph_strided)} (replayed)"
                f"   = {eager_strided[0] / eager[0]:.2f} x / {graph_strided[0] / graph[0]:.2f} x the dword path")
            t_float = device_ms(as_float, a.windows)
            say(f"    image_float (16-byte stores)  {fmt(t_float)}   {rate(t_float, 15 * C * h * w)} (eager)")
            theirs = torch_adjust(images, factors, sdiv, hdiv)
            differ = float((theirs != ours).any(dim=-1).float().mean())
            t_torch = device_ms(lambda: torch_adjust(images, factors, sdiv, hdiv), a.windows)
            say(f"    torch chain on the device     {fmt(t_torch)}   = {t_torch[0] / eager[0]:.1f} x adjust_brightness (eager); pixels that differ: {100 * differ:.4f} %")
            if C == 1:
                t_host = wall_ms(lambda: torch.from_numpy(B.adjust_brightness(host_images, np.array(FACTORS[:C]))).to(dev), 3)
                say(f"    host NumPy restatement + upload {fmt(t_host)}   = {t_host[0] / eager[0]:.0f} x adjust_brightness (eager)")
            del keep, keep_strided

    h, w, N = 1080, 1920, 120000
    yaws = (0.0, 55.0, -55.0, 110.0, -110.0, 165.0, -165.0, 180.0)
    pts = lidar_refs.sweep(rng, N)
    mats = np.stack([lidar_refs.camera(y, 1545.0, rng.uniform(-0.3, 0.3, 3), w, h)[0] for y in yaws])
    host_images = rng.integers(0, 256, (8, h, w, 3), dtype=np.uint8)
    d_pts, d_mats, d_images = torch.from_numpy(pts).to(dev), torch.from_numpy(mats).to(dev), torch.from_numpy(host_images).to(dev)
    run = lambda: M.estimate_brightness_factors(d_pts, d_mats, d_images, return_stats=True)
    factors, stats = run()
    eager = device_ms(run, a.windows)
    replay, keep = captured(run)
    graph = device_ms(replay, a.windows)
    say(f"estimate 8 x {w}x{h}, N={N}: overlap counts {stats[:, 0].tolist()}")
    say(f"    three launches, eager         {fmt(eager)}   replayed graph {fmt(graph)}")
    both = lambda: M.adjust_brightness(d_images, M.estimate_brightness_factors(d_pts, d_mats, d_images), "bgr")
    t_both = device_ms(both, a.windows)
    say(f"    estimate + adjust of the 8 images, eager {fmt(t_both)}")
    pairs = M.NUPLAN_PAIRS
    for name, (p, m, im) in (("device", (d_pts.double(), d_mats, d_images)), ("host", (torch.from_numpy(pts).double(), torch.from_numpy(mats), torch.from_numpy(host_images)))):
        try:
            theirs = torch_estimate(p, m, im, pairs)
            t = wall_ms(lambda: torch_estimate(p, m, im, pairs), 3)
            say(f"    reference's formulation in torch fp64 on the {name:6s} {fmt(t)} (wall)   = {t[0] / eager[0]:.0f} x ours (eager); "
                f"largest factor difference {float(np.abs(theirs - factors.cpu().numpy()).max()):.3g}")
        except Exception as e:                                         # an operator torch lacks for fp64 on this device: say so
            say(f"    reference's formulation in torch fp64 on the {name}: not measured ({type(e).__name__}: {e})")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
