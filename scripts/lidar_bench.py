#!/usr/bin/env python
"""Times mtgs_amd.lidar at the sizes a user runs: depth_image at 960 x 540 and 1920 x 1080 with a sweep of 120 000 points,
paint_points with 8 cameras of 1920 x 1080 and 200 000 points (one sweep) and 4 000 000 points (a stacked traversal).  Each against
two baselines on the same machine:

    host     the host formulation the operators replace -- NumPy: a matrix product, boolean filters, a fancy assignment; torch on the
             CPU: grid_sample in fp64, bilinear for the colours and nearest for the labels -- with the upload of its result
    torch    the same formulas as torch operations on device tensors: grid_sample in fp64, index_put_ for the scatter.  index_put_
             with repeated indices is NOT deterministic: the scatter baseline is timed only, its image is not compared

Device times are HIP events around windows of repeated calls (median of the windows); host times are a wall clock around work that
ends in a device synchronise.  The gather's achieved rate is the bytes the algorithm needs (computed from the counts below) over
the event time of mtgs_lidar_paint, against the HBM peak.  Writes profiles/lidar.txt.

    python scripts/lidar_bench.py [--out profiles/lidar.txt] [--host-max 4000000] [--windows 5]
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from mtgs_amd import lidar  # noqa: E402

HBM_PEAK = 8.0e12          # bytes per second, the specification; a float4 copy measures 6.29e12
HBM_COPY = 6.29e12


def camera(yaw_deg, f, offset, width, height):
    """(lidar -> image, lidar -> camera, K): a camera looking along (cos yaw, sin yaw, 0), x to its right, y down"""
    a = np.deg2rad(yaw_deg)
    E = np.eye(4)
    E[:3, :3] = [[np.sin(a), -np.cos(a), 0.0], [0.0, 0.0, -1.0], [np.cos(a), np.sin(a), 0.0]]
    E[:3, 3] = offset
    K = np.eye(4)
    K[0, 0] = K[1, 1] = f
    K[0, 2], K[1, 2] = width / 2, height / 2
    return K @ E, E, K[:3, :3]


def sweep(rng, n):
    """a street: most returns from the ground and the facades within 60 m, in the order a spinning sensor delivers them"""
    r, a = rng.uniform(2.0, 60.0, n), np.sort(rng.uniform(0.0, 2 * np.pi, n))
    return np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-2.0, 6.0, n)], -1).astype(np.float32)


# ---- the host formulation ---------------------------------------------------------------------------------------------------------
def host_depth(points, lidar2cam, K, width, height):
    homogeneous = np.concatenate([points, np.ones((points.shape[0], 1))], axis=1)
    cam = (homogeneous @ lidar2cam.T)[:, :3]
    uvz = cam[cam[:, 2] > 0] @ K.T
    uvz[:, :2] /= uvz[:, 2:]
    for column, bound in ((1, height), (0, width)):
        uvz = uvz[uvz[:, column] >= 0]
        uvz = uvz[uvz[:, column] < bound]
    uv = uvz[:, :2].astype(int)
    image = np.zeros((height, width), dtype=np.float32)
    image[uv[:, 1], uv[:, 0]] = uvz[:, 2]
    return image[:, :, None]


def projected(points, lidar2imgs, width, height, xp):
    """normalised coordinates [C, N, 2] and the field-of-view mask [C, N], in NumPy (xp = np) or torch (xp = torch)"""
    ones = xp.ones_like(points[:, :1])
    homogeneous = np.concatenate([points, ones], axis=-1) if xp is np else torch.cat([points, ones], dim=-1)
    p = lidar2imgs @ homogeneous.T
    p = p.transpose(0, 2, 1) if xp is np else p.permute(0, 2, 1)
    see = p[..., 2] > 0.1
    z = xp.clip(p[..., 2:3], 1e-5, 99999)
    size = np.array([width, height], dtype=np.float64) if xp is np else torch.tensor([width, height], dtype=torch.float64, device=points.device)
    n = p[..., :2] / z / size
    see = see & (n[..., 0] < 1) & (n[..., 0] >= 0) & (n[..., 1] < 1) & (n[..., 1] >= 0)
    return n, see


def sampled(n, see, images, masks):
    """grid_sample in fp64 on whatever device the tensors are on: colours averaged over the seeing cameras, the first one's label"""
    grid = (n * 2 - 1).unsqueeze(2)
    texels = images.to(torch.float64).flip(-1).permute(0, 3, 1, 2) / 255.0
    rgb = F.grid_sample(texels, grid, align_corners=True, padding_mode="zeros").squeeze(3).permute(0, 2, 1)
    rgb = torch.where(see[..., None], rgb, torch.zeros((), dtype=torch.float64, device=rgb.device)).sum(0)
    count = see.sum(0)
    rgb = rgb / count.clamp(min=1)[:, None]
    labels = F.grid_sample(masks.permute(0, 3, 1, 2).to(torch.float64), grid, mode="nearest", align_corners=True,
                           padding_mode="border").squeeze(3).squeeze(1).to(torch.int32)
    first = torch.argmax(see.to(torch.uint8), dim=0)
    labels = torch.where(count > 0, labels.gather(0, first[None])[0], torch.zeros((), dtype=torch.int32, device=labels.device))
    return rgb, labels, count > 0


def host_paint(points, lidar2imgs, images, masks, width, height):
    n, see = projected(points.astype(np.float64), lidar2imgs, width, height, np)
    return sampled(torch.from_numpy(n), torch.from_numpy(see), torch.from_numpy(images), torch.from_numpy(masks))


def torch_paint(points, lidar2imgs, images, masks, width, height):
    n, see = projected(points.to(torch.float64), lidar2imgs, width, height, torch)
    return sampled(n, see, images, masks)


def torch_depth(points, lidar2cam, K, width, height):
    homogeneous = torch.cat([points.to(torch.float64), torch.ones_like(points[:, :1], dtype=torch.float64)], dim=1)
    cam = (homogeneous @ lidar2cam.T)[:, :3]
    uvz = cam @ K.T
    u, v = uvz[:, 0] / uvz[:, 2], uvz[:, 1] / uvz[:, 2]
    keep = (cam[:, 2] > 0) & (v >= 0) & (v < height) & (u >= 0) & (u < width)
    image = torch.zeros((height, width), dtype=torch.float32, device=points.device)
    image.index_put_((v[keep].long(), u[keep].long()), uvz[keep, 2].to(torch.float32))       # repeated indices: not deterministic
    return image[:, :, None]


# ---- clocks ------------------------------------------------------------------------------------------------------------------------
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
    return f"{t[0]:10.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "lidar.txt"))
    ap.add_argument("--host-max", type=int, default=4_000_000, help="largest N the host formulation of paint_points is timed at")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--paint-sizes", type=int, nargs="+", default=[200_000, 4_000_000])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "lidar_bench needs a HIP device"
    dev = torch.device("cuda")
    rng = np.random.default_rng(7)
    lines = [f"lidar_bench: {torch.cuda.get_device_name(0)}; device times are HIP events, median of {a.windows} windows of >= 0.2 s; host times "
             "are wall clocks that end in a synchronise, upload of the result included",
             "the torch scatter baseline (index_put_ with repeated indices) is not deterministic: it is timed only, never compared"]

    def say(line):
        print(line, flush=True)
        lines.append(line)

    # ---- depth_image ----------------------------------------------------------------------------------------------------------------
    n = 120_000
    pts = sweep(rng, n)
    for width, height in ((960, 540), (1920, 1080)):
        _, E, K = camera(15.0, 1100.0 * width / 1920, (0.2, -0.1, 1.5), width, height)
        E32, K32 = E.astype(np.float32), K.astype(np.float32)
        p_d, E_d, K_d = torch.from_numpy(pts).to(dev), torch.from_numpy(E32).to(dev), torch.from_numpy(K32).to(dev)
        ours, index = lidar.depth_image(p_d, E_d, K_d, width, height, return_index=True)
        want = host_depth(pts, E32, K32, width, height)
        hits = int((index >= 0).sum())
        same = bool(np.array_equal(ours.cpu().numpy(), want))
        t_kernel = device_ms(lambda: lidar.depth_image(p_d, E_d, K_d, width, height), a.windows)
        t_upload = wall_ms(lambda: lidar.depth_image(torch.from_numpy(pts).to(dev), E_d, K_d, width, height), 20)
        t_host = wall_ms(lambda: torch.from_numpy(host_depth(pts, E32, K32, width, height)).to(dev), 5)
        E64, K64 = E_d.to(torch.float64), K_d.to(torch.float64)
        t_torch = device_ms(lambda: torch_depth(p_d, E64, K64, width, height), a.windows)
        say(f"depth_image {width}x{height} N={n}: {hits} pixels hit, equal to the host image: {same}")
        say(f"    mtgs_amd.lidar.depth_image          {fmt(t_kernel)}   with the sweep's upload {fmt(t_upload)}")
        say(f"    host (NumPy) + upload of the image  {fmt(t_host)}   = {t_host[0] / t_upload[0]:.1f} x the device path with its upload")
        say(f"    torch on the device (index_put_)    {fmt(t_torch)}   = {t_torch[0] / t_kernel[0]:.1f} x depth_image")
    # ---- paint_points ---------------------------------------------------------------------------------------------------------------
    width, height, C = 1920, 1080, 8
    mats = np.stack([camera(45.0 * c + 15.0, 1100.0, rng.uniform(-0.5, 0.5, 3) + (0, 0, 1.5), width, height)[0] for c in range(C)])
    images = rng.integers(0, 256, (C, height, width, 3), dtype=np.uint8)
    masks = rng.integers(0, 20, (C, height, width, 1), dtype=np.uint8)
    m_d, i_d, s_d = torch.from_numpy(mats).to(dev), torch.from_numpy(images).to(dev), torch.from_numpy(masks).to(dev)
    for n in a.paint_sizes:
        pts = sweep(rng, n)
        p_d = torch.from_numpy(pts).to(dev)
        ours = lidar.paint_points(p_d, m_d, i_d, s_d)
        pairs = int(ours.count.sum())
        t_kernel = device_ms(lambda: lidar.paint_points(p_d, m_d, i_d, s_d), a.windows)
        t_upload = wall_ms(lambda: lidar.paint_points(torch.from_numpy(pts).to(dev), m_d, i_d, s_d), 10)
        t_torch = device_ms(lambda: torch_paint(p_d, m_d, i_d, s_d, width, height), max(2, a.windows // 2))
        rgb_t, labels_t, fov_t = torch_paint(p_d, m_d, i_d, s_d, width, height)
        agree = (f"fov equal: {bool(torch.equal(fov_t, ours.fov))}, labels differ at {int((labels_t != ours.labels).sum())} points, "
                 f"max |rgb - torch| {float((rgb_t - ours.rgb).abs().max()):.3g}")
        del rgb_t, labels_t, fov_t
        torch.cuda.empty_cache()
        # bytes the algorithm needs: per point 12 in and 24 + 4 + 4 + 1 out; per seeing pair four 3-byte texels (+ 1 label byte for
        # the first); as 64-byte lines a pair touches at least two lines of the image
        useful = n * (12 + 33) + pairs * 12 + int(ours.fov.sum())
        lines64 = n * (12 + 33) + pairs * 2 * 64 + int(ours.fov.sum()) * 64
        say(f"paint_points C={C} {width}x{height} N={n}: {pairs} seeing (point, camera) pairs, {int(ours.fov.sum())} points seen; against torch on the device: {agree}")
        say(f"    mtgs_amd.lidar.paint_points         {fmt(t_kernel)}   with the cloud's upload {fmt(t_upload)}")
        say(f"    gather: {useful / 1e6:.1f} MB needed -> {useful / t_kernel[0] / 1e9 * 1e3:.1f} GB/s = {100 * useful / (t_kernel[0] * 1e-3) / HBM_PEAK:.2f} % of the 8.0 TB/s HBM peak "
            f"({100 * useful / (t_kernel[0] * 1e-3) / HBM_COPY:.2f} % of a 6.29 TB/s copy); as whole 64-byte lines {lines64 / 1e6:.1f} MB -> "
            f"{lines64 / t_kernel[0] / 1e9 * 1e3:.1f} GB/s = {100 * lines64 / (t_kernel[0] * 1e-3) / HBM_PEAK:.2f} % of the peak")
        say(f"    torch on the device (grid_sample)   {fmt(t_torch)}   = {t_torch[0] / t_kernel[0]:.1f} x paint_points")
        if n <= a.host_max:
            def host():
                rgb, labels, fov = host_paint(pts, mats, images, masks, width, height)
                return rgb.to(dev), labels.to(dev), fov.to(dev)
            t_host = wall_ms(host, 1 if n > 1_000_000 else 3)
            say(f"    host (NumPy + torch CPU grid_sample) + upload {fmt(t_host)}   = {t_host[0] / t_upload[0]:.1f} x the device path with its upload")
        del p_d, ours
        torch.cuda.empty_cache()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
