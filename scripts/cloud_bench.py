#!/usr/bin/env python
"""Times mtgs_amd.pointcloud on a street-like stacked lidar cloud at N = 2 M and 10 M: the outlier filter (mtgs_cloud_outlier),
the voxel grid (mtgs_cloud_voxel) and prepare_seed_cloud (both, plus the transform), against the host pipeline they replace --
scipy.spatial.cKDTree (k = 20, every CPU the job has) for open3d's k-d tree and a NumPy voxel grid (np.add.at: the same
sequential fp64 sums).  Writes profiles/cloud_bench.txt.

    python scripts/cloud_bench.py [--sizes 2000000 10000000] [--host-max 10000000] [--out profiles/cloud_bench.txt]
"""
import argparse
import os
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from mtgs_amd import _lib, pointcloud  # noqa: E402


def street_cloud(n, seed, dev):
    """stacked traversals of a 400 m road: a thin dense ground strip, two facades, sparse clutter above"""
    g = torch.Generator(device=dev).manual_seed(seed)
    u = lambda m, lo, hi: torch.rand(m, device=dev, generator=g) * (hi - lo) + lo
    nrm = lambda m, s: torch.randn(m, device=dev, generator=g) * s
    n_g, n_w = n // 2, n // 4
    n_c = n - n_g - n_w
    ground = torch.stack([u(n_g, 0, 400), u(n_g, -8, 8), nrm(n_g, 0.02)], -1)
    side = torch.where(torch.rand(n_w, device=dev, generator=g) < 0.5, -8.0, 8.0)
    walls = torch.stack([u(n_w, 0, 400), side + nrm(n_w, 0.03), u(n_w, 0, 6)], -1)
    clutter = torch.stack([u(n_c, -20, 420), u(n_c, -30, 30), u(n_c, 0, 15)], -1)
    x = torch.cat([ground, walls, clutter])
    return x[torch.randperm(n, device=dev, generator=g)].contiguous()


def wall(fn, reps):
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best * 1e3, out


def host_pipeline(x, c, workers):
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    p = x.astype(np.float64)
    d, _ = cKDTree(p).query(p, k=20, workers=workers)
    avg = d.sum(axis=1) / 20
    pos = avg > 0
    mean = avg[pos].sum() / avg.shape[0]
    std = np.sqrt(((avg[pos] - mean) ** 2).sum() / (avg.shape[0] - 1))
    keep = pos & (avg < mean + 0.5 * std)
    t1 = time.perf_counter()
    p, cc = p[keep], c[keep].astype(np.float64) / 255.0
    index = np.floor((p - (p.min(axis=0) - 0.15 * 0.5)) / 0.15).astype(np.int64)
    key = index[:, 0] << 42 | index[:, 1] << 21 | index[:, 2]
    uniq, inv, counts = np.unique(key, return_inverse=True, return_counts=True)
    acc = np.zeros((uniq.shape[0], 6))
    np.add.at(acc, inv, np.concatenate([p, cc], axis=1))
    acc /= counts[:, None]
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, int(keep.sum()), uniq.shape[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[2_000_000, 10_000_000])
    ap.add_argument("--host-max", type=int, default=10_000_000, help="largest N the host pipeline is timed at")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "cloud_bench.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "cloud_bench needs a HIP device"
    dev = torch.device("cuda")
    workers = int(os.environ.get("OMP_NUM_THREADS", "16"))
    small = street_cloud(4096, 1, dev)
    pointcloud.prepare_seed_cloud(small, torch.zeros(4096, 3, dtype=torch.uint8, device=dev))      # loads the code objects
    lines = []
    for n in a.sizes:
        x = street_cloud(n, 7, dev)
        c = torch.randint(0, 256, (n, 3), device=dev, generator=torch.Generator(device=dev).manual_seed(3)).to(torch.uint8)
        _lib.time_calls(("mtgs_cloud_outlier", "mtgs_cloud_voxel"))
        t_out, keep = wall(lambda: pointcloud.statistical_outlier_removal(x), a.reps)
        xk, ck = x[keep], c[keep]
        t_vox, vox = wall(lambda: pointcloud.voxel_down_sample(xk, ck, 0.15), a.reps)
        torch.cuda.synchronize()
        ev = {k: min(v) for k, v in _lib.timed_ms().items()}
        _lib.time_calls(())
        t_all, out = wall(lambda: pointcloud.prepare_seed_cloud(x, c), a.reps)
        line = (f"street N={n:9d}  outlier filter {t_out:9.2f} ms wall (mtgs_cloud_outlier {ev['mtgs_cloud_outlier']:9.2f} ms)   "
                f"voxel grid {t_vox:8.2f} ms wall (mtgs_cloud_voxel {ev['mtgs_cloud_voxel']:8.2f} ms, {xk.shape[0]} -> {vox[0].shape[0]})   "
                f"prepare_seed_cloud {t_all:9.2f} ms wall -> {out['xyz'].shape[0]} points")
        if n <= a.host_max:
            h_out, h_vox, h_keep, h_m = host_pipeline(x.cpu().numpy(), c.cpu().numpy(), workers)
            assert h_keep == xk.shape[0] or abs(h_keep - xk.shape[0]) <= 1e-5 * n, (h_keep, xk.shape[0])
            line += (f"   host ({workers} CPUs): cKDTree k=20 + statistics {h_out:10.1f} ms, NumPy voxel grid {h_vox:9.1f} ms, "
                     f"together {h_out + h_vox:10.1f} ms ({h_keep} -> {h_m})")
        print(line, flush=True)
        lines.append(line)
        del x, c, xk, ck, vox, out, keep
        torch.cuda.empty_cache()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
