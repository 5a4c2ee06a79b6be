"""Preparing the seeding point cloud on the device.

NuPlanDataparser._load_3D_points (mtgs/dataset/nuplan_dataparser.py:460-500) stacks the lidar clouds of every traversal, runs
open3d's remove_statistical_outlier(nb_neighbors=20, std_ratio=0.5) and voxel_down_sample(voxel_size=0.15) on the host, appends
the SfM cloud, applies the dataparser transform and scale and quantises the colours.  Here the two open3d operators are device
kernels (`statistical_outlier_removal`, mtgs_cloud_outlier: the exact neighbour search of `seed.knn_distances` with up to 31
neighbours; `voxel_down_sample`, mtgs_cloud_voxel) and `prepare_seed_cloud` is the whole function: what it returns goes
straight into `seed.seed_gaussians`.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
from torch import Tensor

from ._inputs import point_rows, row_stride
from ._lib import call, ptr, require_gpu, stream_of, workspace

MIN_NB_NEIGHBORS, MAX_NB_NEIGHBORS = 2, 32
_AXES = "xyz"


def statistical_outlier_removal(points: Tensor, nb_neighbors: int = 20, std_ratio: float = 0.5, return_stats: bool = False):
    """open3d's PointCloud.remove_statistical_outlier as a mask: keep [N] bool on the device, True where the point stays.
    avg[i] is the mean distance of a k-neighbour query against the cloud itself, k = min(nb_neighbors, N), which returns point
    i at distance 0: (the sum of the distances to the k - 1 nearest other points) / k.  keep = avg > 0 and avg < cloud_mean +
    std_ratio * std over the cloud (open3d's definitions: the sums run over avg > 0, the divisors are N and N - 1).  A point with
    k - 1 exact duplicates has avg = 0 and is dropped; N = 1 keeps nothing.  Exact and bitwise reproducible.
    With return_stats also (avg [N] float64, {"cloud_mean", "std", "threshold", "valid"} as a float64 tensor [4]).
    Raises ValueError on non-finite coordinates."""
    require_gpu(points)
    p = point_rows(points)
    N, nb = p.shape[0], int(nb_neighbors)
    if not MIN_NB_NEIGHBORS <= nb <= MAX_NB_NEIGHBORS:
        raise ValueError(f"nb_neighbors must be in [{MIN_NB_NEIGHBORS}, {MAX_NB_NEIGHBORS}], got {nb}")
    dev = p.device
    avg = torch.empty(N, dtype=torch.float64, device=dev)
    stats = torch.full((4,), float("nan"), dtype=torch.float64, device=dev)
    keep = torch.empty(N, dtype=torch.uint8, device=dev)
    if N > 0:
        status = torch.empty(1, dtype=torch.int32, device=dev)
        ws = workspace("mtgs_cloud_outlier_workspace_bytes", N, nb, device=dev, dtype=torch.uint8)
        call("mtgs_cloud_outlier", N, nb, float(std_ratio), ptr(p), row_stride(p), ptr(avg), ptr(stats), ptr(keep),
             ptr(status), ptr(ws), ws.numel(), stream_of(p))
        if int(status.item()) != 0:
            raise ValueError("Input contains NaN or infinity: statistical_outlier_removal needs finite coordinates")
    keep = keep.to(torch.bool)
    return (keep, avg, stats) if return_stats else keep


def voxel_down_sample(points: Tensor, colors: Tensor, voxel_size: float, return_keys: bool = False):
    """open3d's PointCloud.voxel_down_sample: (xyz [M, 3] float64, rgb [M, 3] float64 in [0, 1], counts [M] int32), one row per
    occupied voxel.  The voxel of a point is floor((p - (min_bound - voxel_size / 2)) / voxel_size) per axis in fp64; a row is
    the mean of its points, summed in fp64 in the order of the input rows and divided once, bit for bit what open3d's
    AccumulatedPoint computes.  colors [N, 3]: uint8 (a channel is c / 255) or floating point in [0, 1] (read as float32).
    The rows come in ascending order of the packed voxel index (x << 42 | y << 21 | z), which is deterministic; open3d's order is
    the iteration order of a hash map and nothing downstream depends on it.  With return_keys also those packed indices [M]
    int64.  One host synchronisation (M).  Raises ValueError on non-finite coordinates and when the extent of an axis needs
    more than 2^21 voxels."""
    require_gpu(points, colors)
    p = point_rows(points)
    N, dev = p.shape[0], p.device
    vs = float(voxel_size)
    if not (vs > 0.0 and vs != float("inf")):
        raise ValueError(f"voxel_size must be positive and finite, got {voxel_size}")
    if colors.shape != (N, 3):
        raise ValueError(f"colors must be [N, 3] like points, got {tuple(colors.shape)}")
    c = colors.detach()
    if c.dtype != torch.uint8:
        c = c.to(torch.float32)
    c = c.contiguous()
    xyz = torch.empty((N, 3), dtype=torch.float64, device=dev)
    rgb = torch.empty((N, 3), dtype=torch.float64, device=dev)
    counts = torch.empty(N, dtype=torch.int32, device=dev)
    keys = torch.empty(N, dtype=torch.int64, device=dev) if return_keys else None
    M = 0
    if N > 0:
        ctl = torch.empty(2, dtype=torch.int32, device=dev)             # n_voxels, status: read together
        ws = workspace("mtgs_cloud_voxel_workspace_bytes", N, device=dev, dtype=torch.uint8)
        call("mtgs_cloud_voxel", N, vs, ptr(p), row_stride(p), ptr(c), int(c.dtype == torch.uint8), ptr(xyz), ptr(rgb),
             ptr(counts), ptr(keys), ctl.data_ptr(), ctl.data_ptr() + 4, ptr(ws), ws.numel(), stream_of(p))
        M, status = (int(v) for v in ctl.tolist())
        if status & 1:
            raise ValueError("Input contains NaN or infinity: voxel_down_sample needs finite coordinates")
        if status:
            axes = ", ".join(_AXES[a] for a in range(3) if status & (2 << a))
            raise ValueError(f"voxel_size {vs} is too small for the extent of the cloud: the voxel index of axis {axes} needs more than 21 bits")
    out = (xyz[:M].clone(), rgb[:M].clone(), counts[:M].clone())
    return out + (keys[:M].clone(),) if return_keys else out


def prepare_seed_cloud(lidar_xyz: Tensor, lidar_rgb: Tensor, sfm_xyz: Optional[Tensor] = None, sfm_rgb: Optional[Tensor] = None,
                       transform: Optional[Tensor] = None, scale_factor: float = 1.0, nb_neighbors: int = 20, std_ratio: float = 0.5,
                       voxel_size: float = 0.15, generator: Optional[torch.Generator] = None) -> Dict[str, Tensor]:
    """_load_3D_points end to end: the stacked lidar cloud (lidar_xyz [N, 3], lidar_rgb [N, 3] uint8 or float in [0, 1]) is
    filtered (`statistical_outlier_removal`) and down-sampled (`voxel_down_sample`); the SfM cloud (optional, same formats) is
    appended unfiltered; positions become float32, xyz @ transform[:3, :3].T + transform[:3, 3] (transform [3 or 4, 4],
    optional) times scale_factor; colours become (rgb * 255).to(uint8), which truncates.  Returns {"xyz": float32 [P, 3], "rgb":
    uint8 [P, 3]} on the device of the input, the points_3d of `seed.seed_gaussians`.  When nothing is left the reference's
    fallback cloud is returned: 200 standard-normal points (drawn with `generator`) with black colours."""
    require_gpu(lidar_xyz, lidar_rgb, sfm_xyz, sfm_rgb, transform)
    if (sfm_xyz is None) != (sfm_rgb is None):
        raise ValueError("sfm_xyz and sfm_rgb go together")
    dev = lidar_xyz.device
    if lidar_xyz.shape[0] > 0:
        keep = statistical_outlier_removal(lidar_xyz, nb_neighbors, std_ratio)
        xyz, rgb, _ = voxel_down_sample(lidar_xyz[keep], lidar_rgb[keep], voxel_size)
    else:
        xyz, rgb = (torch.zeros((0, 3), dtype=torch.float64, device=dev) for _ in range(2))
    if sfm_xyz is not None and sfm_xyz.shape[0] > 0:
        if sfm_rgb.shape != sfm_xyz.shape:
            raise ValueError("sfm_rgb must be [N, 3] like sfm_xyz")
        s_rgb = sfm_rgb.to(torch.float64)
        if sfm_rgb.dtype == torch.uint8:
            # a true division: by a Python scalar torch multiplies with the rounded reciprocal, and (c * (1 / 255)) * 255 can
            # truncate to c - 1, where (c / 255) * 255 truncates back to c for every c
            s_rgb = s_rgb / torch.full_like(s_rgb, 255.0)
        xyz = torch.cat([xyz, sfm_xyz.to(torch.float64)])
        rgb = torch.cat([rgb, s_rgb])
    xyz = xyz.to(torch.float32)
    if transform is not None:
        t = transform.to(torch.float32)
        xyz = xyz @ t[:3, :3].T + t[:3, 3]
    xyz = xyz * scale_factor
    rgb = (rgb * 255).to(torch.uint8)
    if xyz.shape[0] == 0:
        xyz = torch.randn((200, 3), device=dev, generator=generator)
        rgb = torch.zeros((200, 3), dtype=torch.uint8, device=dev)
    return {"xyz": xyz, "rgb": rgb}
