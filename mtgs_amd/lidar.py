"""Lidar sweeps through the cameras on the device (include/mtgs_lidar.h, csrc/lidar.hip).

The lidar sweep was the one per-frame input that still took a NumPy detour on the host, twice.  `depth_image` is
CustomInputDataset._get_depth_from_lidar (mtgs/dataset/custom_dataset.py:175-201), the sparse depth image every shipped config
loads for every frame: the sweep is uploaded (about 1 MB) instead of the H x W image (8 MB at 1920 x 1080), and the scatter's
duplicates are resolved as NumPy's assignment resolves them -- the last point wins -- by an integer atomicMax of the point index,
which `index_put_` with repeated indices does not promise.  `paint_points` is get_rgb_point_cloud (mtgs/utils/
nuplan_pointcloud.py:28-60) and get_semantic_point_cloud (nuplan_scripts/utils/nuplan_utils_custom.py:208-265) in one launch: the
colours and labels of the cloud that `pointcloud.prepare_seed_cloud` starts from.

    depth_image(points, lidar2cam, K, width, height, scale=1.0, return_index=False)   -> float32 [H, W, 1] (, int32 [H, W])
    paint_points(points, lidar2imgs, images=None, sem_masks=None, channel_order="bgr") -> PaintedPoints(rgb, labels, fov, count)

All arithmetic is fp64 in the order include/mtgs_lidar.h states; tests/lidar_refs.py restates it in NumPy.  Neither operator reads
anything back to the host, both are bitwise reproducible and can be captured in a HIP graph.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch
from torch import Tensor

from . import _abi
from ._inputs import point_rows, row_stride, shape_of
from ._lib import call, ptr, require_gpu, stream_of, workspace

MAX_CAMERAS = _abi.header_abi("mtgs_lidar.h").constants["MTGS_LIDAR_MAX_CAMERAS"]
_FLOATS = (torch.float32, torch.float64)


class PaintedPoints(NamedTuple):
    """What `paint_points` returns: rgb float64 [N, 3] in [0, 1] (None without images), labels int32 [N] (None without masks),
    fov bool [N], count int32 [N] (the number of cameras that see the point)."""
    rgb: Optional[Tensor]
    labels: Optional[Tensor]
    fov: Tensor
    count: Tensor


def _sweep(points: Tensor) -> Tensor:
    """the rows of a sweep in their own precision (_inputs.point_rows), fewer than 2^31 of them"""
    p = point_rows(points, _FLOATS, convert=False)
    if p.shape[0] >= 1 << 31:
        raise ValueError(f"points must have fewer than 2^31 rows, got {tuple(points.shape)}")
    return p


def _check_matrix(m, name: str, batched: bool) -> None:
    want = "[C, 4, 4] or [C, 3, 4]" if batched else "[4, 4] or [3, 4]"
    if not isinstance(m, Tensor) or m.dim() != 2 + batched or tuple(m.shape[-2:]) not in ((4, 4), (3, 4)):
        raise ValueError(f"{name} must be {want}, got {shape_of(m)}")
    if m.dtype not in _FLOATS:
        raise TypeError(f"{name} must be float32 or float64, got {m.dtype}")


def _rows34(m: Tensor) -> Tensor:
    """the top three rows as contiguous float64 (a float32 value converts exactly)"""
    return m.detach()[..., :3, :].to(torch.float64).contiguous()


def _size(width, height) -> None:
    for name, v in (("width", width), ("height", height)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f"{name} must be a positive integer, got {v!r}")
    if width * height >= 1 << 31:
        raise ValueError(f"width * height must be below 2^31, got {width} x {height}")


def depth_image(points: Tensor, lidar2cam: Tensor, K: Tensor, width: int, height: int, scale: float = 1.0, return_index: bool = False):
    """The sparse lidar depth image [H, W, 1] float32 of `_get_depth_from_lidar`: points [N, 3] (float32 or float64, a row stride is
    kept) through lidar2cam ([4, 4] or [3, 4]) and the full intrinsic matrix K [3, 3]; a point in front of the camera whose (u, v)
    lies in [0, W) x [0, H) writes its depth at ((int)u, (int)v); among the points of one pixel the LARGEST index wins (NumPy's
    assignment); the image is multiplied by `scale` in float32; pixels without a point are 0.  A non-finite point writes nothing.
    With return_index also the winning point's index, int32 [H, W], -1 where no point landed.  N = 0 gives zeros."""
    p = _sweep(points)
    _check_matrix(lidar2cam, "lidar2cam", False)
    if not isinstance(K, Tensor) or tuple(K.shape) != (3, 3):
        raise ValueError(f"K must be [3, 3], got {shape_of(K)}")
    if K.dtype not in _FLOATS:
        raise TypeError(f"K must be float32 or float64, got {K.dtype}")
    _size(width, height)
    require_gpu(points, lidar2cam, K)
    dev, N = p.device, p.shape[0]
    m, k = _rows34(lidar2cam), K.detach().to(torch.float64).contiguous()
    depth = torch.empty((height, width, 1), dtype=torch.float32, device=dev)
    index = torch.empty((height, width), dtype=torch.int32, device=dev) if return_index else None
    ws = workspace("mtgs_lidar_depth_workspace_bytes", height, width, device=dev, dtype=torch.uint8)
    call("mtgs_lidar_depth", N, ptr(p) if N else None, int(p.dtype == torch.float64), row_stride(p), ptr(m), ptr(k),
         height, width, float(scale), ptr(depth), ptr(index), ptr(ws), ws.numel(), stream_of(p))
    return (depth, index) if return_index else depth


def paint_points(points: Tensor, lidar2imgs: Tensor, images: Optional[Tensor] = None, sem_masks: Optional[Tensor] = None,
                 channel_order: str = "bgr") -> PaintedPoints:
    """Colours and semantic labels of a cloud from C cameras of one size: points [N, 3] through lidar2imgs ([C, 4, 4] or [C, 3, 4],
    intrinsics included).  images uint8 [C, H, W, 3] are sampled bilinearly (align_corners) and averaged over the cameras that see
    the point, in camera order: rgb float64 [N, 3] in [0, 1], the format `pointcloud.prepare_seed_cloud` takes; channel_order "bgr"
    (cv2.imread's, the reference's) reverses the channels, "rgb" keeps them.  sem_masks uint8 [C, H, W, 1] or [C, H, W] are read at
    the nearest texel (ties to even) of the FIRST camera that sees the point: labels int32 [N], 0 where none does.  fov = count >
    0.  One of the two inputs may be missing; the projection is done once for both."""
    p = _sweep(points)
    _check_matrix(lidar2imgs, "lidar2imgs", True)
    C = lidar2imgs.shape[0]
    if not 1 <= C <= MAX_CAMERAS:
        raise ValueError(f"lidar2imgs must hold 1 to {MAX_CAMERAS} cameras, got {tuple(lidar2imgs.shape)}")
    if channel_order not in ("bgr", "rgb"):
        raise ValueError(f"channel_order must be 'bgr' or 'rgb', got {channel_order!r}")
    size = None
    if images is not None:
        if not isinstance(images, Tensor) or images.dim() != 4 or images.shape[0] != C or images.shape[3] != 3:
            raise ValueError(f"images must be [C, H, W, 3] with C = {C}, got {shape_of(images)}")
        if images.dtype != torch.uint8:
            raise TypeError(f"images must be uint8, got {images.dtype}")
        size = tuple(images.shape[1:3])
    if sem_masks is not None:
        ok = isinstance(sem_masks, Tensor) and sem_masks.shape[0:1] == (C,) and (sem_masks.dim() == 3 or (sem_masks.dim() == 4 and sem_masks.shape[3] == 1))
        if not ok:
            raise ValueError(f"sem_masks must be [C, H, W, 1] or [C, H, W] with C = {C}, got {shape_of(sem_masks)}")
        if sem_masks.dtype != torch.uint8:
            raise TypeError(f"sem_masks must be uint8, got {sem_masks.dtype}")
        if size is not None and tuple(sem_masks.shape[1:3]) != size:
            raise ValueError(f"images and sem_masks must have one size, got {tuple(images.shape)} and {tuple(sem_masks.shape)}")
        size = tuple(sem_masks.shape[1:3])
    if size is None:
        raise ValueError("paint_points needs images or sem_masks: the size of the cameras' images comes from them")
    h, w = size
    _size(w, h)
    require_gpu(points, lidar2imgs, images, sem_masks)
    dev, N = p.device, p.shape[0]
    m = _rows34(lidar2imgs)
    img = images.detach().contiguous() if images is not None else None
    msk = sem_masks.detach().contiguous() if sem_masks is not None else None
    rgb = torch.empty((N, 3), dtype=torch.float64, device=dev) if img is not None else None
    labels = torch.empty(N, dtype=torch.int32, device=dev) if msk is not None else None
    fov = torch.empty(N, dtype=torch.bool, device=dev)
    count = torch.empty(N, dtype=torch.int32, device=dev)
    if N > 0:
        call("mtgs_lidar_paint", N, ptr(p), int(p.dtype == torch.float64), row_stride(p), C, ptr(m), h, w, ptr(img),
             int(channel_order == "bgr"), ptr(msk), ptr(rgb), ptr(labels), ptr(fov), ptr(count), stream_of(p))
    return PaintedPoints(rgb, labels, fov, count)
