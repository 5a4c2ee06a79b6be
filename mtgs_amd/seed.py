"""Building a Gaussian node from a point cloud on the device.

VanillaGaussianSplattingModel.populate_modules (vanilla_gaussian_splatting.py:114-196) takes the mean distance to the three
nearest neighbours from scikit-learn on the host (k_nearest_sklearn, :372-390) and converts lidar normals to rotations in a
Python loop over rows (gaussian_model/utils.py:153-199).  Here the neighbour search is an exact octree walk over the
Morton-sorted cloud (`knn_distances`, mtgs_knn) and everything per point is one kernel (`seed_gaussians`, mtgs_seed_fwd);
`sky_points` is the sky dome's sampling (skybox_gaussian_splatting.py:51-91).  The dict `seed_gaussians` returns is keyed like a
checkpoint node (checkpoint.GAUSS_PARAM_NAMES).
"""
from __future__ import annotations

import math
from typing import Dict, Mapping, Optional

import torch
from torch import Tensor

from ._inputs import point_rows, row_stride
from ._lib import call, ptr, require_gpu, stream_of, workspace

MAX_K = 8


def num_sh_bases(degree: int) -> int:
    """gaussian_model/utils.py:72-81 (anything above 3 counts as 4)"""
    return (degree + 1) ** 2 if 0 <= degree <= 3 else 25


def knn_distances(points: Tensor, k: int = 3, return_indices: bool = False):
    """Distances [N, k] (float32, ascending) from every point to its k nearest OTHER points: sklearn's
    NearestNeighbors(n_neighbors=k + 1, metric="euclidean").kneighbors(points) without the first column.  Exact; duplicates give
    exact zeros; bitwise reproducible.  With return_indices also their indices [N, k] int64 (the smaller index first among equal
    distances).  Raises ValueError on non-finite coordinates and when N <= k, as sklearn does."""
    require_gpu(points)
    p = point_rows(points)
    N, k = p.shape[0], int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"k must be in [1, {MAX_K}], got {k}")
    if N <= k:
        raise ValueError(f"Expected n_neighbors <= n_samples_fit, but n_neighbors = {k + 1}, n_samples_fit = {N}")
    dev = p.device
    dist = torch.empty((N, k), dtype=torch.float32, device=dev)
    idx = torch.empty((N, k), dtype=torch.int32, device=dev) if return_indices else None
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws = workspace("mtgs_knn_workspace_bytes", N, k, device=dev, dtype=torch.uint8)
    call("mtgs_knn", N, k, ptr(p), row_stride(p), ptr(dist), ptr(idx), ptr(status), ptr(ws), ws.numel(), stream_of(p))
    if int(status.item()) != 0:
        raise ValueError("Input contains NaN or infinity: knn_distances needs finite coordinates")
    return (dist, idx.to(torch.int64)) if return_indices else dist


def random_quats(n: int, device, generator: Optional[torch.Generator] = None) -> Tensor:
    """random_quat_tensor (gaussian_model/utils.py:42-57) drawn on `device`"""
    u, v, w = (torch.rand(n, device=device, generator=generator) for _ in range(3))
    return torch.stack([torch.sqrt(1 - u) * torch.sin(2 * math.pi * v), torch.sqrt(1 - u) * torch.cos(2 * math.pi * v),
                        torch.sqrt(u) * torch.sin(2 * math.pi * w), torch.sqrt(u) * torch.cos(2 * math.pi * w)], dim=-1)


def _empty_node(sh_degree: int, scale_dim: int, features_dc_dim, device) -> Dict[str, Tensor]:
    """_skip_current_model -> __empty_gaussians(0, dim_sh) (vanilla_gaussian_splatting.py:198-217)"""
    z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=device)
    return {"means": z(0, 3), "scales": z(0, scale_dim), "quats": z(0, 4),
            "features_dc": z(0, 3) if features_dc_dim is None else z(0, features_dc_dim, 3),
            "features_rest": z(0, num_sh_bases(sh_degree) - 1, 3), "opacities": z(0, 1)}


def seed_gaussians(points_3d: Mapping[str, Tensor], sh_degree: int, scale_dim: int = 3, features_dc_dim: Optional[int] = None,
                   num_traversals: Optional[int] = None, multi_feature_rest: bool = False,
                   generator: Optional[torch.Generator] = None) -> Dict[str, Tensor]:
    """populate_modules of a vanilla node (num_traversals None), a multi-colour node (multi_color_gaussian_splatting.py:48-71)
    or a rigid node with Fourier colours (features_dc_dim > 1: features_dc [N, D, 3] with row 0 filled).
    points_3d: {"xyz" [N, 3], "rgb" [N, 3] in 0..255, "normals" [N, 3] (optional)} on the device.  Returns the node's parameters
    under checkpoint.GAUSS_PARAM_NAMES: means, scales [N, scale_dim], quats (scale_dim 3 only: from the normals, or random
    rotations drawn with `generator`), features_dc, features_rest (zeros [N, K - 1, 3], or [N, T, K - 1, 3] with
    multi_feature_rest), opacities [N, 1], features_adapters (zeros [N, T, 3] with num_traversals).  N = 0 gives the reference's
    empty node."""
    if scale_dim not in (1, 3):
        raise ValueError(f"scale_dim must be 1 or 3, got {scale_dim}")
    if features_dc_dim is not None and features_dc_dim <= 1:
        raise ValueError(f"invalid features_dc_dim [{features_dc_dim}], must be set to `None` or larger than 1")
    xyz, rgb = points_3d["xyz"], points_3d["rgb"]
    normals = points_3d.get("normals")
    N, dev = xyz.shape[0], xyz.device
    if N == 0:
        return _empty_node(sh_degree, scale_dim, features_dc_dim, dev)
    require_gpu(xyz, rgb, normals)
    if rgb.shape != (N, 3) or (normals is not None and normals.shape != (N, 3)):
        raise ValueError("rgb and normals must be [N, 3] like xyz")
    f32 = lambda t: t.detach().to(torch.float32).contiguous()
    K, k = num_sh_bases(sh_degree), 3
    dist = knn_distances(xyz, k)
    z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
    out = {"means": f32(xyz), "scales": torch.empty((N, scale_dim), dtype=torch.float32, device=dev)}
    with_normals = normals is not None and scale_dim == 3
    if scale_dim == 3:
        out["quats"] = torch.empty((N, 4), dtype=torch.float32, device=dev) if with_normals else random_quats(N, dev, generator)
    out["features_dc"] = z(N, 3) if features_dc_dim is None else z(N, features_dc_dim, 3)
    out["features_rest"] = z(N, num_traversals, K - 1, 3) if (num_traversals is not None and multi_feature_rest) else z(N, K - 1, 3)
    out["opacities"] = torch.empty((N, 1), dtype=torch.float32, device=dev)
    rgb_c = f32(rgb)
    nrm_c = f32(normals) if with_normals else None
    call("mtgs_seed_fwd", N, k, ptr(dist), ptr(rgb_c), ptr(nrm_c), int(sh_degree), int(scale_dim), ptr(out["scales"]),
         ptr(out["quats"]) if with_normals else None, ptr(out["features_dc"]), out["features_dc"].stride(0), ptr(out["opacities"]),
         stream_of(dist))
    if num_traversals is not None:
        out["features_adapters"] = z(N, num_traversals, 3)
    return out


def sky_radius(skybox_radius: float, max_distance: float) -> float:
    """skybox_gaussian_splatting.py:51-59: a dome closer than ten scene extents is pushed out to at least two"""
    return max(skybox_radius, max_distance * 2) if skybox_radius < max_distance * 10 else skybox_radius


def sky_points(num: int, skybox_radius: float, max_distance: float, skybox_type: str = "spheric", generator: Optional[torch.Generator] = None,
               device="cuda") -> Dict[str, Tensor]:
    """The sky dome's point cloud (skybox_gaussian_splatting.py:51-91): radii by `skybox_type` ("spheric": on the sphere,
    "volumetric": uniform in [0, R), anything else: uniform in [max_distance, R)), theta uniform in [0, 2 pi), phi uniform in
    [pi / 4, pi / 2], white colour.  Drawn on `device` with `generator`; seed_gaussians(sky_points(...), ...) is the sky node."""
    R = sky_radius(skybox_radius, max_distance)
    rand = lambda: torch.rand(num, device=device, generator=generator)
    if skybox_type == "spheric":
        radii = torch.ones(num, device=device) * R
    elif skybox_type == "volumetric":
        radii = rand() * R
    else:
        radii = max_distance + rand() * (R - max_distance)
    theta = rand() * 2 * math.pi
    phi = rand() * math.pi / 4 + math.pi / 4
    xyz = torch.stack([radii * torch.sin(phi) * torch.cos(theta), radii * torch.sin(phi) * torch.sin(theta), radii * torch.cos(phi)], dim=-1)
    return {"xyz": xyz, "rgb": torch.ones((num, 3), device=device) * 255}
