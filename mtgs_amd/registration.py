"""Lidar sweeps registered across traversals on the device (include/mtgs_icp.h, csrc/icp.hip).

Every data-preparation stage consumes `lidar2global`; in the reference that pose comes from
nuplan_scripts/lidar_registration_multi_traversal.py, a KISS-ICP run (thirdparty/kiss-icp, with MTGS's warm-up from the log pose at the
start of each traversal) over the sweeps of all traversals of a road block.  Here the sweep is down-sampled, matched against a voxel
map and the map updated on the device; the pose, the adaptive threshold and the motion model stay on the host, as fp64 NumPy.

    KissConfig(max_range, ...)                                    the reference's data / mapping / registration / threshold settings
    downsample(points, config)                                    -> Downsampled(frame, source, counts, status, frame_index, source_index)
    VoxelMap(voxel_size, max_points_per_voxel=20, capacity=...)   insert / prune / point_cloud / empty / check
    associate(source, map, max_distance, kernel)                  -> Association: one association and its 28 sums
    align_points_to_map(source, map, initial_guess, max_distance, kernel, ...) -> (pose [4, 4], iterations)
    LidarOdometry(config).register_frame(points, log_pose, traj_id) -> pose [4, 4]
    register_traversals(scans, log_poses, traj_ids, config)       -> (poses [F, 4, 4], iterations [F])
    align_poses(original, registered), registration_errors(...)   the BEV fit and the errors that decide which traversals are kept

kiss-icp itself cannot be built where this project is tested (Eigen, Sophus, TBB, tsl::robin_map), and it is not reproducible: it
returns a down-sampled cloud in the iteration order of a hash map and sums under tbb::parallel_reduce.  This module follows a canonical
order instead (include/mtgs_icp.h): a down-sampled cloud is in ascending input index, points are offered to the map in that order, sums
have a fixed tree.  tests/icp_refs.py restates it in NumPy; the device equals it bit for bit up to sin / cos, and repeats itself bit
for bit.  Two defined deviations: the LDL^T does not pivot, and an iteration without a correspondence (or with a non-finite step)
stops with `DEGENERATE` and the last good pose, where the reference would go on with NaN.

Out of scope: deskewing (MTGS passes deskew=False), .pcd parsing and `only_top`, `filter_semantic` (off by default;
`lidar.paint_points` yields the labels), the map plots, the scene pickle.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from . import _abi
from ._inputs import point_rows, row_stride, shape_of
from ._lib import call, ptr, require_gpu, size_query, stream_of, workspace

_ABI = _abi.header_abi("mtgs_icp.h")
MAX_POINTS = _ABI.constants["MTGS_ICP_MAX_POINTS"]
RECORD = _ABI.constants["MTGS_ICP_RECORD"]
SUMS = _ABI.constants["MTGS_ICP_SUMS"]
OUT_OF_GRID, MAP_FULL = _ABI.constants["MTGS_ICP_OUT_OF_GRID"], _ABI.constants["MTGS_ICP_MAP_FULL"]
CONVERGED, DEGENERATE, EMPTY_MAP = (_ABI.constants[n] for n in ("MTGS_ICP_CONVERGED", "MTGS_ICP_DEGENERATE", "MTGS_ICP_EMPTY_MAP"))
_FLOATS = (torch.float32, torch.float64)
# Iterations launched between two reads of the record.  The launches behind a converged iteration return at their first instruction,
# so a larger group costs idle launches and a smaller one costs reads; scripts/icp_bench.py times the choices.
GROUP_SIZE = 8


@dataclass
class KissConfig:
    """kiss_icp.config's fields as MTGS uses them.  voxel_size None: max_range / 100.  The map keeps points within 2 max_range."""
    max_range: float
    min_range: float = 5.0
    voxel_size: Optional[float] = None
    max_points_per_voxel: int = 20
    max_num_iterations: int = 500
    convergence_criterion: float = 1e-4
    initial_threshold: float = 2.0
    min_motion_th: float = 0.1

    def __post_init__(self):
        for name in ("max_range", "min_range", "convergence_criterion", "initial_threshold", "min_motion_th"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
                raise ValueError(f"{name} must be a finite number >= 0, got {v!r}")
        if not self.max_range > self.min_range:
            raise ValueError(f"max_range must exceed min_range, got {self.max_range!r} and {self.min_range!r}")
        if self.voxel_size is None:
            self.voxel_size = self.max_range / 100.0
        if isinstance(self.voxel_size, bool) or not isinstance(self.voxel_size, (int, float)) or not (0 < self.voxel_size < math.inf):
            raise ValueError(f"voxel_size must be a positive number, got {self.voxel_size!r}")
        if isinstance(self.max_points_per_voxel, bool) or not isinstance(self.max_points_per_voxel, int) or not 1 <= self.max_points_per_voxel <= MAX_POINTS:
            raise ValueError(f"max_points_per_voxel must be an integer in [1, {MAX_POINTS}], got {self.max_points_per_voxel!r}")
        if isinstance(self.max_num_iterations, bool) or not isinstance(self.max_num_iterations, int) or self.max_num_iterations < 1:
            raise ValueError(f"max_num_iterations must be a positive integer, got {self.max_num_iterations!r}")

    @property
    def max_distance(self) -> float:
        return 2.0 * self.max_range


class Downsampled(NamedTuple):
    """What `downsample` returns, capacity-sized with the counts on the device: frame float64 [N, 3] (counts[0] rows: the first point
    of every 0.5 voxel_size voxel, ascending input index), source float64 [N, 3] (counts[1] rows: the same at 1.5 voxel_size over
    `frame`), counts int64 [2], status int32 [1] (OUT_OF_GRID), frame_index and source_index int32 [N] (input indices)."""
    frame: Tensor
    source: Tensor
    counts: Tensor
    status: Tensor
    frame_index: Tensor
    source_index: Tensor

    def trimmed(self):
        """(frame, source, frame_index, source_index) cut to their counts: one host read; raises on OUT_OF_GRID"""
        n1, n2 = self.counts.cpu().tolist()
        if int(self.status.item()) & OUT_OF_GRID:
            raise ValueError("downsample: a point lies outside the voxel grid of +-2^20 voxels per axis (or is not finite)")
        return self.frame[:n1], self.source[:n2], self.frame_index[:n1], self.source_index[:n2]


def _rows(points: Tensor, name: str = "points") -> Tensor:
    try:
        p = point_rows(points, _FLOATS, convert=False)
    except (ValueError, TypeError) as e:
        raise type(e)(str(e).replace("points", name, 1)) from None
    if p.shape[0] >= 1 << 31:
        raise ValueError(f"{name} must have fewer than 2^31 rows, got {tuple(points.shape)}")
    require_gpu(p)
    return p


def _number(v, name: str, positive: bool = True) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)) or math.isnan(v) or (positive and not 0 < v < math.inf):
        raise ValueError(f"{name} must be a {'positive ' if positive else ''}number, got {v!r}")
    return float(v)


def downsample(points: Tensor, config: KissConfig) -> Downsampled:
    """Preprocess and voxelize of one sweep: points [N, 3] (float32 or float64 on the device, a row stride is kept).  A point is kept
    when min_range < |p| < max_range; `frame` is the first kept point of every voxel of size 0.5 voxel_size and `source` the first of
    every voxel of size 1.5 voxel_size among those, both in ascending input index.  No host read."""
    p = _rows(points)
    dev, N = p.device, p.shape[0]
    frame = torch.empty((N, 3), dtype=torch.float64, device=dev)
    source = torch.empty((N, 3), dtype=torch.float64, device=dev)
    index = torch.empty((2, N), dtype=torch.int32, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws = workspace("mtgs_icp_downsample_workspace_bytes", N, device=dev, dtype=torch.uint8)
    call("mtgs_icp_downsample", N, ptr(p) if N else None, int(p.dtype == torch.float64), row_stride(p), float(config.min_range),
         float(config.max_range), float(config.voxel_size), ptr(frame) if N else None, ptr(source) if N else None, ptr(index[0]) if N else None,
         ptr(index[1]) if N else None, ptr(counts), ptr(status), ptr(ws), ws.numel(), stream_of(p))
    return Downsampled(frame, source, counts, status, index[0], index[1])


def _pose34(pose, name: str) -> np.ndarray:
    m = pose.detach().cpu().numpy() if isinstance(pose, Tensor) else np.asarray(pose)
    if m.shape not in ((4, 4), (3, 4)) or m.dtype.kind != "f":
        raise ValueError(f"{name} must be a float [4, 4] or [3, 4], got {getattr(m, 'shape', None)}")
    return np.ascontiguousarray(m[:3], dtype=np.float64)


class VoxelMap:
    """The local map: at most `capacity` voxels of side voxel_size, each an ordered list of at most max_points_per_voxel float64
    points.  One device allocation; its contents are a function of the sequence of inserts and prunes alone (include/mtgs_icp.h)."""

    def __init__(self, voxel_size: float, max_points_per_voxel: int = 20, capacity: int = 1 << 18, device="cuda"):
        self.voxel_size = _number(voxel_size, "voxel_size")
        if isinstance(max_points_per_voxel, bool) or not isinstance(max_points_per_voxel, int) or not 1 <= max_points_per_voxel <= MAX_POINTS:
            raise ValueError(f"max_points_per_voxel must be an integer in [1, {MAX_POINTS}], got {max_points_per_voxel!r}")
        if isinstance(capacity, bool) or not isinstance(capacity, int) or not 1 <= capacity < 1 << 31:
            raise ValueError(f"capacity must be an integer in [1, 2^31), got {capacity!r}")
        self.max_points, self.capacity, self.device = max_points_per_voxel, capacity, torch.device(device)
        require_gpu(torch.empty(0, device=self.device))
        self._buf = torch.empty(size_query("mtgs_icp_map_bytes", capacity, max_points_per_voxel), dtype=torch.uint8, device=self.device)
        self.state = self._buf[:32].view(torch.int64)      # {voxels in the table, status bits, voxels that hold a point, side}
        self._touched = False
        call("mtgs_icp_map_init", ptr(self._buf), self._buf.numel(), capacity, max_points_per_voxel, self._stream())

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _args(self):
        return ptr(self._buf), self.capacity, self.max_points

    def insert(self, points: Tensor, pose=None, count: Optional[Tensor] = None) -> None:
        """Offers points [M, 3] (the first count[0] of them when `count`, an int64 tensor on the device, is given), moved through `pose`
        ([4, 4] or [3, 4]; a host array or a float64 device tensor of 12 or more elements by rows) when given, in their order.  No host
        read: a full table is reported by the next `check`, `empty` or `point_cloud`."""
        p = _rows(points)
        M = p.shape[0]
        d_pose = None
        if pose is not None:
            d_pose = pose if isinstance(pose, Tensor) and pose.is_cuda and pose.dtype == torch.float64 and pose.dim() == 1 and pose.numel() >= 12 \
                else torch.from_numpy(_pose34(pose, "pose").reshape(12)).to(self.device)
        if count is not None and (not isinstance(count, Tensor) or count.dtype != torch.int64 or not count.is_cuda or count.numel() < 1):
            raise ValueError(f"count must be an int64 tensor on the device, got {shape_of(count)}")
        ws = workspace("mtgs_icp_map_insert_workspace_bytes", M, device=self.device, dtype=torch.uint8)
        call("mtgs_icp_map_insert", *self._args(), self.voxel_size, M, ptr(p) if M else None, int(p.dtype == torch.float64), row_stride(p),
             ptr(count), ptr(d_pose), ptr(ws), ws.numel(), self._stream())
        self._touched = self._touched or M > 0

    def prune(self, origin, max_distance: float) -> None:
        """Empties every voxel whose first point q has |q - origin|^2 >= max_distance^2.  origin: three numbers on the host, or a float64
        device tensor of three."""
        if isinstance(origin, Tensor) and origin.is_cuda and origin.dtype == torch.float64 and origin.numel() == 3:
            d_origin = origin.contiguous()
        else:
            o = np.asarray(origin.detach().cpu().numpy() if isinstance(origin, Tensor) else origin, dtype=np.float64)
            if o.shape != (3,):
                raise ValueError(f"origin must be three numbers, got {getattr(o, 'shape', None)}")
            d_origin = torch.from_numpy(o).to(self.device)
        call("mtgs_icp_map_prune", *self._args(), ptr(d_origin), _number(max_distance, "max_distance", positive=False), self._stream())

    def status(self):
        """(voxels in the table, status bits, voxels that hold a point): one host read, nothing raised"""
        voxels, status, live, _ = self.state.cpu().tolist()
        return voxels, status, live

    def check(self):
        """(voxels in the table, voxels that hold a point): one host read.  Raises when an insert ran out of capacity or met a point
        outside the grid."""
        voxels, status, live = self.status()
        if status & MAP_FULL:
            raise RuntimeError(f"VoxelMap: an insert needed more than capacity = {self.capacity} voxels and was refused; the map is as it was before it")
        if status & OUT_OF_GRID:
            raise ValueError("VoxelMap: an offered point lies outside the voxel grid of +-2^20 voxels per axis (or is not finite)")
        return voxels, live

    def empty(self) -> bool:
        if not self._touched:
            return True
        return self.check()[1] == 0

    def point_cloud(self, strict: bool = True) -> Tensor:
        """The map's points float64 [P, 3], by ascending voxel key, then list order.  strict=False: do not raise on the status bits."""
        live = self.check()[1] if strict else self.status()[2]
        rows = live * self.max_points
        out = torch.empty((rows, 3), dtype=torch.float64, device=self.device)
        total = torch.zeros(1, dtype=torch.int64, device=self.device)
        ws = workspace("mtgs_icp_map_export_workspace_bytes", self.capacity, device=self.device, dtype=torch.uint8)
        call("mtgs_icp_map_export", *self._args(), rows, ptr(out) if rows else None, ptr(total), ptr(ws), ws.numel(), self._stream())
        return out[:int(total.item())]


class Association(NamedTuple):
    """One association of a source against the map: nn_index int32 [S] (32 * probe + list position, probe = 9 (i + 1) + 3 (j + 1) +
    (k + 1); -1 without a neighbour), distance float64 [S] (DBL_MAX without), mask bool [S] (the correspondences), sums float64 [28]
    in the order of include/mtgs_icp.h."""
    nn_index: Tensor
    distance: Tensor
    mask: Tensor
    sums: Tensor


def associate(source: Tensor, voxel_map: VoxelMap, max_distance: float, kernel: float) -> Association:
    """The first half of an ICP iteration on `source` as it is: the nearest neighbour of every point among the 27 voxels around it,
    the correspondences (distance < max_distance) and the sums of J^T w J, J^T w r and the count."""
    p = _rows(source, "source")
    if not isinstance(voxel_map, VoxelMap):
        raise TypeError(f"voxel_map must be a VoxelMap, got {type(voxel_map).__name__}")
    dev, S = p.device, p.shape[0]
    nn = torch.empty(S, dtype=torch.int32, device=dev)
    dist = torch.empty(S, dtype=torch.float64, device=dev)
    mask = torch.empty(S, dtype=torch.uint8, device=dev)
    sums = torch.empty(SUMS, dtype=torch.float64, device=dev)
    ws = workspace("mtgs_icp_align_workspace_bytes", S, device=dev, dtype=torch.uint8)
    call("mtgs_icp_associate", *voxel_map._args(), voxel_map.voxel_size, S, ptr(p) if S else None, int(p.dtype == torch.float64), row_stride(p),
         _number(max_distance, "max_distance", positive=False), _number(kernel, "kernel"), ptr(nn), ptr(dist), ptr(mask), ptr(sums), ptr(ws),
         ws.numel(), stream_of(p))
    return Association(nn, dist, mask.bool(), sums)


# ---- rigid 4 x 4 algebra on the host, in the order tests/icp_refs.py restates ------------------------------------------------------------
def _compose(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    out = np.eye(4)
    for r in range(3):
        row = (a[r, 0] * b[0, :4] + a[r, 1] * b[1, :4]) + a[r, 2] * b[2, :4]
        row[3] = row[3] + a[r, 3]
        out[r] = row
    return out


def _inverse(a: np.ndarray) -> np.ndarray:
    out = np.eye(4)
    out[:3, :3] = a[:3, :3].T
    for r in range(3):
        out[r, 3] = -((a[0, r] * a[0, 3] + a[1, r] * a[1, 3]) + a[2, r] * a[2, 3])
    return out


def _as44(m34: np.ndarray) -> np.ndarray:
    out = np.eye(4)
    out[:3] = m34
    return out


def _rotation_angle(R: np.ndarray) -> float:
    """2 atan2(|vec|, |w|) of the rotation's quaternion (the conversion branches on the trace, then on the largest diagonal entry)"""
    m = [[float(v) for v in row] for row in R[:3, :3]]
    t = (m[0][0] + m[1][1]) + m[2][2]
    if t > 0.0:
        t = math.sqrt(t + 1.0)
        w, t = 0.5 * t, 0.5 / t
        vec = [(m[2][1] - m[1][2]) * t, (m[0][2] - m[2][0]) * t, (m[1][0] - m[0][1]) * t]
    else:
        i = 0
        if m[1][1] > m[0][0]:
            i = 1
        if m[2][2] > m[i][i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = math.sqrt(((m[i][i] - m[j][j]) - m[k][k]) + 1.0)
        vec = [0.0, 0.0, 0.0]
        vec[i], t = 0.5 * t, 0.5 / t
        w = (m[k][j] - m[j][k]) * t
        vec[j], vec[k] = (m[j][i] + m[i][j]) * t, (m[k][i] + m[i][k]) * t
    return 2.0 * math.atan2(math.sqrt((vec[0] * vec[0] + vec[1] * vec[1]) + vec[2] * vec[2]), abs(w))


class AlignRecord(NamedTuple):
    """The device record of one alignment on the host: T_icp [4, 4], |dx| of the last step, iterations run, correspondences of the last
    iteration, status bits (CONVERGED, DEGENERATE, EMPTY_MAP; 0: max_num_iterations ran out), the 28 sums of the last iteration."""
    T_icp: np.ndarray
    dx_norm: float
    iterations: int
    correspondences: int
    status: int
    sums: np.ndarray


def _align(source: Tensor, voxel_map: VoxelMap, guess44: np.ndarray, max_distance: float, kernel: float, max_num_iterations: int,
           convergence_criterion: float, group_size: int, count: Optional[Tensor]) -> AlignRecord:
    p = _rows(source, "source")
    dev, S = p.device, p.shape[0]
    stream = stream_of(p)
    record = torch.empty(RECORD, dtype=torch.float64, device=dev)
    d_guess = torch.from_numpy(np.ascontiguousarray(guess44[:3]).reshape(12)).to(dev)
    ws = workspace("mtgs_icp_align_workspace_bytes", S, device=dev, dtype=torch.uint8)
    call("mtgs_icp_align_begin", S, ptr(p) if S else None, int(p.dtype == torch.float64), row_stride(p), ptr(count), ptr(d_guess), ptr(record),
         ptr(ws), ws.numel(), stream)
    launched = 0
    while True:
        n = min(group_size, max_num_iterations - launched)
        call("mtgs_icp_align_iterate", *voxel_map._args(), voxel_map.voxel_size, S, ptr(count), max_distance, kernel, convergence_criterion, n,
             ptr(record), ptr(ws), ws.numel(), stream)
        launched += n
        r = record.cpu().numpy()                    # the one read of the group
        if r[27] != 0.0 or launched >= max_num_iterations:
            return AlignRecord(_as44(r[:12].reshape(3, 4)), float(r[24]), int(r[25]), int(r[26]), int(r[27]), r[28:28 + SUMS].copy())


def _align_args(voxel_map, initial_guess, max_distance, kernel, max_num_iterations, convergence_criterion, group_size, count):
    if not isinstance(voxel_map, VoxelMap):
        raise TypeError(f"voxel_map must be a VoxelMap, got {type(voxel_map).__name__}")
    for name, v in (("max_num_iterations", max_num_iterations), ("group_size", group_size)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f"{name} must be a positive integer, got {v!r}")
    if group_size > 4096:
        raise ValueError(f"group_size must be at most 4096, got {group_size!r}")
    if count is not None and (not isinstance(count, Tensor) or count.dtype != torch.int64 or not count.is_cuda or count.numel() < 1):
        raise ValueError(f"count must be an int64 tensor on the device, got {shape_of(count)}")
    return (_as44(_pose34(initial_guess, "initial_guess")), _number(max_distance, "max_distance", positive=False), _number(kernel, "kernel"),
            _number(convergence_criterion, "convergence_criterion", positive=False))


def align_record(source: Tensor, voxel_map: VoxelMap, initial_guess, max_distance: float, kernel: float, max_num_iterations: int = 500,
                 convergence_criterion: float = 1e-4, group_size: int = GROUP_SIZE, count: Optional[Tensor] = None) -> AlignRecord:
    """`align_points_to_map`'s device record (the status bits and the last sums with it)."""
    guess, max_distance, kernel, convergence_criterion = _align_args(voxel_map, initial_guess, max_distance, kernel, max_num_iterations,
                                                                     convergence_criterion, group_size, count)
    return _align(source, voxel_map, guess, max_distance, kernel, max_num_iterations, convergence_criterion, group_size, count)


def align_points_to_map(source: Tensor, voxel_map: VoxelMap, initial_guess, max_distance: float, kernel: float,
                        max_num_iterations: int = 500, convergence_criterion: float = 1e-4, group_size: int = GROUP_SIZE,
                        count: Optional[Tensor] = None):
    """Registration::AlignPointsToMap: source [S, 3] on the device (the first count[0] rows when `count` is given) through
    initial_guess, then up to max_num_iterations iterations of nearest-neighbour association and a robust Gauss-Newton step, until a
    step is shorter than convergence_criterion.  Returns (T_icp initial_guess as float64 [4, 4] on the host, iterations run); an empty
    map returns the guess and 0.  Iterations are launched group_size at a time with one read of the record behind each group."""
    guess, max_distance, kernel, convergence_criterion = _align_args(voxel_map, initial_guess, max_distance, kernel, max_num_iterations,
                                                                     convergence_criterion, group_size, count)
    if not voxel_map._touched:
        return guess, 0
    r = _align(source, voxel_map, guess, max_distance, kernel, max_num_iterations, convergence_criterion, group_size, count)
    if r.status & EMPTY_MAP:
        return guess, 0
    return _compose(r.T_icp, guess), r.iterations


class LidarOdometry:
    """MTGS's KissICP (thirdparty/kiss-icp/python/kiss_icp/kiss_icp.py:47-97, deskew off).  `register_frame` per sweep in order;
    `last_pose`, `iterations` (one count per frame) and `last_status` (the alignment's status bits) are kept on the host."""

    def __init__(self, config: KissConfig, capacity: int = 1 << 18, device="cuda", group_size: int = GROUP_SIZE):
        if not isinstance(config, KissConfig):
            raise TypeError(f"config must be a KissConfig, got {type(config).__name__}")
        self.config, self.group_size = config, group_size
        self.last_pose, self.last_delta = np.eye(4), np.eye(4)
        self.last_traj_id, self.warmup = -1, -1
        self.model_sse, self.num_samples = config.initial_threshold * config.initial_threshold, 1
        self.local_map = VoxelMap(config.voxel_size, config.max_points_per_voxel, capacity, device)
        self.iterations, self.last_status = [], 0

    def threshold(self) -> float:
        return math.sqrt(self.model_sse / self.num_samples)

    def register_frame(self, points: Tensor, log_pose, traj_id) -> np.ndarray:
        """One sweep points [N, 3] on the device with its log pose ([4, 4], host) and the id of its traversal; returns the registered
        pose float64 [4, 4].  The first two frames of a traversal start from the log pose with sigma = 2, the others from the
        constant-velocity guess with the adaptive threshold; the map takes the sweep's `frame` cloud through the new pose."""
        c = self.config
        ds = downsample(points, c)
        sigma = self.threshold()
        log_pose = _as44(_pose34(log_pose, "log_pose"))
        if self.last_traj_id != traj_id:
            self.warmup = 1
            self.last_pose = log_pose
        if self.warmup >= 0:
            self.warmup -= 1
            guess, sigma = log_pose, 2.0
        else:
            guess = _compose(self.last_pose, self.last_delta)
        if self.local_map._touched:
            r = _align(ds.source, self.local_map, guess, 3.0 * sigma, sigma / 3.0, c.max_num_iterations, c.convergence_criterion,
                       self.group_size, ds.counts[1:])
        else:
            r = AlignRecord(np.eye(4), 0.0, 0, 0, EMPTY_MAP, np.zeros(SUMS))
        empty = bool(r.status & EMPTY_MAP)
        pose = guess if empty else _compose(r.T_icp, guess)
        self.last_status = r.status
        self.iterations.append(0 if empty else r.iterations)
        deviation = _compose(_inverse(guess), pose)
        t = deviation[:3, 3]
        error = math.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]) + 2.0 * c.max_range * math.sin(_rotation_angle(deviation) / 2.0)
        if error > c.min_motion_th:
            self.model_sse += error * error
            self.num_samples += 1
        update = torch.from_numpy(np.concatenate([pose[:3].reshape(12), pose[:3, 3]])).to(self.local_map.device)     # one upload
        self.local_map.insert(ds.frame, update[:12], ds.counts[:1])
        self.local_map.prune(update[12:], c.max_distance)
        self.last_delta = _compose(_inverse(self.last_pose), pose)
        self.last_pose, self.last_traj_id = pose, traj_id
        self._last_downsample = ds
        return pose

    def check(self) -> None:
        """Raises if a sweep or the map met a point outside the voxel grid, or the map ran out of capacity: one host read."""
        self.local_map.check()
        ds = getattr(self, "_last_downsample", None)
        if ds is not None and int(ds.status.item()) & OUT_OF_GRID:
            raise ValueError("downsample: a point lies outside the voxel grid of +-2^20 voxels per axis (or is not finite)")


def register_traversals(scans: Sequence[Tensor], log_poses, traj_ids, config: KissConfig, capacity: int = 1 << 18,
                        group_size: int = GROUP_SIZE):
    """The registration of a road block: scans, one [N_f, 3] device tensor per frame, all traversals in order; log_poses [F, 4, 4]
    (lidar2global of the logs, host); traj_ids [F].  As datasets/mtgs.py does, the poses are registered relative to the first pose's
    translation and moved back afterwards (apply_calibration).  Returns (poses float64 [F, 4, 4], iterations int64 [F]) on the host."""
    poses = np.array(log_poses.detach().cpu().numpy() if isinstance(log_poses, Tensor) else log_poses, dtype=np.float64)
    if poses.ndim != 3 or poses.shape[1:] != (4, 4) or poses.shape[0] != len(scans) or len(traj_ids) != len(scans):
        raise ValueError(f"log_poses must be [F, 4, 4] and traj_ids [F] with F = {len(scans)} scans, got {poses.shape} and {len(traj_ids)}")
    if len(scans) == 0:
        return np.zeros((0, 4, 4)), np.zeros(0, dtype=np.int64)
    first = poses[0, :3, 3].copy()
    poses[:, :3, 3] = poses[:, :3, 3] - first[None]
    odometry = LidarOdometry(config, capacity, scans[0].device if isinstance(scans[0], Tensor) else "cuda", group_size)
    out = []
    for scan, pose, tid in zip(scans, poses, traj_ids):
        out.append(odometry.register_frame(scan, pose, int(tid)))
        odometry.check()
    out = np.stack(out)
    out[:, :3, 3] = out[:, :3, 3] + first[None]
    return out, np.asarray(odometry.iterations, dtype=np.int64)


# ---- the two host functions that decide which traversals are kept (plain NumPy, no kernels) -------------------------------------------------
def align_poses(original_poses, registered_poses) -> np.ndarray:
    """lidar_registration_multi_traversal.py:68-111: the BEV Kabsch fit of the registered trajectory onto the original one.  Both
    [F, 4, 4]; returns the registered poses left-multiplied by the fitted transform, of which -- as the script does -- only the 2 x 2
    rotation and the difference of the mean positions are applied."""
    orig, reg = np.asarray(original_poses, dtype=np.float64), np.asarray(registered_poses, dtype=np.float64)
    if orig.ndim != 3 or orig.shape[1:] != (4, 4) or orig.shape != reg.shape or len(orig) == 0:
        raise ValueError(f"original_poses and registered_poses must both be [F, 4, 4] with F >= 1, got {orig.shape} and {reg.shape}")
    a, b = orig[:, :2, 3], reg[:, :2, 3]
    H = (b - b.mean(axis=0)).T @ (a - a.mean(axis=0))
    U, _, Vh = np.linalg.svd(H)
    R = Vh.T @ U.T
    if np.linalg.det(R) < 0:
        Vh[-1, :] *= -1
        R = Vh.T @ U.T
    t = a.mean(axis=0) - b.mean(axis=0)
    T = np.eye(4)
    T[:2, :2] = R[:2, :2]
    T[:2, 3] = t[:2]
    return T[None] @ reg


def _yaw(R: np.ndarray) -> float:
    """pyquaternion's yaw_pitch_roll[0] of a rotation matrix: atan2(2 (w z - x y), 1 - 2 (y^2 + z^2)) = atan2(-R_01, R_00)"""
    return math.atan2(-R[0, 1], R[0, 0])


def registration_errors(original_poses, registered_poses, traj_ids, max_end_point_error: float = 1.0, max_mean_error: float = 0.5):
    """calculate_errors and the rule of the script's __main__: per traversal (in order of first appearance) a dict with
    `max_end_point_error` (EPE: the larger BEV error of its first and last frame), `mean_error` (ATE-BEV), `mean_heading_error`
    (ARE-BEV, degrees) and `bad` (EPE > max_end_point_error or ATE > max_mean_error)."""
    orig, reg = np.asarray(original_poses, dtype=np.float64), np.asarray(registered_poses, dtype=np.float64)
    ids = np.asarray(traj_ids)
    if orig.ndim != 3 or orig.shape[1:] != (4, 4) or orig.shape != reg.shape or ids.shape != (len(orig),):
        raise ValueError(f"poses must be [F, 4, 4] and traj_ids [F], got {orig.shape}, {reg.shape} and {ids.shape}")
    out = {}
    for tid in dict.fromkeys(ids.tolist()):
        sel = np.flatnonzero(ids == tid)
        errors = np.linalg.norm(reg[sel, :2, 3] - orig[sel, :2, 3], axis=1)
        heading = [np.rad2deg(abs(_yaw(reg[i]) - _yaw(orig[i]))) for i in sel]
        epe, ate = float(max(errors[0], errors[-1])), float(errors.mean())
        out[tid] = {"max_end_point_error": epe, "mean_error": ate, "mean_heading_error": float(np.mean(heading)),
                    "bad": bool(epe > max_end_point_error or ate > max_mean_error)}
    return out
