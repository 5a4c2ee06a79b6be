"""Lidar sweeps stacked into a background cloud and one cloud per tracked object, on the device (include/mtgs_stack.h,
csrc/stack.hip).

StackRGBPointCloud (nuplan_scripts/stack_RGB_point_cloud.py:89-126, 153-183) builds the clouds `_load_3D_points` and
`_generate_instance_infos` seed the nodes from: every frame's top-lidar sweep is split against the frame's annotated boxes
(extract_frame_background_instance_lidar, nuplan_scripts/utils/stack_point_cloud_utils.py: a Python loop over the boxes, one fp64
product and two masked copies of the remaining sweep per box), painted by the cameras, filtered by field of view and concatenated
over the traversal (accumulate_background_box_point).  The loop is a per-point rule -- the FIRST box whose inflated test holds owns
the point; it is an instance point if the tight test holds too and is dropped otherwise -- which include/mtgs_stack.h states.

    box_matrices(boxes)                                          -> (lidar2box [B, 4, 4], box2lidar [B, 4, 4], half_sizes [B, 3]), NumPy
    upload_boxes(boxes, include=None, fill_scale=0.25, device=)  -> BoxTable on the device (once per frame)
    split_sweep(points, boxes, include=None, fill_scale=0.25)    -> SplitSweep(points, offsets, slot)
    stack_frame(points, table, lidar2imgs, images, sem_masks, channel_order="bgr", label_cutoff=10, equalise_brightness=False) -> FrameClouds
    SweepStack(fill_scale=0.25, label_cutoff=10, skip_classes=...).add_frame(...) / .finish() -> StackedClouds
    SweepStack(...).configure_brightness(equalise_brightness=True, pairs=NUPLAN_PAIRS): every frame's images equalised before the painting

The box matrices are built on the host with the NumPy calls the reference uses (np.cos / np.sin, np.linalg.inv) and uploaded once per
call; the kernels take matrices, never boxes.  A frame reads nothing back and can be captured in a HIP graph (given a BoxTable);
`finish` makes one host read, of the totals that size its outputs.  All arithmetic is fp64 in the stated order; tests/stack_refs.py
restates it in NumPy.

Out of scope: parsing the .pcd sweeps and the `only_top` selection, and writing the .pcd files: the caller hands in the sweep and
the undistorted images and takes device tensors back.  The undistortion itself (mode keep_focal_length, linear for the images,
nearest for the masks) is mtgs_amd.undistort.undistort_plane, and the brightness equalisation between it and the painting
(stack_RGB_point_cloud.py:81-87) is mtgs_amd.brightness, switched on by `equalise_brightness=`: both by rules the project defines.
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _abi
from ._inputs import point_rows, row_stride, shape_of
from ._lib import call, ptr, require_gpu, stream_of, workspace
from . import lidar as _lidar
from .brightness import NUPLAN_PAIRS, adjust_brightness, estimate_brightness_factors

_ABI = _abi.header_abi("mtgs_stack.h")
MAX_BOXES = _ABI.constants["MTGS_STACK_MAX_BOXES"]
BOX_CHUNK = _ABI.constants["MTGS_STACK_BOX_CHUNK"]
_FRAME_DESC = _ABI.structs["mtgs_stack_frame_desc"]
SKIP_CLASSES = ("traffic_cone", "barrier", "czone_sign")
_FLOATS = (torch.float32, torch.float64)


class BoxTable(NamedTuple):
    """The boxes of one frame as the kernels read them, float64 on the device: lidar2box and box2lidar [B, 12] (3 x 4 by rows),
    half_tight and half_inflated [B, 3], include uint8 [B]."""
    lidar2box: Tensor
    box2lidar: Tensor
    half_tight: Tensor
    half_inflated: Tensor
    include: Tensor


class SplitSweep(NamedTuple):
    """What `split_sweep` returns: points float64 [N, 3] (the background rows, then the box-frame rows of box 0, 1, ...; zero from
    offsets[B + 1] on, one row per dropped point), offsets int64 [B + 2] on the device, slot int32 [N] (0 background, 1 + b, -1
    dropped)."""
    points: Tensor
    offsets: Tensor
    slot: Tensor


class FrameClouds(NamedTuple):
    """One frame, capacity-sized, counts on the device: points float64 [N, 3] (background rows in the lidar frame, then box-frame
    rows), rgb float64 [N, 3], labels int32 [N], offsets int64 [B + 2] (rows from offsets[B + 1] on are unspecified), bg_sel int32
    [N] (the background rows whose label is below the cutoff; bg_kept int64 [1] of them), slot int32 [N] of the input points."""
    points: Tensor
    rgb: Tensor
    labels: Tensor
    offsets: Tensor
    bg_sel: Tensor
    bg_kept: Tensor
    slot: Tensor


class StackedClouds(NamedTuple):
    """What `SweepStack.finish` returns: background = (xyz float64 [M, 3] in global coordinates, rgb float64 [M, 3] in [0, 1], labels
    int32 [M]); instances = {track token: (xyz float64 [K, 3] in the box frame, rgb float64 [K, 3])}, tracks without a point left
    out.  xyz and rgb go to `pointcloud.prepare_seed_cloud` and `seed.seed_gaussians` as they are."""
    background: Tuple[Tensor, Tensor, Tensor]
    instances: Dict[str, Tuple[Tensor, Tensor]]


def _boxes(boxes) -> np.ndarray:
    if isinstance(boxes, Tensor):
        boxes = boxes.detach().cpu().numpy()
    b = np.asarray(boxes)
    if b.ndim != 2 or b.shape[1] != 7 or b.dtype.kind not in "fiu":
        raise ValueError(f"boxes must be [B, 7] numbers (xc, yc, zc, l, w, h, yaw), got {shape_of(boxes) if isinstance(boxes, Tensor) else getattr(b, 'shape', type(boxes).__name__)}")
    if b.shape[0] > MAX_BOXES:
        raise ValueError(f"boxes must hold at most {MAX_BOXES} boxes, got {tuple(b.shape)}")
    return b.astype(np.float64)


def box_matrices(boxes):
    """(lidar2box [B, 4, 4], box2lidar [B, 4, 4], half_sizes [B, 3]) float64 on the HOST of boxes [B, 7] = (xc, yc, zc, l, w, h, yaw)
    in the lidar frame: the pose as InstanceObject builds it (np.cos / np.sin of each yaw, the centre) and its np.linalg.inv, as
    split_points takes it (one call for all boxes: the same LAPACK routine per matrix, the same bits); half_sizes = (l, w, h) / 2."""
    b = _boxes(boxes)
    B = b.shape[0]
    c, s = (np.array([f(t) for t in b[:, 6]], dtype=np.float64) for f in (np.cos, np.sin))      # per yaw, as the reference calls them
    box2lidar = np.zeros((B, 4, 4))
    box2lidar[:, 0, 0], box2lidar[:, 0, 1], box2lidar[:, 1, 0], box2lidar[:, 1, 1] = c, -s, s, c
    box2lidar[:, 2, 2] = box2lidar[:, 3, 3] = 1.0
    box2lidar[:, :3, 3] = b[:, :3]
    lidar2box = np.linalg.inv(box2lidar) if B else np.zeros((0, 4, 4))
    return lidar2box, box2lidar, b[:, 3:6] / 2


def _host_table(boxes, include, fill_scale):
    """([B, 30] float64: lidar2box, box2lidar, half_tight, half_inflated by rows; include uint8 [B]) on the host"""
    b = _boxes(boxes)
    B = b.shape[0]
    if include is None:
        inc = np.ones(B, dtype=np.uint8)
    else:
        inc = np.asarray(include.detach().cpu().numpy() if isinstance(include, Tensor) else include)
        if inc.shape != (B,):
            raise ValueError(f"include must be [B] with B = {B}, got {tuple(inc.shape)}")
        inc = (inc != 0).astype(np.uint8)
    if isinstance(fill_scale, bool) or not isinstance(fill_scale, (int, float)) or not fill_scale >= 0:
        raise ValueError(f"fill_scale must be a number >= 0, got {fill_scale!r}")
    if not np.isfinite(b).all():
        raise ValueError("boxes must be finite")
    lidar2box, box2lidar, half = box_matrices(b)
    inflated = (b[:, 3:6] + float(fill_scale)) / 2
    return np.concatenate([lidar2box[:, :3].reshape(B, 12), box2lidar[:, :3].reshape(B, 12), half, inflated], axis=1), inc


def _upload(packed, inc, device) -> BoxTable:
    dev = torch.device(device)
    require_gpu(torch.empty(0, device=dev))
    t = torch.from_numpy(np.ascontiguousarray(packed)).to(dev)            # one copy for the four float arrays
    return BoxTable(t[:, 0:12].contiguous(), t[:, 12:24].contiguous(), t[:, 24:27].contiguous(), t[:, 27:30].contiguous(),
                    torch.from_numpy(inc).to(dev))


def upload_boxes(boxes, include=None, fill_scale: float = 0.25, device="cuda") -> BoxTable:
    """The BoxTable of boxes [B, 7]: `box_matrices` on the host, half_inflated = (size + fill_scale) / 2, include [B] (None: all),
    uploaded once."""
    return _upload(*_host_table(boxes, include, fill_scale), device)


def _sweep(points: Tensor) -> Tensor:
    p = point_rows(points, _FLOATS, convert=False)
    if p.shape[0] >= 1 << 31:
        raise ValueError(f"points must have fewer than 2^31 rows, got {tuple(points.shape)}")
    return p


def split_sweep(points: Tensor, boxes, include=None, fill_scale: float = 0.25) -> SplitSweep:
    """One sweep against the boxes of its frame: points [N, 3] (float32 or float64 on the device, a row stride is kept), boxes [B, 7]
    on the host (or a BoxTable from `upload_boxes`), include [B] (False: the box is skipped, as the reference skips traffic cones,
    barriers and construction-zone signs).  Of the included boxes in order, the first whose inflated test holds owns the point; the
    point is an instance point (its box-frame coordinates are kept) if the tight test holds too, dropped otherwise; a point no box
    owns, a NaN among them, is background.  No host read."""
    p = _sweep(points)
    if isinstance(boxes, BoxTable):
        if include is not None:
            raise ValueError("include goes into upload_boxes: a BoxTable carries its own")
        require_gpu(points, *boxes)
        t = boxes
    else:
        host = _host_table(boxes, include, fill_scale)
        require_gpu(points)
        t = _upload(*host, p.device)
    dev, N, B = p.device, p.shape[0], t.lidar2box.shape[0]
    out = torch.empty((N, 3), dtype=torch.float64, device=dev)
    offsets = torch.empty(B + 2, dtype=torch.int64, device=dev)
    slot = torch.empty(N, dtype=torch.int32, device=dev)
    ws = workspace("mtgs_stack_split_workspace_bytes", N, B, device=dev, dtype=torch.uint8)
    call("mtgs_stack_split", N, ptr(p) if N else None, int(p.dtype == torch.float64), row_stride(p), B, ptr(t.lidar2box), ptr(t.half_tight),
         ptr(t.half_inflated), ptr(t.include), ptr(out), ptr(offsets), ptr(slot), ptr(ws), ws.numel(), stream_of(p))
    return SplitSweep(out, offsets, slot)


def _cameras(lidar2imgs, images, sem_masks, channel_order):
    _lidar._check_matrix(lidar2imgs, "lidar2imgs", True)
    C = lidar2imgs.shape[0]
    if not 1 <= C <= _lidar.MAX_CAMERAS:
        raise ValueError(f"lidar2imgs must hold 1 to {_lidar.MAX_CAMERAS} cameras, got {tuple(lidar2imgs.shape)}")
    if channel_order not in ("bgr", "rgb"):
        raise ValueError(f"channel_order must be 'bgr' or 'rgb', got {channel_order!r}")
    if not isinstance(images, Tensor) or images.dim() != 4 or images.shape[0] != C or images.shape[3] != 3:
        raise ValueError(f"images must be [C, H, W, 3] with C = {C}, got {shape_of(images)}")
    if images.dtype != torch.uint8:
        raise TypeError(f"images must be uint8, got {images.dtype}")
    h, w = images.shape[1:3]
    ok = isinstance(sem_masks, Tensor) and sem_masks.shape[0:1] == (C,) and (sem_masks.dim() == 3 or (sem_masks.dim() == 4 and sem_masks.shape[3] == 1))
    if not ok or tuple(sem_masks.shape[1:3]) != (h, w):
        raise ValueError(f"sem_masks must be [C, H, W, 1] or [C, H, W] with C = {C} and the images' size {h} x {w}, got {shape_of(sem_masks)}")
    if sem_masks.dtype != torch.uint8:
        raise TypeError(f"sem_masks must be uint8, got {sem_masks.dtype}")
    _lidar._size(w, h)
    return C, h, w


def stack_frame(points: Tensor, table: BoxTable, lidar2imgs: Tensor, images: Tensor, sem_masks: Tensor, channel_order: str = "bgr",
                label_cutoff: int = 10, equalise_brightness: bool = False, brightness_pairs=NUPLAN_PAIRS,
                brightness_points: Optional[Tensor] = None) -> FrameClouds:
    """One frame of the stack (stack_RGB_point_cloud.py:91-126): `split_sweep`, the cameras' colours and labels of the background
    points and of the instance points taken back to the lidar frame (`lidar.paint_points`' kernel and arguments), and the rows some
    camera sees, group by group, order kept.  Everything stays on the device at the sweep's capacity N; nothing is read back, so the
    call can be captured in a HIP graph.  equalise_brightness (off by default, and then nothing changes): the images first go through
    `brightness.estimate_brightness_factors` (over brightness_points, the reference's combined sweep, or over `points` when None;
    brightness_pairs as that function takes them) and `brightness.adjust_brightness`, as stack_RGB_point_cloud.py:81-87 has it."""
    p = _sweep(points)
    if not isinstance(table, BoxTable):
        raise TypeError(f"table must be a BoxTable (upload_boxes), got {type(table).__name__}")
    C, h, w = _cameras(lidar2imgs, images, sem_masks, channel_order)
    if isinstance(label_cutoff, bool) or not isinstance(label_cutoff, int):
        raise ValueError(f"label_cutoff must be an integer, got {label_cutoff!r}")
    if not isinstance(equalise_brightness, bool):
        raise ValueError(f"equalise_brightness must be True or False, got {equalise_brightness!r}")
    require_gpu(points, *table, lidar2imgs, images, sem_masks)
    dev, N, B = p.device, p.shape[0], table.lidar2box.shape[0]
    if equalise_brightness:
        factors = estimate_brightness_factors(p if brightness_points is None else brightness_points, lidar2imgs, images, brightness_pairs)
        images = adjust_brightness(images, factors, channel_order)
    m = _lidar._rows34(lidar2imgs)
    img, msk = images.detach().contiguous(), sem_masks.detach().contiguous()
    out = torch.empty((N, 3), dtype=torch.float64, device=dev)
    rgb = torch.empty((N, 3), dtype=torch.float64, device=dev)
    labels = torch.empty(N, dtype=torch.int32, device=dev)
    offsets = torch.empty(B + 2, dtype=torch.int64, device=dev)
    bg_sel = torch.empty(N, dtype=torch.int32, device=dev)
    bg_kept = torch.empty(1, dtype=torch.int64, device=dev)
    slot = torch.empty(N, dtype=torch.int32, device=dev)
    ws = workspace("mtgs_stack_frame_workspace_bytes", N, B, device=dev, dtype=torch.uint8)
    call("mtgs_stack_frame", N, ptr(p) if N else None, int(p.dtype == torch.float64), row_stride(p), B, ptr(table.lidar2box),
         ptr(table.box2lidar), ptr(table.half_tight), ptr(table.half_inflated), ptr(table.include), C, ptr(m), h, w, ptr(img),
         int(channel_order == "bgr"), ptr(msk), label_cutoff, ptr(out), ptr(rgb), ptr(labels), ptr(offsets), ptr(bg_sel), ptr(bg_kept),
         ptr(slot), ptr(ws), ws.numel(), stream_of(p))
    return FrameClouds(out, rgb, labels, offsets, bg_sel, bg_kept, slot)


class SweepStack:
    """The traversal: `add_frame` per frame in frame order (device work only), `finish` once (one host read).

    fill_scale: the margin around a box (split_points' 0.25); label_cutoff: the background keeps labels below it (`< 10` drops sky,
    person, rider and the vehicles); skip_classes: the box classes that take no points.  `configure_brightness` switches the
    equalisation of every frame's images on (`stack_frame(equalise_brightness=True)`); it is off by default, and off is what the stack
    computed before the option existed."""

    equalise_brightness, brightness_pairs = False, NUPLAN_PAIRS

    def __init__(self, fill_scale: float = 0.25, label_cutoff: int = 10, skip_classes: Sequence[str] = SKIP_CLASSES):
        if isinstance(label_cutoff, bool) or not isinstance(label_cutoff, int):
            raise ValueError(f"label_cutoff must be an integer, got {label_cutoff!r}")
        if isinstance(fill_scale, bool) or not isinstance(fill_scale, (int, float)) or not fill_scale >= 0:
            raise ValueError(f"fill_scale must be a number >= 0, got {fill_scale!r}")
        self.fill_scale, self.label_cutoff, self.skip_classes = float(fill_scale), label_cutoff, tuple(skip_classes)
        self._frames = []      # (FrameClouds, lidar2global [3, 4] float64 on the host, [(slot, token)] of the included boxes)
        self._device = None

    def __len__(self) -> int:
        return len(self._frames)

    def configure_brightness(self, equalise_brightness: bool = True, pairs=NUPLAN_PAIRS) -> "SweepStack":
        """equalise_brightness=True: from the next frame on the images go through `brightness.estimate_brightness_factors` (over the
        frame's own sweep, with `pairs`) and `brightness.adjust_brightness` in front of the painting, as stack_RGB_point_cloud.py:81-87
        has it (the reference estimates from the combined sweep of all lidars: `stack_frame(brightness_points=)` takes one).  Returns
        self: `SweepStack().configure_brightness(equalise_brightness=True)`."""
        if not isinstance(equalise_brightness, bool):
            raise ValueError(f"equalise_brightness must be True or False, got {equalise_brightness!r}")
        self.equalise_brightness, self.brightness_pairs = equalise_brightness, tuple(tuple(int(v) for v in row) for row in pairs)
        return self

    def add_frame(self, points: Tensor, boxes, names: Sequence[str], track_tokens: Sequence[str], lidar2global, lidar2imgs: Tensor,
                  images: Tensor, sem_masks: Tensor, channel_order: str = "bgr") -> FrameClouds:
        """One frame: the top-lidar sweep points [N, 3] on the device, its boxes [B, 7] in the lidar frame with their class names and
        track tokens (host), lidar2global [4, 4] or [3, 4] (host or device), and the cameras as `lidar.paint_points` takes them
        (lidar2imgs [C, 4, 4], undistorted images uint8 [C, H, W, 3], sem_masks uint8 [C, H, W, 1]).  Returns the frame's clouds."""
        b = _boxes(boxes)
        names, tokens = list(names), list(track_tokens)
        if len(names) != b.shape[0] or len(tokens) != b.shape[0]:
            raise ValueError(f"names and track_tokens must have one entry per box ({b.shape[0]}), got {len(names)} and {len(tokens)}")
        include = np.array([n not in self.skip_classes for n in names], dtype=bool)
        kept = [t for t, inc in zip(tokens, include) if inc]
        if len(set(kept)) != len(kept):
            raise ValueError("track_tokens must be unique within a frame")
        g = lidar2global.detach().cpu().numpy() if isinstance(lidar2global, Tensor) else np.asarray(lidar2global)
        if g.shape not in ((4, 4), (3, 4)) or g.dtype.kind != "f":
            raise ValueError(f"lidar2global must be a float [4, 4] or [3, 4], got {getattr(g, 'shape', None)}")
        p = _sweep(points)
        require_gpu(points)
        if self._device is not None and p.device != self._device:
            raise ValueError(f"every frame must be on one device, got {p.device} after {self._device}")
        table = upload_boxes(b, include, self.fill_scale, p.device)
        frame = stack_frame(p, table, lidar2imgs, images, sem_masks, channel_order, self.label_cutoff, self.equalise_brightness,
                            self.brightness_pairs)
        self._device = p.device
        self._frames.append((frame, g[:3].astype(np.float64), [(1 + i, tokens[i]) for i in range(len(tokens)) if include[i]]))
        return frame

    def finish(self) -> StackedClouds:
        """The stacked clouds: the backgrounds through their frames' lidar2global, concatenated in frame order, rows with a label
        below the cutoff only; every track's groups concatenated in frame order.  One scan over the (frame, slot) counts, one host
        read of the totals, one gather launch."""
        dev = self._device if self._device is not None else torch.device("cuda")
        F = len(self._frames)
        tracks: Dict[str, list] = {}
        for f, (_, _, slots) in enumerate(self._frames):
            for slot, token in slots:
                tracks.setdefault(token, []).append((f, slot))
        segments = [(f, 0) for f in range(F)]
        starts = [0, F]                                 # the first segment of the background, of every track, and the end
        for token, groups in tracks.items():
            segments += groups
            starts.append(len(segments))
        S = len(segments)
        empty = lambda n, dtype: torch.empty((0, n) if n else (0,), dtype=dtype, device=dev)
        if S == 0:
            return StackedClouds((empty(3, torch.float64), empty(3, torch.float64), empty(0, torch.int32)), {})
        desc = np.zeros(F, dtype=_FRAME_DESC)
        for f, (fr, g, _) in enumerate(self._frames):
            desc[f] = (ptr(fr.points) or 0, ptr(fr.rgb) or 0, ptr(fr.labels) or 0, ptr(fr.offsets), ptr(fr.bg_sel) or 0, ptr(fr.bg_kept),
                       fr.offsets.shape[0] - 1, g.reshape(12))
        seg = np.asarray(segments, dtype=np.int32).T.copy()                   # [2, S]: frames, slots
        host = np.concatenate([desc.view(np.uint8).reshape(-1), seg.view(np.uint8).reshape(-1)])
        table = torch.from_numpy(host).to(dev)                                # one upload; desc is a multiple of 8 bytes
        d_desc, d_seg = table[:desc.nbytes], table[desc.nbytes:].view(torch.int32).view(2, S)
        prefix = torch.empty(S + 1, dtype=torch.int64, device=dev)
        ws = workspace("mtgs_stack_plan_workspace_bytes", S, device=dev, dtype=torch.uint8)
        stream = torch.cuda.current_stream(dev).cuda_stream
        call("mtgs_stack_plan", S, ptr(d_seg[0]), ptr(d_seg[1]), F, ptr(d_desc), ptr(prefix), ptr(ws), ws.numel(), stream)
        at = prefix[torch.tensor(starts, dtype=torch.int64, device=dev)].cpu().tolist()     # the one host read
        total = at[-1]
        if total >= 1 << 31:
            raise ValueError(f"the stacked clouds must have fewer than 2^31 rows, got {total}")
        xyz = torch.empty((total, 3), dtype=torch.float64, device=dev)
        rgb = torch.empty((total, 3), dtype=torch.float64, device=dev)
        labels = torch.empty(total, dtype=torch.int32, device=dev)
        call("mtgs_stack_gather", S, ptr(d_seg[0]), ptr(d_seg[1]), F, ptr(d_desc), ptr(prefix), total, ptr(xyz) if total else None,
             ptr(rgb) if total else None, ptr(labels) if total else None, stream)
        instances = {token: (xyz[a:b], rgb[a:b]) for token, a, b in zip(tracks, at[1:-1], at[2:]) if b > a}
        return StackedClouds((xyz[:at[1]], rgb[:at[1]], labels[:at[1]]), instances)
