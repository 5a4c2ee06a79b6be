"""Rendering inside an oriented crop box.

MTGSSceneModel.get_gaussians and get_gaussian_params (mtgs_scene_graph.py:457-459, 493-495) keep, outside training, only the
Gaussians whose means lie inside the viewer's or the render tool's crop box: `crop_ids = self.crop_box.within(means)` and one
boolean-mask index per collected tensor, each a nonzero + gather pair with its own host synchronisation.  Here the selection is
mtgs_crop_select (the kept indices in ascending order, their count and the mask in one prefix sum) and the compaction of every
collected tensor ONE launch of mtgs_crop_gather; `crop_gaussians` is the two lines of the reference, with the one host read
that sizes the outputs.

`OrientedBox` stands in for nerfstudio's (nerfstudio/data/scene_box.py, version 1.1.5), which is not part of the reference tree:
what it does is recalled, not read ([NS-RECALL] in SURVEY.md's sense), and the two recalled facts each live in ONE place here --
`_inside` (strict comparisons against +-S / 2 in box coordinates; the kernel's `inside` in csrc/crop.hip is its device twin) and
`_rpy_matrix` (R = Rz(yaw) Ry(pitch) Rx(roll)).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional

import numpy as np
import torch
from torch import Tensor

from ._inputs import point_rows, row_stride
from ._lib import call, ptr, require_gpu, stream_of, workspace

MAX_TENSORS = 16       # rows of one mtgs_crop_gather table


def _inside(q: Tensor, h: Tensor) -> Tensor:
    """[NS-RECALL] the crop decision in box coordinates q [N, 3] against the half sizes h [3]: STRICTLY inside on every axis (a
    point on a face is out; NaN fails both comparisons)."""
    return ((q > -h) & (q < h)).all(dim=-1)


def _rpy_matrix(rpy) -> np.ndarray:
    """[NS-RECALL] OrientedBox.from_params: R = Rz(yaw) @ Ry(pitch) @ Rx(roll) of rpy = (roll, pitch, yaw), in fp64."""
    roll, pitch, yaw = (float(a) for a in rpy)
    cr, sr, cp, sp, cy, sy = math.cos(roll), math.sin(roll), math.cos(pitch), math.sin(pitch), math.cos(yaw), math.sin(yaw)
    rx = np.array([[1.0, 0.0, 0.0], [0.0, cr, -sr], [0.0, sr, cr]])
    ry = np.array([[cp, 0.0, sp], [0.0, 1.0, 0.0], [-sp, 0.0, cp]])
    rz = np.array([[cy, -sy, 0.0], [sy, cy, 0.0], [0.0, 0.0, 1.0]])
    return rz @ ry @ rx


def _host_f64(x, shape, name) -> np.ndarray:
    a = torch.as_tensor(x).detach().to("cpu", torch.float64).numpy()
    if a.shape != shape:
        raise ValueError(f"OrientedBox: {name} must be {list(shape)}, got {list(a.shape)}")
    return a


class OrientedBox:
    """An oriented box: rotation R [3, 3], centre T [3], full side lengths S [3] (any float dtype, any device; the fifteen
    numbers are read to the host once, here).  `within` decides in BOX coordinates: the world->box matrix is the inverse of
    H = [[R, T], [0, 1]] -- a general inverse in fp64, not R^T, because nerfstudio inverts H -- rounded to fp32, and the half
    sizes are S / 2 in fp32.  `box` holds them as the 15 floats mtgs_crop_select takes: the 3x4 matrix by rows, then S / 2."""

    def __init__(self, R, T, S):
        self.R, self.T, self.S = _host_f64(R, (3, 3), "R"), _host_f64(T, (3,), "T"), _host_f64(S, (3,), "S")
        H = np.eye(4)
        H[:3, :3], H[:3, 3] = self.R, self.T
        self.world_to_box = np.linalg.inv(H)[:3].astype(np.float32)
        self.half = self.S.astype(np.float32) / np.float32(2.0)
        self.box = np.concatenate([self.world_to_box.reshape(-1), self.half]).astype(np.float32)

    @classmethod
    def from_params(cls, pos, rpy, scale) -> "OrientedBox":
        """The box of get_crop_from_json (tools/render.py:341) and of the viewer's control panel: centre `pos`, Euler angles
        `rpy` = (roll, pitch, yaw), side lengths `scale`."""
        return cls(_rpy_matrix(rpy), pos, scale)

    def within(self, points: Tensor) -> Tensor:
        """bool [N]: which of points [N, 3] lie strictly inside.  q_k = ((m_k0 x + m_k1 y) + m_k2 z) + m_k3 in fp32, in that
        order, kept iff -h_k < q_k < h_k for every k.  On a GPU tensor this is mtgs_crop_select; on a CPU tensor the same
        operations in the same order in torch, so both give the same decision for every point."""
        if points.is_cuda:
            return _select(point_rows(points), self, want_mask=True)[2].to(torch.bool)
        p = point_rows(points)
        m, h = torch.from_numpy(self.world_to_box), torch.from_numpy(self.half)
        x, y, z = p[:, 0:1], p[:, 1:2], p[:, 2:3]
        q = ((m[:, 0] * x + m[:, 1] * y) + m[:, 2] * z) + m[:, 3]
        return _inside(q, h)


def _select(p: Tensor, box: OrientedBox, want_mask: bool):
    """(keep_ids int32 [N] capacity, count int64 [1] on the device, mask u8 [N] or None) of float32 rows p [N, 3]"""
    N, dev = p.shape[0], p.device
    keep_ids = torch.empty(N, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    mask = torch.empty(N, dtype=torch.uint8, device=dev) if want_mask else None
    ws = workspace("mtgs_crop_workspace_bytes", N, device=dev, dtype=torch.uint8)
    call("mtgs_crop_select", N, ptr(p), row_stride(p), box.box.ctypes.data_as(C.c_void_p), ptr(keep_ids), ptr(count),
         ptr(mask), ptr(ws), ws.numel(), stream_of(p))
    return keep_ids, count, mask


def gather_rows(tensors, keep_ids: Tensor, n_keep: int):
    """[v[keep_ids[:n_keep].long()] for v in tensors] in one mtgs_crop_gather launch per 16 tensors.  Every tensor has the same
    number of rows (the range of keep_ids) and rows that are a whole number of 4-byte words (a bool or uint8 entry with an odd
    row raises TypeError).  The kernel reads contiguous rows: a tensor that is not contiguous (none of the collected ones) is
    first copied whole by torch, one more pass over its N rows."""
    srcs, outs, table = [], [], []
    for v in tensors:
        s = v.detach().contiguous()
        out = torch.empty((n_keep,) + tuple(s.shape[1:]), dtype=s.dtype, device=s.device)
        row_bytes = math.prod(s.shape[1:]) * s.element_size()
        if row_bytes % 4:
            raise TypeError(f"crop: rows of {row_bytes} bytes ({s.dtype}, {tuple(s.shape)}): a row must be a whole number of 4-byte words")
        srcs.append(s)
        outs.append(out)
        if row_bytes and n_keep:
            table.append((s.data_ptr(), out.data_ptr(), row_bytes))
    n_rows = srcs[0].shape[0] if srcs else 0
    for at in range(0, len(table), MAX_TENSORS):
        part = table[at:at + MAX_TENSORS]
        n = len(part)
        call("mtgs_crop_gather", n_keep, n_rows, ptr(keep_ids), n, (C.c_uint64 * n)(*(t[0] for t in part)),
             (C.c_uint64 * n)(*(t[1] for t in part)), (C.c_int64 * n)(*(t[2] for t in part)), stream_of(keep_ids))
    return outs


def crop_gaussians(gaussians: Dict[str, Optional[Tensor]], box: OrientedBox) -> Dict[str, Optional[Tensor]]:
    """`{k: v[box.within(gaussians["means"])] for k, v in gaussians.items()}` (mtgs_scene_graph.py:457-459, 493-495) for the
    dictionaries `collect_gaussians` returns and for the get_gaussian_params shape (features_dc / features_rest): every tensor
    entry with one row per Gaussian is compacted to the kept rows, in their order.  One selection, one read of the count (the
    only host synchronisation: it sizes the outputs) and one gather launch.  Entries that are None stay None; `node_table` is
    dropped, because its slices no longer describe the rows.  "One row per Gaussian" is decided by the shape alone: EVERY tensor
    entry whose leading dimension equals the number of means is compacted, whatever it holds, and such an entry whose rows are not
    a whole number of 4-byte words (bool, uint8 [N]) raises TypeError; other entries pass through.  An evaluation feature, as in the reference (`not self.training`):
    the outputs never carry a graph, and inputs that would need one are refused."""
    if gaussians.get("color_source") is not None:
        raise NotImplementedError("crop_gaussians: a 'color_source' entry (collect_gaussians(..., deferred_colors=True)) addresses its "
                                  "rows through the node table and cannot be cropped: collect with deferred_colors=False")
    if torch.is_grad_enabled():
        needs = sorted(k for k, v in gaussians.items() if isinstance(v, Tensor) and v.requires_grad)
        if needs:
            raise ValueError(f"crop_gaussians: {needs} require grad while grad is enabled: the crop is an evaluation feature (the "
                             "reference applies it when not training) -- call it under torch.no_grad()")
    means = gaussians["means"]
    require_gpu(means)
    N = means.shape[0]
    rows = [k for k, v in gaussians.items() if k != "node_table" and isinstance(v, Tensor) and v.dim() >= 1 and v.shape[0] == N]
    require_gpu(*(gaussians[k] for k in rows))
    keep_ids, count, _ = _select(point_rows(means), box, want_mask=False)
    n_keep = int(count.item())
    out = {k: v for k, v in gaussians.items() if k != "node_table"}
    out.update(zip(rows, gather_rows([gaussians[k] for k in rows], keep_ids, n_keep)))
    return out
