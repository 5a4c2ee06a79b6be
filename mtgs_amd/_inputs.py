"""What the operators do to their inputs before a launch, in one place: the point rows, the image pair and its mask, the fp32 and
uint8 forms the kernels read, and the "got ..." fragment of a refusal.  Private: the operator modules import from here."""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from ._lib import require_gpu


def shape_of(x) -> str:
    """what a refusal says it got: the shape of a tensor, the type's name of anything else"""
    return str(tuple(x.shape)) if isinstance(x, Tensor) else type(x).__name__


def mask_u8(mask: Optional[Tensor], H: int, W: int) -> Optional[Tensor]:
    """[H,W] uint8 view of a pixel mask for the kernels.  A bool mask is REINTERPRETED (True is the byte 1): `.to(torch.uint8)`
    is a copy kernel, and the loss head takes the same mask four or five times per iteration."""
    if mask is None:
        return None
    m = mask.reshape(H, W).contiguous()
    return m.view(torch.uint8) if m.dtype == torch.bool else m.to(torch.uint8)


def as_f32(t: Tensor, *shape) -> Tensor:
    """The detached fp32 contiguous array (reshaped to `shape` when given) a kernel reads: no copy when `t` already is one."""
    t = t.detach().to(torch.float32)
    return (t.reshape(shape) if shape else t).contiguous()


def point_rows(points: Tensor, dtypes=(torch.float32,), convert: bool = True) -> Tensor:
    """Detached rows [N, 3] of one of `dtypes` whose three coordinates are adjacent.  A row stride >= 3 is kept, so a [N, 4][:, :3]
    view is read in place; any other layout -- a column stride, whatever N, or rows that overlap -- is copied.  Another dtype is
    converted to dtypes[0], or refused when `convert` is off."""
    if not isinstance(points, Tensor) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be [N, 3], got {shape_of(points)}")
    p = points.detach()
    if p.dtype not in dtypes:
        if not convert:
            raise TypeError(f"points must be {' or '.join(str(d).removeprefix('torch.') for d in dtypes)}, got {p.dtype}")
        p = p.to(dtypes[0])
    if p.stride(1) != 1 or (p.shape[0] > 1 and p.stride(0) < 3):
        p = p.contiguous()
    return p


def row_stride(p: Tensor) -> int:
    """the row stride a launcher is given for point_rows' result: torch reports any stride for a single row"""
    return p.stride(0) if p.shape[0] > 1 else 3


def image_pair(pred: Tensor, gt: Tensor, mask: Optional[Tensor], names=("pred", "gt"), metric: Optional[str] = None):
    """(pred fp32, gt fp32, mask uint8 [H, W] or None) of two [H, W, 3] images of one shape on the device and a mask of H * W
    elements, as the kernels read them.  `metric` names an operator that is forward only and refuses an input that requires grad."""
    a, b = names
    if pred.dim() != 3:
        raise ValueError(f"{a} must be [H, W, C], got {tuple(pred.shape)}")
    if pred.shape[-1] != 3:
        raise NotImplementedError(f"{a} has {pred.shape[-1]} channels: only 3-channel images are implemented")
    if pred.shape != gt.shape:
        raise ValueError(f"{a} {tuple(pred.shape)} and {b} {tuple(gt.shape)} must have the same shape")
    if metric is not None and torch.is_grad_enabled() and (pred.requires_grad or gt.requires_grad):
        raise RuntimeError(f"{metric} is a metric here, forward only: an input requires grad (detach it or call under torch.no_grad())")
    H, W = pred.shape[:2]
    if mask is not None and mask.numel() != H * W:
        raise ValueError(f"mask must have H * W = {H * W} elements, got {tuple(mask.shape)}")
    require_gpu(pred, gt, mask)
    return as_f32(pred), as_f32(gt), mask_u8(mask, H, W)


def image_plane(x, name: str, dtypes, channels=(1, 2, 3)):
    """(view [H, W, C] of `x` in its own strides, whether `x` came as [H, W]) of one plane of a frame: a tensor [H, W] or [H, W, C]
    of one of `dtypes` with at least one pixel.  Nothing is copied: the frame kernels take any strides."""
    if not isinstance(x, Tensor) or x.dim() not in (2, 3):
        raise ValueError(f"{name} must be [H, W] or [H, W, C], got {shape_of(x)}")
    if x.dtype not in dtypes:
        raise TypeError(f"{name} must be {' or '.join(str(d).removeprefix('torch.') for d in dtypes)}, got {x.dtype}")
    flat = x.dim() == 2
    v = x.detach()
    v = v.unsqueeze(-1) if flat else v
    if v.shape[2] not in channels:
        raise NotImplementedError(f"{name} has {v.shape[2]} channels: only {', '.join(map(str, channels))} are implemented")
    if v.shape[0] < 1 or v.shape[1] < 1:
        raise ValueError(f"{name} must have at least one pixel, got {tuple(x.shape)}")
    return v, flat


def image_size(size, name: str = "size"):
    """(height, width) of a target size: two integers of at least 1"""
    ok = isinstance(size, (tuple, list)) and len(size) == 2 and all(isinstance(v, int) and not isinstance(v, bool) for v in size)
    if not ok:
        raise ValueError(f"{name} must be (height, width), two integers, got {size!r}")
    if size[0] < 1 or size[1] < 1:
        raise ValueError(f"{name} must be at least 1 x 1, got {tuple(size)}")
    return int(size[0]), int(size[1])
