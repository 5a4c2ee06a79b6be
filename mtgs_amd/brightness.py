"""Camera brightness equalisation on the device (include/mtgs_brightness.h, csrc/brightness.hip).

With `use_exposure_alignment` (the default of NuPlanDataParserConfig, mtgs/dataset/nuplan_dataparser.py:98) every training frame goes
from the decoder straight into `adjust_brightness(image, v_factor)` (mtgs/dataset/custom_dataset.py:26-32, 90-92), and the point
stack equalises its eight undistorted images before it paints the sweep (stack_RGB_point_cloud.py:81-87): one factor per camera from
the lidar points two neighbouring cameras both see (adjust_brightness_single_frame, nuplan_scripts/utils/nuplan_utils_custom.py:
334-423), then the V channel of every image scaled by its factor (adjust_brightness, :425-431).  Both run here on the device:

    adjust_brightness(images, factors, channel_order="rgb" | "bgr", image_float=False, out=None)        one launch for C images
    estimate_brightness_factors(points, lidar2imgs, images, pairs=NUPLAN_PAIRS, strip=100, min_overlap=10, return_stats=False)
    pair_table(pairs, C) -> int32 [P, 3] on the host, checked          NUPLAN_PAIRS, NUPLAN_CAMERAS

The estimate reads only V = max(R, G, B) of the HSV conversion and is pinned against the reference's own function
(tests/golden/brightness_ref.npz).  [RECALLED] The adjustment is OpenCV's 8-bit HSV round trip, and cv2 was not available to run: the
rule is OpenCV's as recalled and is this project's DEFINITION (the header states it in full; tests/brightness_refs.py restates it in
NumPy and pins it with known answers that need no recall); nothing here claims byte equality with OpenCV.  Factor 1.0 is not the
identity: the round trip runs whatever the factor, as the reference's does.

NOT covered: decoding PNG files, RGBA images, HSV_FULL and the float HSV conversions, changes of hue or saturation.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import lidar as _lidar
from ._abi import header_abi
from ._inputs import row_stride, shape_of
from ._lib import call, ptr, require_gpu, stream_of, workspace

_ABI = header_abi("mtgs_brightness.h")
MAX_IMAGES = _ABI.constants["MTGS_BRIGHTNESS_MAX_IMAGES"]
MAX_CAMERAS = _ABI.constants["MTGS_BRIGHTNESS_MAX_CAMERAS"]
MAX_PAIRS = _ABI.constants["MTGS_BRIGHTNESS_MAX_PAIRS"]

# the camera order the reference's table is written for, and its `matches` with their `overlapped_regions`: (cam1, cam2, side); side 0:
# the left strip of cam1 and the right strip of cam2 stand in when the overlap is too small, side 1 the reverse
NUPLAN_CAMERAS = ("CAM_F0", "CAM_L0", "CAM_R0", "CAM_L1", "CAM_R1", "CAM_L2", "CAM_R2", "CAM_B0")
NUPLAN_PAIRS = ((0, 1, 0), (0, 2, 1), (1, 3, 0), (2, 4, 1), (3, 5, 0), (4, 6, 1), (5, 7, 0), (6, 7, 1))


def pair_table(pairs: Sequence[Tuple[int, int, int]], C: int) -> np.ndarray:
    """The pair table int32 [P, 3] = (cam1, cam2, side) on the HOST, checked against C cameras: 1 to MAX_PAIRS rows of integers,
    two different cameras in [0, C), side 0 (left strip of cam1, right strip of cam2) or 1 (the reverse).  The order of the rows is
    the order the chain walks them; camera 0 is the one that starts at 1.0."""
    if isinstance(pairs, Tensor):
        pairs = pairs.detach().cpu().numpy()
    try:
        t = np.asarray(pairs)
    except ValueError:
        t = None
    if t is None or t.ndim != 2 or t.shape[1] != 3 or t.dtype.kind not in "iu":
        raise ValueError(f"pairs must be [P, 3] integers (cam1, cam2, side), got {pairs!r}")
    if not 1 <= t.shape[0] <= MAX_PAIRS:
        raise ValueError(f"pairs must hold 1 to {MAX_PAIRS} rows, got {t.shape[0]}")
    for p, (a, b, side) in enumerate(t.tolist()):
        if not (0 <= a < C and 0 <= b < C):
            raise ValueError(f"pairs[{p}] names a camera outside [0, {C}): {(a, b, side)}")
        if a == b:
            raise ValueError(f"pairs[{p}] names camera {a} twice")
        if side not in (0, 1):
            raise ValueError(f"pairs[{p}] has side {side}: it must be 0 (left of cam1, right of cam2) or 1")
    return np.ascontiguousarray(t, dtype=np.int32)


_tables: dict = {}     # (table bytes, device) -> the device table: uploaded once


def _device_pairs(pairs, C: int, device) -> Tensor:
    host = pair_table(pairs, C)
    key = (host.tobytes(), str(device))
    t = _tables.get(key)
    if t is None:
        t = torch.empty(host.shape, dtype=torch.int32, device=device)
        t.copy_(torch.from_numpy(host))                # a blocking copy, once per table and device: before anything is captured
        _tables[key] = t
    return t


def _images(images, name: str = "images") -> Tuple[Tensor, bool]:
    """(view [C, h, w, 3] in its own strides, whether it came as [h, w, 3])"""
    if not isinstance(images, Tensor) or images.dim() not in (3, 4):
        raise ValueError(f"{name} must be [h, w, 3] or [C, h, w, 3], got {shape_of(images)}")
    if images.shape[-1] == 4:
        raise NotImplementedError(f"{name} has 4 channels: RGBA images are not implemented (nuPlan frames are RGB)")
    if images.shape[-1] != 3:
        raise ValueError(f"{name} must be [h, w, 3] or [C, h, w, 3], got {tuple(images.shape)}")
    if images.dtype != torch.uint8:
        raise TypeError(f"{name} must be uint8, got {images.dtype}")
    single = images.dim() == 3
    v = images.detach()
    v = v.unsqueeze(0) if single else v
    C, h, w = v.shape[:3]
    if C < 1 or h < 1 or w < 1:
        raise ValueError(f"{name} must have at least one image of one pixel, got {tuple(images.shape)}")
    if C > MAX_IMAGES:
        raise ValueError(f"{name} must hold at most {MAX_IMAGES} images, got {tuple(images.shape)}")
    if h * w >= 1 << 31:
        raise ValueError(f"{name} must have fewer than 2^31 pixels each, got {tuple(images.shape)}")
    return v, single


def _extent(t: Tensor) -> Tuple[int, int]:
    """[first byte, one past the last byte) of the storage a tensor's elements touch"""
    lo = hi = t.data_ptr()
    for n, s in zip(t.shape, t.stride()):
        step = (n - 1) * s * t.element_size()
        lo, hi = lo + min(step, 0), hi + max(step, 0)
    return lo, hi + t.element_size()


def adjust_brightness(images: Tensor, factors, channel_order: str = "rgb", image_float: bool = False, out: Optional[Tensor] = None,
                      _force_strided: bool = False) -> Tensor:
    """`adjust_brightness(image, factor)` of the reference for C images in ONE launch: 8-bit RGB -> HSV, V' = trunc(clip(V * factor,
    0, 255)) in fp64, HSV -> RGB, by the project's rule [RECALLED].  images: uint8 [h, w, 3] or [C, h, w, 3] in any strides and a base off a
    dword included (contiguous dword-aligned images take 4 pixels per thread; every other layout goes byte by byte, to the same
    bytes; the kernel also takes negative strides, which torch cannot express: `_launch` with strides written by hand).  factors: a Python float (filled into a device scalar), or a DEVICE float64 tensor [C] or [] -- the
    kernel reads it from device memory, so `estimate_brightness_factors` feeds it with no host read and a captured launch follows a
    factor written later.  A NaN factor gives V' = 0.  channel_order "bgr" (cv2.imread's) swaps the first and third channel on the
    way in and out.  The result is contiguous uint8 of the images' shape, or with image_float float32 = (float)byte / 255.0f
    (get_gt_img's rule, one correctly rounded division).  out: a contiguous tensor of the result's shape and dtype that does NOT
    overlap the images (a pixel's thread writes where a neighbour's may still read on the strided layouts): an alias is refused."""
    v, single = _images(images)
    if channel_order not in ("rgb", "bgr"):
        raise ValueError(f"channel_order must be 'rgb' or 'bgr', got {channel_order!r}")
    C, h, w = v.shape[:3]
    dtype = torch.float32 if image_float else torch.uint8
    if isinstance(factors, Tensor):
        if factors.dtype != torch.float64:
            raise TypeError(f"factors must be float64, got {factors.dtype}")
        if factors.dim() > 1 or (factors.dim() == 1 and factors.shape[0] != C):
            raise ValueError(f"factors must be [C] with C = {C} or [], got {tuple(factors.shape)}")
        if factors.device != v.device:
            raise RuntimeError(f"images are on {v.device}, factors on {factors.device}: factors must be a DEVICE tensor (or a Python float)")
    elif isinstance(factors, bool) or not isinstance(factors, (int, float)):
        raise TypeError(f"factors must be a Python float or a device float64 tensor, got {type(factors).__name__}")
    if out is not None:
        if not isinstance(out, Tensor) or out.shape != images.shape or out.dtype != dtype or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous {dtype} tensor of shape {tuple(images.shape)}, got {shape_of(out)}"
                             f"{' ' + str(out.dtype) if isinstance(out, Tensor) else ''}")
        if out.device != v.device:
            raise RuntimeError(f"images are on {v.device}, out on {out.device}")
        (a0, a1), (b0, b1) = _extent(v), _extent(out)
        if a0 < b1 and b0 < a1:
            raise ValueError("out overlaps images: adjust_brightness does not work in place, pass another tensor")
    require_gpu(v)
    if isinstance(factors, Tensor):
        f = factors.detach()
        f = f if f.dim() == 0 or f.stride(0) == 1 or C == 1 else f.contiguous()
        f_stride = 0 if f.dim() == 0 else 1
    else:
        f, f_stride = torch.full((), float(factors), dtype=torch.float64, device=v.device), 0
    res = out if out is not None else torch.empty(images.shape, dtype=dtype, device=v.device)
    _launch(ptr(v), v.stride(), (C, h, w), f, f_stride, channel_order == "bgr", res, stream_of(v), _force_strided)
    return res


def _launch(src: int, strides, size, factors: Tensor, factor_stride: int, bgr: bool, res: Tensor, stream, force_strided: bool = False) -> None:
    """the launch itself: `src` the address of pixel (0, 0, 0) channel 0, strides (image, row, column, channel) in bytes of any sign"""
    call("mtgs_brightness_adjust", *size, src, *strides, ptr(factors), factor_stride, int(bgr), int(res.dtype == torch.float32),
         int(force_strided), ptr(res), stream)


def estimate_brightness_factors(points: Tensor, lidar2imgs: Tensor, images: Tensor, pairs=NUPLAN_PAIRS, strip: int = 100,
                                min_overlap: int = 10, return_stats: bool = False):
    """`adjust_brightness_single_frame` on the device: one V factor per camera, a DEVICE float64 tensor [C] whose mean is 1, in
    three launches with no host read.  points [N, 3] (float32 or float64, a row stride is kept) go through lidar2imgs ([C, 4, 4] or
    [C, 3, 4]) with `lidar.paint_points`' projection, `see` test and bilinear sample; images uint8 [C, h, w, 3] in any channel order
    (only max(R, G, B) is read).  For every pair (cam1, cam2, side) of `pairs`, in order: the points both cameras see give the two
    mean V's -- or, with fewer than min_overlap of them, the `strip` columns at the facing edges of the two images do -- and cam2's
    factor becomes cam1's factor (1.0 if it has none) times mean1 / mean2, averaged with the factor it already had.  Camera 0 starts at
    1.0; a camera no pair reaches keeps 1.0 (the reference raises KeyError there); finally every factor is divided by np.mean of
    all.  An all-black strip gives inf or NaN, as the reference's arithmetic does.  pairs: rows of integers on the host, checked
    by `pair_table` and uploaded once per table (call once before capturing a HIP graph).  return_stats adds the device int64 [P, 5]
    = n, s1, s2, strip1, strip2 per pair: the overlap count and V sums, and the two strip sums."""
    p = _lidar._sweep(points)
    _lidar._check_matrix(lidar2imgs, "lidar2imgs", True)
    C = lidar2imgs.shape[0]
    if not 1 <= C <= MAX_CAMERAS:
        raise ValueError(f"lidar2imgs must hold 1 to {MAX_CAMERAS} cameras, got {tuple(lidar2imgs.shape)}")
    if not isinstance(images, Tensor) or images.dim() != 4 or images.shape[0] != C or images.shape[3] != 3:
        raise ValueError(f"images must be [C, H, W, 3] with C = {C}, got {shape_of(images)}")
    if images.dtype != torch.uint8:
        raise TypeError(f"images must be uint8, got {images.dtype}")
    h, w = images.shape[1:3]
    _lidar._size(w, h)
    for name, value, least in (("strip", strip, 1), ("min_overlap", min_overlap, 0)):
        if isinstance(value, bool) or not isinstance(value, int) or not least <= value < 1 << 31:
            raise ValueError(f"{name} must be an integer >= {least}, got {value!r}")
    host = pair_table(pairs, C)
    require_gpu(points, lidar2imgs, images)
    dev, N, P = p.device, p.shape[0], host.shape[0]
    table = _device_pairs(host, C, dev)
    m = _lidar._rows34(lidar2imgs)
    img = images.detach().contiguous()
    factors = torch.empty(C, dtype=torch.float64, device=dev)
    stats = torch.empty((P, 5), dtype=torch.int64, device=dev)
    ws = workspace("mtgs_brightness_estimate_workspace_bytes", P, device=dev, dtype=torch.uint8)
    call("mtgs_brightness_estimate", N, ptr(p) if N else None, int(p.dtype == torch.float64), row_stride(p), C, ptr(m), h, w, ptr(img),
         P, ptr(table), strip, min_overlap, ptr(factors), ptr(stats), ptr(ws), ws.numel(), stream_of(p))
    return (factors, stats) if return_stats else factors


__all__ = ["adjust_brightness", "estimate_brightness_factors", "pair_table", "NUPLAN_PAIRS", "NUPLAN_CAMERAS", "MAX_IMAGES",
           "MAX_CAMERAS", "MAX_PAIRS"]
