"""A training frame at its stage's resolution on the device (include/mtgs_frame.h, csrc/frame.hip).

MTGS trains coarse to fine: for every frame and every scale stage CustomInputDataset._resize_data (mtgs/dataset/custom_dataset.py:
279-304) runs up to five Pillow resizes on the host -- BILINEAR on the uint8 image and the float32 depth, NEAREST on the mask, the
semantic and the instance map -- after a host pass that splits the panoptic map, fills the invalid pixels and masks the chosen
labels (:203-274).  Here the frame is kept once at full resolution on the device and taken at any size when it is needed:

    resize_plane(x, size, resample="bilinear" | "nearest", out_dtype=None)      one plane, Pillow's bytes
    resize_frame(data, size, image_float=False) -> dict                          _resize_data over the tensor entries of `data`
    frame_masks(panoptic=None, semantic=None, valid=None, labels=(255,), size=None) -> (instance_map, semantic_map, mask)
    masked_labels(load_custom_masks, mask_all_foreground) -> the label ids of _get_custom_mask
    scaled_size(H, W, factor) -> (height, width) of the rescaled camera

Every result is byte for byte what Pillow 12.2.0 gives (tests/golden/frame_ref.npz holds its outputs; tests/frame_refs.py restates
the arithmetic in NumPy): the 8-bit path is integer arithmetic with 22 fractional bits and a rounding to uint8 between the two
passes, the float32 path accumulates (double)pixel * weight in double in tap order and rounds to float32 after each pass, NEAREST
is a gather through source indices that Pillow finds by repeated addition.  The tables are built on the host in double
(mtgs_amd.dino's builders), uploaded with a blocking copy and kept per (source size, target size, device): call once before
capturing a HIP graph.  No atomics, no host read; a whole frame is three launches (image, depth, all nearest planes).

NOT covered, because nothing here can pin them: decoding the depth PNG, and RGBA images (Pillow premultiplies alpha around the
resize; nuPlan frames are RGB).  The cv2.remap undistortion in front of the resize is mtgs_amd.undistort and adjust_brightness
(cv2's HSV round trip) in front of that is mtgs_amd.brightness, both by rules the project defines; undistort's valid_mask, panoptic
and semantic planes are what frame_masks takes.
"""
from __future__ import annotations

from typing import Dict, Iterable, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from ._abi import header_abi
from ._inputs import image_plane, image_size, shape_of
from ._lib import call, ptr, require_gpu, stream_of
from .dino import bilinear_coefficients, bilinear_weights, nearest_sources

_ABI = header_abi("mtgs_frame.h")
_PLANE = _ABI.structs["mtgs_frame_plane"]
TILE_W, TILE_H = _ABI.constants["MTGS_FRAME_TILE_W"], _ABI.constants["MTGS_FRAME_TILE_H"]
CHUNK_ROWS = _ABI.constants["MTGS_FRAME_CHUNK_ROWS"]
MAX_PLANES = _ABI.constants["MTGS_FRAME_MAX_PLANES"]
MAX_SIZE = _ABI.constants["MTGS_FRAME_MAX_SIZE"]
_COPY, _INSTANCE, _SEMANTIC, _MASK = (_ABI.constants["MTGS_FRAME_" + k] for k in ("COPY", "INSTANCE", "SEMANTIC", "MASK"))

# CustomInputDataset.RESAMPLE_MAP: the filter of every array entry of a frame
RESAMPLE_MAP = {"image": "bilinear", "depth": "bilinear", "mask": "nearest", "semantic_map": "nearest", "instance_map": "nearest"}
# the Cityscapes train ids _get_custom_mask masks (cityscape_label)
CITYSCAPES = {"person": 11, "rider": 12, "car": 13, "truck": 14, "bus": 15, "motorcycle": 17, "bicycle": 18}
INVALID_SEMANTIC = 255
_BILINEAR_DTYPES = (torch.uint8, torch.float32)
_NEAREST_DTYPES = (torch.uint8, torch.int32, torch.bool)


def masked_labels(load_custom_masks: Iterable[str] = (), mask_all_foreground: bool = False) -> Tuple[int, ...]:
    """The label ids `_get_custom_mask` removes from the mask, in its order: 255 (the invalid class) always; person for
    'pedestrian'; bicycle, motorcycle, rider for 'bicycle'; car, truck, bus for 'vehicle'; all of them when the traversal is
    evaluation only (mask_all_foreground)."""
    chosen = set(load_custom_masks)
    out = [INVALID_SEMANTIC]
    if "pedestrian" in chosen or mask_all_foreground:
        out += [CITYSCAPES["person"]]
    if "bicycle" in chosen or mask_all_foreground:
        out += [CITYSCAPES["bicycle"], CITYSCAPES["motorcycle"], CITYSCAPES["rider"]]
    if "vehicle" in chosen or mask_all_foreground:
        out += [CITYSCAPES["car"], CITYSCAPES["truck"], CITYSCAPES["bus"]]
    return tuple(out)


def scaled_size(H: int, W: int, factor: float) -> Tuple[int, int]:
    """[RECALLED] (height, width) after nerfstudio's Cameras.rescale_output_resolution(factor) with its default rounding mode
    "floor": (size * factor).to(torch.int64).  The product of an int64 tensor and a Python float is a float32 tensor, so the
    product is taken in float32 here too.  nerfstudio was not available to run."""
    if H < 1 or W < 1 or not factor > 0:
        raise ValueError(f"a {H} x {W} camera scaled by {factor!r}")
    h, w = (int(np.floor(np.float32(v) * np.float32(factor))) for v in (H, W))
    if h < 1 or w < 1:
        raise ValueError(f"a {H} x {W} camera scaled by {factor!r} has no pixel left")
    return h, w


def label_bits(labels: Iterable[int]) -> np.ndarray:
    """HOST uint8 [32]: the 256-bit membership table of `labels` (label l is bit l & 7 of byte l >> 3)"""
    bits = np.zeros(32, np.uint8)
    for l in labels:
        if isinstance(l, bool) or int(l) != l or not 0 <= int(l) <= 255:
            raise ValueError(f"labels must be integers in [0, 255], got {l!r}")
        bits[int(l) >> 3] |= np.uint8(1 << (int(l) & 7))
    return bits


# ---- the tables (HOST, double; kept on the device per axis) ------------------------------------------------------------------------
_tables: dict = {}          # (kind, in size, out size, device) -> tuple of device tensors (+ ksize)


def _upload(a: np.ndarray, device) -> Tensor:
    dev = torch.empty(a.shape, dtype=torch.from_numpy(a).dtype, device=device)
    dev.copy_(torch.from_numpy(a))                  # a blocking copy: the tables are complete before anything is captured
    return dev


def _axis(kind: str, n_in: int, n_out: int, device):
    """kind "u8" / "f32": (bounds int32 [n_out, 2], coefficients int32 / float64 [n_out, ksize], ksize), all None / 0 for an
    identity pass; kind "nearest": (source indices int32 [n_out],)"""
    key = (kind, n_in, n_out, device)
    t = _tables.get(key)
    if t is None:
        if kind == "nearest":
            t = (_upload(nearest_sources(n_in, n_out, 0, n_out), device),)
        elif n_in == n_out:
            t = (None, None, 0)
        else:
            bounds, coef = (bilinear_coefficients if kind == "u8" else bilinear_weights)(n_in, n_out, 0, n_out)
            t = (_upload(bounds, device), _upload(np.ascontiguousarray(coef), device), coef.shape[1])
        _tables[key] = t
    return t


def _check_target(size, name="size") -> Tuple[int, int]:
    oh, ow = image_size(size, name)
    if oh > MAX_SIZE or ow > MAX_SIZE:
        raise ValueError(f"{name} must be at most {MAX_SIZE} on a side, got {tuple(size)}")
    return oh, ow


def _check_source(v: Tensor, name: str) -> None:
    if v.shape[0] > MAX_SIZE or v.shape[1] > MAX_SIZE:
        raise ValueError(f"{name} must be at most {MAX_SIZE} on a side, got {tuple(v.shape)}")


def _bilinear_launch(v: Tensor, oh: int, ow: int, out_float: bool) -> Tensor:
    H, W, C = v.shape
    kind = "u8" if v.dtype == torch.uint8 else "f32"
    hb, hk, hks = _axis(kind, W, ow, v.device)
    vb, vk, vks = _axis(kind, H, oh, v.device)
    out = torch.empty((oh, ow, C), dtype=torch.float32 if (out_float or kind == "f32") else torch.uint8, device=v.device)
    head = (H, W, C, ptr(v), v.stride(0), v.stride(1), v.stride(2), oh, ow, ptr(hb), ptr(hk), hks, ptr(vb), ptr(vk), vks)
    if kind == "u8":
        call("mtgs_frame_resize_u8", *head, int(out_float), ptr(out), stream_of(v))
    else:
        call("mtgs_frame_resize_f32", *head, ptr(out), stream_of(v))
    return out


def _bilinear(v: Tensor, oh: int, ow: int, out_float: bool = False, two_pass: bool = False) -> Tensor:
    """[H, W, C] uint8 or float32 -> [oh, ow, C].  two_pass: the same kernel twice, through an [H, ow, C] intermediate image --
    the form scripts/frame_bench.py times against the one launch; the bytes are the same."""
    if two_pass and v.shape[0] != oh and v.shape[1] != ow:
        v = _bilinear_launch(v, v.shape[0], ow, False)
    return _bilinear_launch(v, oh, ow, out_float)


def _plane(src: Tensor, dst: Tensor, op: int, valid: Optional[Tensor] = None, channel: int = 0) -> tuple:
    """one mtgs_frame_plane of the nearest launch's table, in the struct's member order: src [H, W, C] in its own strides (from
    `channel` on), dst contiguous"""
    return (src.data_ptr() + channel * src.stride(2) * src.element_size(), 0 if valid is None else valid.data_ptr(), dst.data_ptr(),
            tuple(src.stride()), (0, 0) if valid is None else tuple(valid.stride()[:2]), op, src.element_size(),
            src.shape[2] if op == _COPY else 1, 0)


def _nearest_launch(H: int, W: int, oh: int, ow: int, planes, bits: Optional[np.ndarray], device, stream) -> None:
    (sy,), (sx,) = _axis("nearest", H, oh, device), _axis("nearest", W, ow, device)
    for at in range(0, len(planes), MAX_PLANES):
        group = planes[at:at + MAX_PLANES]
        table = np.array(group, dtype=_PLANE)               # HOST; copied into the launch before the call returns
        call("mtgs_frame_nearest", H, W, oh, ow, ptr(sy), ptr(sx), len(group), table.ctypes.data,
             None if bits is None else bits.ctypes.data, stream)


def _valid_u8(valid, H: int, W: int) -> Optional[Tensor]:
    if valid is None:
        return None
    v, _ = image_plane(valid, "valid", (torch.bool, torch.uint8), channels=(1,))
    if tuple(v.shape[:2]) != (H, W):
        raise ValueError(f"valid must be [{H}, {W}] or [{H}, {W}, 1], got {tuple(valid.shape)}")
    return v.view(torch.uint8) if v.dtype == torch.bool else v


def _as_bytes(v: Tensor) -> Tensor:
    return v.view(torch.uint8) if v.dtype == torch.bool else v


# ---- the operators -----------------------------------------------------------------------------------------------------------------
def _check_plane(x, name: str, resample: str, out_dtype=None):
    """(view [H, W, C], came as [H, W], dtype of the result) of one plane for one filter, or the refusal"""
    if resample not in ("bilinear", "nearest"):
        raise ValueError(f"resample must be 'bilinear' or 'nearest', got {resample!r}")
    if resample == "nearest":
        v, flat = image_plane(x, name, _NEAREST_DTYPES)
        allowed = (v.dtype,)
    else:
        if isinstance(x, Tensor) and x.dim() == 3 and x.shape[2] == 4:
            raise NotImplementedError(f"{name} has 4 channels: Pillow premultiplies RGBA around a resize, which is not implemented")
        v, flat = image_plane(x, name, _BILINEAR_DTYPES, channels=(1, 3))
        if v.dtype == torch.float32 and v.shape[2] != 1:
            raise NotImplementedError(f"{name} is float32 with {v.shape[2]} channels: Pillow's mode 'F' has one")
        allowed = (torch.uint8, torch.float32) if v.dtype == torch.uint8 else (torch.float32,)
    _check_source(v, name)
    out_dtype = v.dtype if out_dtype is None else out_dtype
    if out_dtype not in allowed:
        raise ValueError(f"out_dtype of a {resample} resize of {v.dtype} must be {' or '.join(map(str, allowed))}, got {out_dtype}")
    return v, flat, out_dtype


def resize_plane(x: Tensor, size: Tuple[int, int], resample: str = "bilinear", out_dtype=None) -> Tensor:
    """Pillow's Image.resize of one plane, byte for byte.  x is [H, W] or [H, W, C] in any strides; `size` is (height, width) --
    NOTE Pillow's own argument is (width, height).  "bilinear": uint8 with 1 or 3 channels (out_dtype torch.float32 gives
    byte / 255 as one correctly rounded division, get_gt_img's conversion) or float32 with one channel (mode "F").  "nearest":
    uint8, int32 or bool with 1 to 3 channels.  The result has x's rank and is contiguous."""
    v, flat, out_dtype = _check_plane(x, "x", resample, out_dtype)
    oh, ow = _check_target(size)
    require_gpu(x)
    if resample == "bilinear":
        out = _bilinear(v, oh, ow, out_float=out_dtype == torch.float32)
    else:
        out = torch.empty((oh, ow, v.shape[2]), dtype=v.dtype, device=v.device)
        _nearest_launch(v.shape[0], v.shape[1], oh, ow, [_plane(_as_bytes(v), _as_bytes(out), _COPY)], None, v.device, stream_of(v))
    return out[..., 0] if flat else out


def resize_frame(data: Dict, size: Tuple[int, int], image_float: bool = False) -> Dict:
    """`_resize_data` over the tensor entries of `data`: RESAMPLE_MAP chooses the filter by key (image, depth: bilinear; mask,
    semantic_map, instance_map: nearest), an unknown tensor key raises KeyError as the reference's lookup does, anything that is
    not a tensor is passed through, [H, W, 1] stays [h, w, 1].  `size` is (height, width) (`scaled_size`).  image_float: the image
    comes back as float32 byte / 255 (get_gt_img) instead of uint8.  One launch for the image, one for the depth, one for all
    nearest planes of one source size."""
    oh, ow = _check_target(size)
    checked = {}
    for key, x in data.items():
        if isinstance(x, Tensor):
            resample = RESAMPLE_MAP[key]
            checked[key] = _check_plane(x, key, resample, torch.float32 if (key == "image" and image_float and x.dtype == torch.uint8) else None)
    require_gpu(*(data[k] for k in checked))
    out, nearest = dict(data), {}
    for key, (v, flat, out_dtype) in checked.items():
        if RESAMPLE_MAP[key] == "bilinear":
            res = _bilinear(v, oh, ow, out_float=out_dtype == torch.float32)
        else:
            res = torch.empty((oh, ow, v.shape[2]), dtype=v.dtype, device=v.device)
            nearest.setdefault((v.shape[0], v.shape[1], v.device), []).append(_plane(_as_bytes(v), _as_bytes(res), _COPY))
        out[key] = res[..., 0] if flat else res
    for (H, W, device), planes in nearest.items():
        _nearest_launch(H, W, oh, ow, planes, None, device, torch.cuda.current_stream(device).cuda_stream)
    return out


def frame_masks(panoptic: Optional[Tensor] = None, semantic: Optional[Tensor] = None, valid: Optional[Tensor] = None,
                labels: Iterable[int] = (INVALID_SEMANTIC,), size: Optional[Tuple[int, int]] = None):
    """The masks of a frame from its panoptic map (uint8 [H, W, 3]: `_get_panoptic_map`) or its semantic map (uint8 [H, W] or
    [H, W, 1]: `_get_semantic_map`), an optional valid mask (bool or uint8, [H, W] or [H, W, 1]) and the label ids to mask
    (`masked_labels`), at `size` = (height, width) by NEAREST or at full size, in one launch:
        instance_map int32 [h, w, 1] = channel 0 + 256 * channel 1, 0 where the pixel is not valid (None without a panoptic map)
        semantic_map uint8 [h, w, 1] = channel 2 (or the semantic map), 255 where the pixel is not valid
        mask         bool  [h, w, 1] = valid and the semantic label is not in `labels`
    A pointwise rule commutes with a gather, so this equals the reference's order: prepare at full size, then resize each."""
    if (panoptic is None) == (semantic is None):
        raise ValueError("frame_masks takes a panoptic map or a semantic map, one of the two")
    if panoptic is not None:
        src, _ = image_plane(panoptic, "panoptic", (torch.uint8,), channels=(3,))
        if panoptic.dim() != 3:
            raise ValueError(f"panoptic must be [H, W, 3], got {shape_of(panoptic)}")
    else:
        src, _ = image_plane(semantic, "semantic", (torch.uint8,), channels=(1,))
    _check_source(src, "panoptic" if panoptic is not None else "semantic")
    H, W = src.shape[:2]
    val = _valid_u8(valid, H, W)
    bits = label_bits(labels)
    oh, ow = (H, W) if size is None else _check_target(size)
    require_gpu(src, val)
    if val is not None and val.device != src.device:
        raise RuntimeError(f"valid is on {val.device}, the map on {src.device}")
    dev = src.device
    instance = torch.empty((oh, ow, 1), dtype=torch.int32, device=dev) if panoptic is not None else None
    sem = torch.empty((oh, ow, 1), dtype=torch.uint8, device=dev)
    mask = torch.empty((oh, ow, 1), dtype=torch.bool, device=dev)
    channel = 2 if panoptic is not None else 0
    planes = [_plane(src, sem, _SEMANTIC, val, channel), _plane(src, mask.view(torch.uint8), _MASK, val, channel)]
    if instance is not None:
        planes.insert(0, _plane(src, instance, _INSTANCE, val))
    _nearest_launch(H, W, oh, ow, planes, bits, dev, stream_of(src))
    return instance, sem, mask


__all__ = ["resize_plane", "resize_frame", "frame_masks", "masked_labels", "scaled_size", "label_bits", "RESAMPLE_MAP", "CITYSCAPES",
           "TILE_W", "TILE_H", "CHUNK_ROWS", "MAX_PLANES", "MAX_SIZE"]
