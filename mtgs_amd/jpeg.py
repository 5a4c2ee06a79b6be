"""Presented frames as baseline JPEG on the device (include/mtgs_jpeg.h, csrc/jpeg.hip).

The last step before a frame leaves the process is a host JPEG encoder in all three places that write one: the viewer thread,
every frame (custom_viewer/render_state_machine.py:276-310: `.cpu().numpy()`, then `set_background_image(format="jpeg",
jpeg_quality=40 | 75 | config.jpeg_quality)`), the evaluation image dump (scene_model/custom_pipeline.py:98-143: Pillow's save at
its defaults, quality 75 and 4:2:0) and the render tool (tools/render.py:729-734).  Here the frame `mtgs_amd.present` composed is
encoded where it lies, and what crosses to the host is the file: tens of kilobytes instead of the raw frame.

    encode_jpeg(image, quality=75, subsampling="4:2:0")   -> JpegStream      uint8 or float32 [H, W, 3], any strides
    JpegStream.tobytes()                                  -> bytes           the ONE host read (the length), then that many bytes
    header(h, w, quality, subsampling)                    -> bytes           SOI .. SOS, built on the host, cached on the device
    sizes(h, w, subsampling)                              -> (workspace bytes, the capacity that cannot overflow)

The stream is byte for byte what Pillow 12.2.0 (libjpeg-turbo) writes for the same pixels, quality and subsampling: baseline,
YCbCr, one interleaved scan, the Annex K Huffman tables.  encode_jpeg makes no host read and, once the header and the workspace
of its shape exist (the first call) and with `out=`, no allocation: it can be captured in a HIP graph.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _abi
from ._inputs import shape_of
from ._lib import call, ptr, require_gpu, scratch, stream_of

_ABI = _abi.header_abi("mtgs_jpeg.h")
HEADER_BYTES = _ABI.constants["MTGS_JPEG_HEADER_BYTES"]
BLOCK_BITS = _ABI.constants["MTGS_JPEG_BLOCK_BITS"]
_SUBSAMPLINGS = {"4:2:0": _ABI.constants["MTGS_JPEG_420"], "4:4:4": _ABI.constants["MTGS_JPEG_444"]}
_CONVERSIONS = {k: _abi.header_abi("mtgs_present.h").constants["MTGS_PRESENT_U8_" + k.upper()] for k in ("truncate", "round")}


@dataclass
class JpegStream:
    """An encoded frame on the device: `data` uint8 [capacity], of which the first `nbytes` are the file; `meta` int64 [2] holds
    the length and the overflow flag.  Pass it back as `out=` to encode the next frame into the same buffers."""
    data: Tensor
    meta: Tensor

    @property
    def nbytes(self) -> Tensor:
        """device int64: the bytes of the whole file, whether they fitted or not"""
        return self.meta[0]

    @property
    def overflow(self) -> Tensor:
        """device int64, 1 if the file did not fit in `data` (nothing was written beyond it)"""
        return self.meta[1]

    def tobytes(self) -> bytes:
        """The file.  One host read (the length and the flag, 16 bytes), then a copy of exactly that many bytes."""
        nbytes, overflow = self.meta.tolist()
        if overflow:
            raise RuntimeError(f"JpegStream: the file needs {nbytes} bytes, the buffer holds {self.data.numel()} (overflow): "
                               "encode again with a larger capacity (the default cannot overflow)")
        return self.data[:nbytes].cpu().numpy().tobytes()


def _check_options(quality, subsampling, conversion, options) -> None:
    for name, value in options.items():
        if name in ("optimize", "progressive") and not value:
            continue
        raise NotImplementedError(f"encode_jpeg: {name}={value!r} is not implemented (baseline streams with the Annex K tables only)")
    if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
        raise NotImplementedError(f"encode_jpeg: quality={quality!r} is not implemented (an integer in 1..100)")
    if subsampling not in _SUBSAMPLINGS:
        raise NotImplementedError(f"encode_jpeg: subsampling={subsampling!r} is not implemented ('4:2:0' or '4:4:4')")
    if conversion not in _CONVERSIONS:
        raise ValueError(f"encode_jpeg: conversion must be 'truncate' or 'round', got {conversion!r}")


def sizes(h: int, w: int, subsampling: str = "4:2:0") -> Tuple[int, int]:
    """(bytes of workspace, the capacity no image of this shape can overflow): the header, every block at its longest code
    (MTGS_JPEG_BLOCK_BITS, derived in include/mtgs_jpeg.h), every byte of that stuffed, EOI."""
    ws, capacity = C.c_size_t(0), C.c_size_t(0)
    call("mtgs_jpeg_sizes", h, w, _SUBSAMPLINGS[subsampling], C.byref(ws), C.byref(capacity))
    return ws.value, capacity.value


def header(h: int, w: int, quality: int = 75, subsampling: str = "4:2:0") -> bytes:
    """SOI, the JFIF APP0, the two DQT, SOF0, the four DHT and the SOS header: everything before the entropy-coded segment"""
    _check_options(quality, subsampling, "truncate", {})
    buf = (C.c_uint8 * HEADER_BYTES)()
    call("mtgs_jpeg_header", h, w, quality, _SUBSAMPLINGS[subsampling], buf, HEADER_BYTES)
    return bytes(buf)


# ---- uploaded once per (h, w, quality, subsampling, device) ------------------------------------------------------------------------
_DEVICE_HEADERS: Dict[tuple, Tensor] = {}


def _device_header(h, w, quality, subsampling, device) -> Tensor:
    key = (h, w, quality, subsampling, device)
    if key not in _DEVICE_HEADERS:
        _DEVICE_HEADERS[key] = torch.from_numpy(np.frombuffer(header(h, w, quality, subsampling), dtype=np.uint8).copy()).to(device)
    return _DEVICE_HEADERS[key]


def encode_jpeg(image: Tensor, quality: int = 75, subsampling: str = "4:2:0", *, conversion: str = "truncate",
                out: Optional[JpegStream] = None, capacity: Optional[int] = None, **options) -> JpegStream:
    """The JPEG file of `image`, uint8 [H, W, 3] (what present.viewer_frame / render_frame produce) or float32 [H, W, 3] in any
    strides; float32 is converted on load as the presented frame's uint8 formats: "truncate" is (x * 255).astype(uint8) for x in
    [0, 1] (the evaluation dump's), "round" adds 0.5 first.  `capacity` (default: the worst case of the shape, sizes()) is the size
    of the buffer; a file that does not fit sets `overflow` and is cut at the capacity.  `out` (a JpegStream) is encoded into
    in place.  Anything else JPEG offers (other channel counts, 4:2:2, optimize, progressive) raises NotImplementedError."""
    _check_options(quality, subsampling, conversion, options)
    if not isinstance(image, Tensor) or image.dim() != 3:
        raise ValueError(f"image must be a [H, W, 3] tensor, got {shape_of(image)}")
    if image.shape[2] != 3:
        raise NotImplementedError(f"encode_jpeg: {image.shape[2]} channel(s) are not implemented (RGB [H, W, 3] only)")
    if image.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"image must be uint8 or float32, got {image.dtype}")
    h, w = image.shape[:2]
    if h < 1 or w < 1:
        raise ValueError(f"image must have at least one pixel, got {tuple(image.shape)}")
    if any(s < 0 for s in image.stride()):
        raise ValueError(f"image must have non-negative strides, got {image.stride()}")
    require_gpu(image)
    device = image.device
    if out is not None:
        if capacity is not None and capacity != out.data.numel():
            raise ValueError(f"capacity {capacity} is not the size of out.data ({out.data.numel()})")
        ok = (out.data.dtype == torch.uint8 and out.data.dim() == 1 and out.data.is_contiguous() and out.meta.dtype == torch.int64
              and tuple(out.meta.shape) == (2,) and out.meta.is_contiguous() and out.data.device == device == out.meta.device)
        if not ok:
            raise ValueError(f"out must hold a contiguous uint8 [capacity] data and an int64 [2] meta on {device}")
    stream = stream_of(image)
    head = _device_header(h, w, quality, subsampling, device)
    ws = scratch(("jpeg", h, w, subsampling), lambda: sizes(h, w, subsampling)[0], device, stream)      # once per stream and shape
    if out is None:
        capacity = sizes(h, w, subsampling)[1] if capacity is None else int(capacity)
        if capacity < 0:
            raise ValueError(f"capacity must not be negative, got {capacity}")
        out = JpegStream(torch.empty(capacity, dtype=torch.uint8, device=device), torch.empty(2, dtype=torch.int64, device=device))
    sy, sx, sc = image.stride()
    call("mtgs_jpeg_encode", ptr(image), int(image.dtype == torch.float32), _CONVERSIONS[conversion], h, w, sy, sx, sc,
         _SUBSAMPLINGS[subsampling], ptr(head), ptr(out.data) if out.data.numel() else None, out.data.numel(), ptr(out.meta), ptr(ws),
         ws.numel(), stream)
    return out
