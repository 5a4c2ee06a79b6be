"""Depth and label planes as indexed PNG on the device (include/mtgs_png.h, csrc/png.hip).

Three planes of every training frame arrive as PNG (the pseudo depth, the panoptic / semantic map, the ego mask:
mtgs/dataset/custom_dataset.py:154-243) and two preprocessing stages leave the device only to write such files
(nuplan_scripts/generate_dense_depth.py:236-247 and the semantic-mask stage).  A foreign zlib stream is one serial chain, so this is
a PAIR: a writer whose files every PNG reader accepts (Pillow, cv2.imread), and a reader that decodes the writer's files in
parallel, one lane per segment, guided by the private index chunk `mtIX`.  A PNG without it is refused by name: decode it on the
host once, encode it here; after that the plane lives on the device compressed and decodes per step without the host.

    encode_png(image, filter="sub", segment_bytes=SEGMENT_BYTES, order="rgb", to="host" | "device")   -> bytes | PngStream
    encode_depth_png(depth, raw_size=(H, W), roi=(x, y, w, h), max_range=80, min_depth=0.1, ...)      -> bytes | PngStream
    PngStream.tobytes()              the ONE host read (the length), a copy of that many bytes, the two CRC-32s by zlib.crc32
    parse_png(data)                  -> PngInfo     host only: the chunks, mtIX, the block header, the decode tables
    upload_png(data, device="cuda")  -> DevicePng   the payload, the segment offsets and the tables on the device: a cache entry
    decode_png(source, order="rgb", out=None, workspace=None, return_status=False)         -> uint8 [H, W] or [H, W, 3]
    decode_depth_png(source, out=None, workspace=None, return_status=False)                -> float32 [H, W, 1]
    sizes(h, w, channels, segment_bytes)                                                    -> (encoder workspace, capacity, decoder workspace)

The file is stated in include/mtgs_png.h and restated in tests/png_refs.py; the device file equals the restatement's byte for byte.
The encoder makes no host read and, with `out=`, no allocation once the workspace of its shape exists; the decoder, from a DevicePng
with `out=` and `workspace=`, makes no copy, no allocation and no host read.  Both can be captured in a HIP graph.
"""
from __future__ import annotations

import ctypes as C
import struct
import zlib
from dataclasses import dataclass
from typing import List, Optional, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from . import _abi
from ._inputs import shape_of
from ._lib import call, ptr, require_gpu, scratch, stream_of

_ABI = _abi.header_abi("mtgs_png.h")
_K = _ABI.constants
INDEX_VERSION = _K["MTGS_PNG_INDEX_VERSION"]
SEGMENT_BYTES = _K["MTGS_PNG_SEGMENT_BYTES"]
MIN_SEGMENT_BYTES, MAX_SEGMENT_BYTES = _K["MTGS_PNG_MIN_SEGMENT_BYTES"], _K["MTGS_PNG_MAX_SEGMENT_BYTES"]
TABLE_WORDS = _K["MTGS_PNG_TABLE_WORDS"]
FAST_BITS = _K["MTGS_PNG_FAST_BITS"]
STATUS_WORDS = _K["MTGS_PNG_STATUS_WORDS"]
ERR_SEGMENT, ERR_ADLER = _K["MTGS_PNG_ERR_SEGMENT"], _K["MTGS_PNG_ERR_ADLER"]
_FILTERS = {"none": _K["MTGS_PNG_FILTER_NONE"], "sub": _K["MTGS_PNG_FILTER_SUB"], "up": _K["MTGS_PNG_FILTER_UP"]}
_FILTER_NAMES = {v: k for k, v in _FILTERS.items()}
_ORDERS = {"rgb": _K["MTGS_PNG_ORDER_RGB"], "bgr": _K["MTGS_PNG_ORDER_BGR"]}
_SIGNATURE = b"\x89PNG\r\n\x1a\n"
_CLC_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
_COLOUR_NAMES = {3: "a palette", 4: "gray with alpha", 6: "RGB with alpha"}


# ---- the writer ----------------------------------------------------------------------------------------------------------------------
@dataclass
class PngStream:
    """An encoded plane on the device: `data` uint8 [capacity], of which the first `nbytes` are the file with the CRC-32 fields of
    mtIX and IDAT still zero; `meta` int64 [2] holds the length and the overflow flag.  Pass it back as `out=`."""
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
        """The file.  One host read (the length and the flag), a copy of exactly that many bytes, then the CRC-32s of the mtIX and
        IDAT chunks by zlib.crc32: the file crosses the host to reach a disk anyway, and the device reader never consults them."""
        nbytes, overflow = self.meta.tolist()
        if overflow:
            raise RuntimeError(f"PngStream: the file needs {nbytes} bytes, the buffer holds {self.data.numel()} (overflow): "
                               "encode again with a larger capacity (the default cannot overflow)")
        return fill_crcs(self.data[:nbytes].cpu().numpy().tobytes())


def fill_crcs(data: bytes) -> bytes:
    """`data` with the CRC-32 of every chunk written behind it"""
    out = bytearray(data)
    at = 8
    while at + 12 <= len(out):
        n = int.from_bytes(out[at:at + 4], "big")
        if at + 12 + n > len(out):
            raise ValueError("fill_crcs: a chunk runs beyond the file")
        out[at + 8 + n:at + 12 + n] = zlib.crc32(out[at + 4:at + 8 + n]).to_bytes(4, "big")
        at += 12 + n
    return bytes(out)


def _segment_bytes(segment_bytes) -> int:
    s = SEGMENT_BYTES if segment_bytes is None else segment_bytes
    if isinstance(s, bool) or not isinstance(s, int) or not MIN_SEGMENT_BYTES <= s <= MAX_SEGMENT_BYTES:
        raise ValueError(f"segment_bytes must be an integer in [{MIN_SEGMENT_BYTES}, {MAX_SEGMENT_BYTES}], got {segment_bytes!r}")
    return s


def sizes(h: int, w: int, channels: int = 3, segment_bytes: Optional[int] = None) -> Tuple[int, int, int]:
    """(bytes of the encoder's workspace, the capacity no image of this shape can overflow, bytes of the decoder's workspace)"""
    s = _segment_bytes(segment_bytes)
    ws, capacity, dec = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    call("mtgs_png_sizes", h, w, channels, s, C.byref(ws), C.byref(capacity))
    call("mtgs_png_decode_sizes", h, w, channels, s, C.byref(dec))
    return ws.value, capacity.value, dec.value


def _encode(fn, image, is_depth, h, w, channels, strides, order, filter, segment_bytes, roi, max_range, min_depth, out, capacity, to,
            first=None):
    if filter not in _FILTERS:
        if filter in ("average", "paeth", 3, 4):
            raise NotImplementedError(f"{fn}: filter={filter!r} is not implemented (Average and Paeth serialise a row; 'none', 'sub' or 'up')")
        raise ValueError(f"{fn}: filter must be 'none', 'sub' or 'up', got {filter!r}")
    if order not in _ORDERS:
        raise ValueError(f"{fn}: order must be 'rgb' or 'bgr', got {order!r}")
    if to not in ("host", "device"):
        raise ValueError(f"{fn}: to must be 'host' or 'device', got {to!r}")
    s = _segment_bytes(segment_bytes)
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
    ws = scratch(("png", h, w, channels, s), lambda: sizes(h, w, channels, s)[0], device, stream)      # once per stream and shape
    if out is None:
        capacity = sizes(h, w, channels, s)[1] if capacity is None else int(capacity)
        if capacity < 0:
            raise ValueError(f"capacity must not be negative, got {capacity}")
        out = PngStream(torch.empty(capacity, dtype=torch.uint8, device=device), torch.empty(2, dtype=torch.int64, device=device))
    sy, sx, sc = strides
    call("mtgs_png_encode", ptr(image) if first is None else first, int(is_depth), h, w, channels, sy, sx, sc, _ORDERS[order],
         _FILTERS[filter], s, *roi, float(max_range), float(min_depth), ptr(out.data) if out.data.numel() else None,
         out.data.numel(), ptr(out.meta), ptr(ws), ws.numel(), stream)
    return out.tobytes() if to == "host" else out


def encode_png(image: Tensor, filter: str = "sub", segment_bytes: Optional[int] = None, order: str = "rgb", to: str = "host", *,
               flip: str = "", out: Optional[PngStream] = None, capacity: Optional[int] = None):
    """The PNG file of `image`, uint8 [H, W] (gray) or [H, W, 3] in any strides, in the file's channel order or `order="bgr"`
    (OpenCV's array order: channel 0 is the file's blue).  `filter`: ONE for the image, "none", "sub" or "up".  `segment_bytes`: the
    unit of parallel decoding (the default is the measured one, profiles/png.txt).  `flip` ("y", "x" or "yx") encodes the image
    mirrored along those axes without a copy: the strides handed to the kernel are negative, which a tensor cannot express.
    to="host" returns the file's bytes (PngStream.tobytes()), to="device" the PngStream.  `capacity` (default: the worst case of the
    shape, sizes()) is the size of the buffer; a file that does not fit sets `overflow` and is cut at the capacity."""
    if not isinstance(image, Tensor) or image.dim() not in (2, 3):
        raise ValueError(f"image must be a [H, W] or [H, W, 3] tensor, got {shape_of(image)}")
    if image.dim() == 3 and image.shape[2] != 3:
        raise NotImplementedError(f"encode_png: {image.shape[2]} channel(s) in a [H, W, C] image are not implemented (gray [H, W] or RGB "
                                  "[H, W, 3]; alpha is out of scope)")
    if image.dtype != torch.uint8:
        raise NotImplementedError(f"encode_png: {image.dtype} is not implemented (8-bit samples only)")
    if set(flip) - set("xy") or len(set(flip)) != len(flip):
        raise ValueError(f"flip must be '', 'x', 'y' or 'yx', got {flip!r}")
    h, w = image.shape[:2]
    if h < 1 or w < 1:
        raise ValueError(f"image must have at least one pixel, got {tuple(image.shape)}")
    channels = 3 if image.dim() == 3 else 1
    sy, sx = image.stride()[:2]
    sc = image.stride(2) if channels == 3 else 0
    first = image.data_ptr()
    if "y" in flip:
        first, sy = first + (h - 1) * sy, -sy
    if "x" in flip:
        first, sx = first + (w - 1) * sx, -sx
    return _encode("encode_png", image, False, h, w, channels, (sy, sx, sc), order, filter, segment_bytes, (0, 0, 0, 0), 0.0, 0.0, out,
                   capacity, to, first)


def encode_depth_png(depth: Tensor, raw_size: Optional[Tuple[int, int]] = None, roi: Optional[Tuple[int, int, int, int]] = None,
                     max_range: float = 80, min_depth: float = 0.1, *, filter: str = "sub", segment_bytes: Optional[int] = None,
                     to: str = "host", out: Optional[PngStream] = None, capacity: Optional[int] = None):
    """The dense-depth stage's file (nuplan_scripts/generate_dense_depth.py:236-247) from float32 `depth` [h, w] in metres, in float32
    with every operation rounded once: values > max_range or < min_depth (and NaN) become 0; t = depth * 100; the low byte is
    (uint8) fmod(t, 256), the high byte (uint8) floor(t / 256); they are OpenCV's channels 0 and 1 (the file's blue and green) inside
    the window roi = (x, y, w, h) of an otherwise zero [H, W, 3] image, raw_size = (H, W) (defaults: the depth's own size, the whole
    image).  The byte image is never stored: the rule runs where the encoder loads.  The round trip through decode_depth_png is NOT
    the identity: it truncates to centimetres and clears what is out of range."""
    if not isinstance(depth, Tensor) or depth.dim() != 2 or depth.dtype != torch.float32:
        raise ValueError(f"depth must be a float32 [h, w] tensor, got {shape_of(depth)}")
    if float(np.float32(max_range) * np.float32(100)) >= 65536:
        raise NotImplementedError(f"encode_depth_png: max_range={max_range!r} is not implemented: max_range * 100 must stay below 65536 "
                                  "(two bytes of centimetres)")
    dh, dw = depth.shape
    H, W = (dh, dw) if raw_size is None else (int(raw_size[0]), int(raw_size[1]))
    x, y, w, h = (0, 0, dw, dh) if roi is None else (int(v) for v in roi)
    if (h, w) != (dh, dw):
        raise ValueError(f"roi (x, y, w, h) = {(x, y, w, h)} is not the size of depth {(dh, dw)}")
    if min(H, W, w, h) < 1 or x < 0 or y < 0 or x + w > W or y + h > H:
        raise ValueError(f"roi {(x, y, w, h)} is empty or leaves the {W} x {H} image")
    return _encode("encode_depth_png", depth, True, H, W, 3, (depth.stride(0), depth.stride(1), 0), "rgb", filter, segment_bytes,
                   (x, y, w, h), float(max_range), float(min_depth), out, capacity, to)


# ---- the reader ----------------------------------------------------------------------------------------------------------------------
@dataclass
class PngInfo:
    """What parse_png read.  `filter` is "none" | "sub" | "up"; `offsets` the bit offset of every segment's first token from the
    first byte of the IDAT payload and `eob` that of the end-of-block code; `lit_lengths` the 286 code lengths; `tables` the packed
    int32 array the kernels read (include/mtgs_png.h); the payload is data[payload_offset : payload_offset + payload_length]."""
    height: int
    width: int
    channels: int
    filter: str
    segment_bytes: int
    offsets: List[int]
    eob: int
    lit_lengths: List[int]
    has_distance: bool
    tables: np.ndarray
    payload_offset: int
    payload_length: int


@dataclass
class DevicePng:
    """A compressed plane on the device: the entry of a compressed frame cache.  `payload` uint8 [payload_length] (the IDAT chunk's
    data), `segment_bits` int32 [segments + 1] holding uint32 bit offsets, `tables` int32 [TABLE_WORDS]."""
    info: PngInfo
    payload: Tensor
    segment_bits: Tensor
    tables: Tensor


class _Bits:
    def __init__(self, data: bytes, at: int):
        self.data, self.at = data, at

    def take(self, n: int) -> int:
        if self.at + n > 8 * len(self.data):
            raise ValueError("parse_png: the file is cut short inside the block header")
        v = 0
        for k in range(n):
            v |= ((self.data[(self.at + k) >> 3] >> ((self.at + k) & 7)) & 1) << k
        self.at += n
        return v


def _canonical(lengths, longest):
    """(count of codes per length, symbols by (length, symbol), {(length, code): symbol}); ValueError unless the code is complete"""
    count = [0] * (longest + 1)
    for n in lengths:
        count[n] += 1
    count[0] = 0
    kraft = sum(c << (longest - n) for n, c in enumerate(count) if n)
    if kraft != 1 << longest and not (sum(count) == 1 and count[1] == 1):
        raise ValueError("parse_png: a Huffman code of the block header is not complete")
    code, nxt = 0, [0] * (longest + 2)
    for n in range(1, longest + 1):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    table, syms = {}, sorted((n, s) for s, n in enumerate(lengths) if n)
    for s, n in enumerate(lengths):
        if n:
            table[(n, nxt[n])] = s
            nxt[n] += 1
    return count, [s for _, s in syms], table


def _tables(lit_lengths, has_distance) -> np.ndarray:
    words = np.zeros(TABLE_WORDS, dtype=np.int32)
    count, syms, table = _canonical(lit_lengths, 15)
    words[_K["MTGS_PNG_COUNT_AT"]:][:16] = count
    words[_K["MTGS_PNG_SYMS_AT"]:][:len(syms)] = syms
    fast = words[_K["MTGS_PNG_FAST_AT"]:][:1 << FAST_BITS]
    for (n, code), s in table.items():
        if n <= FAST_BITS:
            low = int(format(code, "0%db" % n)[::-1], 2)                 # the stream holds a code from its most significant bit
            fast[low::1 << n] = (n << 9) | s
    words[_K["MTGS_PNG_DIST_AT"]] = int(has_distance)
    return words


def parse_png(data: bytes) -> PngInfo:
    """Reads the chunks, mtIX, the zlib header and the block header (a few hundred bytes) and builds the decode tables.
    NotImplementedError names what this reader does not read -- a file without mtIX first of all: it was not written by this
    encoder --; ValueError a file that is cut short or malformed.  Both before any launch."""
    data = bytes(data)
    if len(data) < 8 or data[:8] != _SIGNATURE:
        raise ValueError("parse_png: not a PNG file (no signature)")
    at, ihdr, index, payload_at, payload_n, ended = 8, None, None, None, 0, False
    while not ended:
        if at + 8 > len(data):
            raise ValueError("parse_png: the file is cut short: no IEND before its end")
        n, name = int.from_bytes(data[at:at + 4], "big"), data[at + 4:at + 8]
        if at + 12 + n > len(data):
            raise ValueError(f"parse_png: the file is cut short: the chunk {name!r} at byte {at} runs to byte {at + 12 + n} of {len(data)}")
        body = data[at + 8:at + 8 + n]
        if ihdr is None and name != b"IHDR":
            raise ValueError("parse_png: the first chunk is not IHDR")
        if name == b"IHDR":
            if n != 13 or ihdr is not None:
                raise ValueError("parse_png: malformed IHDR")
            ihdr = struct.unpack(">IIBBBBB", body)
            w, h, depth, colour, compression, method, interlace = ihdr
            if depth == 16:
                raise NotImplementedError("parse_png: 16-bit samples are not implemented (8 bits only)")
            if colour in _COLOUR_NAMES:
                raise NotImplementedError(f"parse_png: {_COLOUR_NAMES[colour]} (colour type {colour}) is not implemented (gray or RGB only)")
            if depth != 8:
                raise NotImplementedError(f"parse_png: {depth}-bit samples are not implemented (8 bits only)")
            if colour not in (0, 2) or compression != 0 or method != 0:
                raise ValueError("parse_png: malformed IHDR")
            if interlace != 0:
                raise NotImplementedError("parse_png: an interlaced (Adam7) file is not implemented")
            if not (1 <= w <= 65535 and 1 <= h <= 65535):
                raise ValueError(f"parse_png: width and height outside [1, 65535] ({w}, {h})")
        elif name == b"mtIX":
            index = body
        elif name == b"IDAT":
            if payload_at is not None:
                raise NotImplementedError("parse_png: several IDAT chunks are not implemented (this encoder writes one)")
            payload_at, payload_n = at + 8, n
        elif name == b"IEND":
            ended = True
        elif not name[0] & 0x20:
            raise NotImplementedError(f"parse_png: the critical chunk {name!r} is not implemented")
        at += 12 + n
    if index is None:
        raise NotImplementedError("parse_png: no mtIX chunk: not written by this encoder: decode on the host (Pillow, cv2.imread) and "
                                  "encode with mtgs_amd.png.encode_png")
    if payload_at is None:
        raise ValueError("parse_png: no IDAT chunk")
    if len(index) < 20 or len(index) % 4:
        raise ValueError("parse_png: malformed mtIX")
    version, filter, segment_bytes, n = struct.unpack("<4I", index[:16])
    if version != INDEX_VERSION:
        raise NotImplementedError(f"parse_png: mtIX version {version} is not implemented ({INDEX_VERSION} only)")
    if filter in (3, 4):
        raise NotImplementedError(f"parse_png: filter {filter} ({'Average' if filter == 3 else 'Paeth'}) is not implemented: it serialises a row")
    if filter not in _FILTER_NAMES:
        raise ValueError(f"parse_png: mtIX names filter {filter}")
    channels = 3 if colour == 2 else 1
    row = 1 + w * channels
    if not MIN_SEGMENT_BYTES <= segment_bytes <= MAX_SEGMENT_BYTES or n != h * -(-row // segment_bytes) or len(index) != 4 * (5 + n):
        raise ValueError("parse_png: mtIX does not describe this image")
    words = struct.unpack("<%dI" % (n + 1), index[16:])
    payload = data[payload_at:payload_at + payload_n]
    if payload_n < 8:
        raise ValueError("parse_png: the file is cut short: an IDAT of fewer than 8 bytes")
    if payload[:2] != b"\x78\x01":
        raise NotImplementedError(f"parse_png: the zlib header {payload[:2].hex()} is not this encoder's (78 01)")
    bits = _Bits(payload, 16)
    if bits.take(1) != 1 or bits.take(2) != 2:
        raise NotImplementedError("parse_png: the stream is not ONE dynamic-Huffman block: not written by this encoder")
    hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
    if hlit > 286 or hdist != 1:
        raise NotImplementedError("parse_png: more than one distance code: not written by this encoder")
    clc = [0] * 19
    for k in range(hclen):
        clc[_CLC_ORDER[k]] = bits.take(3)
    _, _, table = _canonical(clc, 7)
    lengths: List[int] = []
    while len(lengths) < hlit + 1:
        code, sym = 0, None
        for length in range(1, 8):
            code = (code << 1) | bits.take(1)
            sym = table.get((length, code))
            if sym is not None:
                break
        if sym is None:
            raise ValueError("parse_png: a prefix of the block header is no code")
        if sym < 16:
            lengths.append(sym)
        elif sym == 17:
            lengths.extend([0] * (3 + bits.take(3)))
        elif sym == 18:
            lengths.extend([0] * (11 + bits.take(7)))
        else:
            raise NotImplementedError("parse_png: code-length symbol 16: not written by this encoder")
    if len(lengths) != hlit + 1 or lengths[hlit] > 1:
        raise ValueError("parse_png: malformed code lengths in the block header")
    lit = lengths[:hlit] + [0] * (286 - hlit)
    if lit[256] == 0:
        raise ValueError("parse_png: the block has no end-of-block code")
    last = 8 * (payload_n - 4)
    if n and (words[0] != bits.at or any(a > b for a, b in zip(words, words[1:])) or words[n] >= last):
        raise ValueError("parse_png: mtIX's offsets do not fit the payload")
    return PngInfo(h, w, channels, _FILTER_NAMES[filter], segment_bytes, list(words[:n]), words[n], lit, bool(lengths[hlit]),
                   _tables(lit, bool(lengths[hlit])), payload_at, payload_n)


def _file_bytes(source) -> bytes:
    if isinstance(source, (bytes, bytearray, memoryview)):
        return bytes(source)
    if isinstance(source, Tensor):
        if source.dtype != torch.uint8 or source.dim() != 1 or source.is_cuda:
            raise TypeError("a file given as a tensor must be a host uint8 [n] tensor (or upload_png's DevicePng)")
        return source.contiguous().numpy().tobytes()
    if isinstance(source, np.ndarray):
        if source.dtype != np.uint8 or source.ndim != 1:
            raise TypeError("a file given as an array must be uint8 [n]")
        return source.tobytes()
    raise TypeError(f"source must be bytes, a host uint8 tensor or array, or a DevicePng, got {type(source).__name__}")


def upload_png(data, device="cuda") -> DevicePng:
    """Parses the file on the host and puts its payload, its segment offsets and its tables on the device"""
    data = _file_bytes(data)
    info = parse_png(data)
    payload = np.frombuffer(data, dtype=np.uint8, count=info.payload_length, offset=info.payload_offset).copy()
    offsets = np.array(info.offsets + [info.eob], dtype=np.uint32).view(np.int32)
    return DevicePng(info, torch.from_numpy(payload).to(device), torch.from_numpy(offsets).to(device), torch.from_numpy(info.tables).to(device))


def _decode(fn, source, as_depth, order, out, workspace, return_status):
    if order not in _ORDERS:
        raise ValueError(f"{fn}: order must be 'rgb' or 'bgr', got {order!r}")
    png = source if isinstance(source, DevicePng) else upload_png(source)
    info = png.info
    require_gpu(png.payload, png.segment_bits, png.tables)
    device = png.payload.device
    if png.payload.dtype != torch.uint8 or png.payload.numel() != info.payload_length or not png.payload.is_contiguous():
        raise ValueError("DevicePng.payload must be the contiguous uint8 [payload_length] payload of its info")
    if (png.segment_bits.dtype != torch.int32 or png.segment_bits.numel() != len(info.offsets) + 1 or not png.segment_bits.is_contiguous()
            or png.segment_bits.device != device):
        raise ValueError(f"DevicePng.segment_bits must be the contiguous int32 [segments + 1] offsets of its info, on {device}")
    if png.tables.dtype != torch.int32 or png.tables.numel() != TABLE_WORDS or not png.tables.is_contiguous() or png.tables.device != device:
        raise ValueError(f"DevicePng.tables must be the contiguous int32 [{TABLE_WORDS}] tables of its info, on {device}")
    if as_depth and info.channels != 3:
        raise ValueError(f"{fn}: a depth file has 3 channels, this one has {info.channels}")
    if as_depth:
        dtype, shape = torch.float32, (info.height, info.width, 1)
    else:
        dtype, shape = torch.uint8, ((info.height, info.width, 3) if info.channels == 3 else (info.height, info.width))
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=device)
    elif not isinstance(out, Tensor) or tuple(out.shape) != shape or out.dtype != dtype or out.device != device:
        raise ValueError(f"out must be a {dtype} {list(shape)} tensor on {device}")
    elif any(s < 0 for s in out.stride()):
        raise ValueError(f"out must have non-negative strides, got {out.stride()}")
    if workspace is None:
        workspace = torch.empty(sizes(info.height, info.width, info.channels, info.segment_bytes)[2], dtype=torch.uint8, device=device)
    elif (not isinstance(workspace, Tensor) or workspace.dtype != torch.uint8 or workspace.dim() != 1 or not workspace.is_contiguous()
          or workspace.device != device):
        raise ValueError(f"workspace must be a contiguous uint8 [n] tensor on {device}")
    status = workspace[:4 * STATUS_WORDS].view(torch.int32)
    sy, sx = out.stride()[:2]
    sc = out.stride(2) if len(shape) == 3 else 0
    call("mtgs_png_decode", ptr(png.payload), info.payload_length, ptr(png.segment_bits), ptr(png.tables), info.height, info.width,
         info.channels, _FILTERS[info.filter], info.segment_bytes, ptr(out), int(as_depth), sy, sx, sc, _ORDERS[order], ptr(status),
         ptr(workspace), workspace.numel(), stream_of(png.payload))
    return (out, status) if return_status else out


def decode_png(source: Union[bytes, Tensor, np.ndarray, DevicePng], order: str = "rgb", *, out: Optional[Tensor] = None,
               workspace: Optional[Tensor] = None, return_status: bool = False):
    """The pixels of a file of this encoder: uint8 [H, W] (gray) or [H, W, 3] on the device, in the file's channel order or
    `order="bgr"` (what cv2.imread returns).  `source` is the file (bytes, a host uint8 tensor or array: parsed and uploaded here) or a
    DevicePng.  `out` (any non-negative strides) and `workspace` (uint8, at least sizes(...)[2] bytes, 16-byte aligned) are used in
    place.  return_status: also the device int32 [4] {error word, segments decoded, segments expected, 1 if the recomputed Adler-32
    is the stored one}; it lives in the workspace's first bytes."""
    return _decode("decode_png", source, False, order, out, workspace, return_status)


def decode_depth_png(source: Union[bytes, Tensor, np.ndarray, DevicePng], *, out: Optional[Tensor] = None,
                     workspace: Optional[Tensor] = None, return_status: bool = False):
    """float32 [H, W, 1] metres from a depth file by _get_depth_from_image's rule (mtgs/dataset/custom_dataset.py:166-168):
    (float(b0) + float(b1) * 256.0f) * 0.01f with b0 and b1 OpenCV's channels 0 and 1 (the file's blue and green).  It runs inside
    the unfilter launch: no byte image is stored.  What encode_depth_png wrote comes back truncated to centimetres."""
    return _decode("decode_depth_png", source, True, "rgb", out, workspace, return_status)
