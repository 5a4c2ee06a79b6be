"""Baseline JPEG frames decoded on the device (include/mtgs_jpegdec.h, csrc/jpegdec.hip).

The first thing the reference does with every training frame is `Image.open(...)` followed by `np.array(...)`
(mtgs/dataset/custom_dataset.py:78-97): a host JPEG decode whose raw pixels then cross to the device.  Here the FILE crosses (a tenth
of the bytes or less) and the device decodes it; a cache of frames can stay compressed in device memory.

    parse_jpeg(data)                     -> JpegInfo      host only: the header's fields, the tables the kernels read, the scan's place
    upload_jpeg(data, device="cuda")     -> DeviceJpeg    the info, the scan's bytes and the tables on the device: a cache entry
    decode_jpeg(source, image_float=False, out=None, workspace=None, subsequence_bits=None, return_status=False)
                                         -> uint8 [H, W, 3] (float32 byte / 255 with image_float), optionally with the status words
    sizes(info, subsequence_bits=None)   -> workspace bytes

The pixels are byte for byte what `np.array(Image.open(...))` gives with Pillow 12.2.0 (libjpeg-turbo: integer islow IDCT, fancy
upsampling, 16-bit fixed-point colour) for what is accepted: 8-bit baseline sequential DCT (SOF0), three components read as YCbCr,
one interleaved scan, luma sampled 1x1 / 2x1 / 2x2 with chroma 1x1 ("4:4:4", "4:2:2", "4:2:0"), 8-bit quantisation tables, with or
without restart markers and with any Huffman tables.  Everything else is refused by name with NotImplementedError, a file that is
cut short with ValueError, both before any launch.  Exactness is claimed for files whose IDCT stays inside the library's sample
range, which every file an encoder writes does.  The brightness adjustment of the reference's loader (a dataset with
v_adjust_factors) and the undistortion (cv2.remap) take the decoded pixels on the device: mtgs_amd.brightness and mtgs_amd.undistort,
by rules the project defines (INTEGRATION.md sections 23 and 22).

From a DeviceJpeg, with `out` and `workspace` given, decode_jpeg makes no copy, no allocation and no host read.
"""
from __future__ import annotations

import ctypes as C
import re
from dataclasses import dataclass
from typing import Dict, Optional, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from . import _abi
from ._lib import call, ptr, require_gpu, stream_of

_ABI = _abi.header_abi("mtgs_jpegdec.h")
_K = _ABI.constants
TABLE_WORDS = _K["MTGS_JPEGDEC_TABLE_WORDS"]
FAST_BITS = _K["MTGS_JPEGDEC_FAST_BITS"]
RUN = _K["MTGS_JPEGDEC_RUN"]
SUBSEQUENCE_BITS = _K["MTGS_JPEGDEC_SUBSEQUENCE_BITS"]
STATUS_WORDS = _K["MTGS_JPEGDEC_STATUS_WORDS"]
ERR_MARKERS, ERR_BLOCKS = _K["MTGS_JPEGDEC_ERR_MARKERS"], _K["MTGS_JPEGDEC_ERR_BLOCKS"]
_SUBSAMPLINGS = {"4:4:4": _K["MTGS_JPEGDEC_444"], "4:2:2": _K["MTGS_JPEGDEC_422"], "4:2:0": _K["MTGS_JPEGDEC_420"]}
_SAMPLING = {(1, 1): "4:4:4", (2, 1): "4:2:2", (2, 2): "4:2:0"}
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])
_SOF_NAMES = {0xC1: "extended sequential DCT (SOF1)", 0xC2: "progressive DCT (SOF2)", 0xC3: "lossless (SOF3)",
              0xC5: "differential sequential DCT (SOF5)", 0xC6: "differential progressive DCT (SOF6)", 0xC7: "differential lossless (SOF7)",
              0xC9: "extended sequential DCT with arithmetic coding (SOF9)", 0xCA: "progressive DCT with arithmetic coding (SOF10)",
              0xCB: "lossless with arithmetic coding (SOF11)", 0xCD: "differential sequential DCT with arithmetic coding (SOF13)",
              0xCE: "differential progressive DCT with arithmetic coding (SOF14)", 0xCF: "differential lossless with arithmetic coding (SOF15)"}
_OTHER_NAMES = {0xC8: "JPG extension", 0xDE: "DHP, hierarchical progression", 0xDF: "EXP, hierarchical expansion"}
_SLOTS = ("dc0", "dc1", "ac0", "ac1")
_SCAN_END = re.compile(rb"\xff([\x01-\xcf\xd8-\xfe])")        # FF and a byte that is no stuffed zero, restart marker or fill byte


@dataclass
class JpegInfo:
    """What parse_jpeg read.  `quant` is int32 [3, 64], each component's table in NATURAL order; `huffman` maps "dc0" | "dc1" |
    "ac0" | "ac1" to (BITS, HUFFVAL) or None; `selectors` holds each component's (DC table, AC table); `tables` is the packed int32
    array the kernels read (include/mtgs_jpegdec.h); the scan is data[scan_offset : scan_offset + scan_length], EOI behind it."""
    height: int
    width: int
    subsampling: str
    restart_interval: int
    quant: np.ndarray
    huffman: Dict[str, Optional[Tuple[Tuple[int, ...], Tuple[int, ...]]]]
    selectors: Tuple[Tuple[int, int], ...]
    tables: np.ndarray
    scan_offset: int
    scan_length: int


@dataclass
class DeviceJpeg:
    """A compressed frame on the device: the entry of a compressed frame cache.  `scan` uint8 [scan_length], `tables` int32."""
    info: JpegInfo
    scan: Tensor
    tables: Tensor


def _huffman_words(bits, vals, out, slot) -> None:
    """fills the fast, maxcode, valoff and huffval words of one slot: Annex C's canonical codes"""
    fast = out[_K["MTGS_JPEGDEC_FAST_AT"] + (slot << FAST_BITS):][:1 << FAST_BITS]
    maxcode = out[_K["MTGS_JPEGDEC_MAXCODE_AT"] + slot * 18:][:18]
    valoff = out[_K["MTGS_JPEGDEC_VALOFF_AT"] + slot * 18:][:18]
    out[_K["MTGS_JPEGDEC_HUFFVAL_AT"] + slot * 256:][:len(vals)] = vals
    maxcode[:] = -1
    code, k = 0, 0
    for length in range(1, 17):
        n = bits[length - 1]
        if n:
            if code + n > (1 << length):
                raise ValueError(f"parse_jpeg: a Huffman table has more codes of {length} bits than fit")
            valoff[length] = k - code
            maxcode[length] = code + n - 1
            if length <= FAST_BITS:
                for j in range(n):
                    lo = (code + j) << (FAST_BITS - length)
                    fast[lo:lo + (1 << (FAST_BITS - length))] = (length << 8) | vals[k + j]
            code, k = code + n, k + n
        code <<= 1


def parse_jpeg(data: bytes) -> JpegInfo:
    """Reads SOI, the APPn / COM segments (skipped), DQT, SOF0, DHT, DRI and the SOS header, finds the scan and checks that EOI is
    there.  NotImplementedError names what this decoder does not read; ValueError a file that is cut short or malformed."""
    data = bytes(data)
    n = len(data)
    if n < 4 or data[:2] != b"\xff\xd8":
        raise ValueError("parse_jpeg: not a JPEG file (no SOI)")
    quant: Dict[int, np.ndarray] = {}
    huffman: Dict[str, Optional[tuple]] = {name: None for name in _SLOTS}
    frame = None                         # [(id, h, v, quant table)]
    restart, jfif, adobe = 0, False, None
    at = 2
    while True:
        if at + 2 > n:
            raise ValueError("parse_jpeg: the file is cut short: no SOS before its end")
        if data[at] != 0xFF:
            raise ValueError(f"parse_jpeg: no marker at byte {at} (0x{data[at]:02x})")
        while at + 1 < n and data[at + 1] == 0xFF:            # fill bytes in front of a marker
            at += 1
        if at + 2 > n:
            raise ValueError("parse_jpeg: the file is cut short: no SOS before its end")
        marker = data[at + 1]
        if marker == 0xD9:
            raise ValueError("parse_jpeg: EOI before any scan")
        if marker == 0x01 or 0xD0 <= marker <= 0xD8:
            raise ValueError(f"parse_jpeg: marker 0x{marker:02x} outside a scan")
        if at + 4 > n:
            raise ValueError("parse_jpeg: the file is cut short inside a segment header")
        length = int.from_bytes(data[at + 2:at + 4], "big")
        if length < 2 or at + 2 + length > n:
            raise ValueError(f"parse_jpeg: the file is cut short: the segment 0x{marker:02x} at byte {at} runs to byte {at + 2 + length} of {n}")
        body = data[at + 4:at + 2 + length]
        at += 2 + length
        if marker in _SOF_NAMES:
            raise NotImplementedError(f"parse_jpeg: {_SOF_NAMES[marker]} is not implemented (baseline sequential DCT, SOF0, only)")
        if marker == 0xCC:
            raise NotImplementedError("parse_jpeg: arithmetic coding (DAC) is not implemented")
        if marker == 0xDC:
            raise NotImplementedError("parse_jpeg: DNL (the height defined after the scan) is not implemented")
        if marker == 0xE0 and body[:5] == b"JFIF\x00":
            jfif = True
        elif marker == 0xEE and body[:5] == b"Adobe" and len(body) >= 12:
            adobe = body[11]
        elif marker == 0xDB:
            k = 0
            while k < len(body):
                pq, tq = body[k] >> 4, body[k] & 15
                if pq != 0:
                    raise NotImplementedError(f"parse_jpeg: a 16-bit quantisation table (DQT {tq}, precision {pq}) is not implemented")
                if tq > 3 or k + 65 > len(body):
                    raise ValueError("parse_jpeg: malformed DQT segment")
                table = np.zeros(64, dtype=np.int32)
                table[ZIGZAG] = np.frombuffer(body[k + 1:k + 65], dtype=np.uint8)
                quant[tq] = table
                k += 65
        elif marker == 0xC4:
            k = 0
            while k < len(body):
                if k + 17 > len(body):
                    raise ValueError("parse_jpeg: malformed DHT segment")
                tc, th = body[k] >> 4, body[k] & 15
                bits = tuple(body[k + 1:k + 17])
                count = sum(bits)
                if tc > 1 or count > 256 or k + 17 + count > len(body):
                    raise ValueError("parse_jpeg: malformed DHT segment")
                if th > 1:
                    raise NotImplementedError(f"parse_jpeg: Huffman table {th} is not implemented (a baseline file has tables 0 and 1)")
                huffman[_SLOTS[2 * tc + th]] = (bits, tuple(body[k + 17:k + 17 + count]))
                k += 17 + count
        elif marker == 0xDD:
            if len(body) != 2:
                raise ValueError("parse_jpeg: malformed DRI segment")
            restart = int.from_bytes(body, "big")
        elif marker == 0xC0:
            if frame is not None:
                raise ValueError("parse_jpeg: a second SOF")
            if len(body) < 6 or len(body) != 6 + 3 * body[5]:
                raise ValueError("parse_jpeg: malformed SOF0 segment")
            precision, height, width, nf = body[0], int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big"), body[5]
            if precision != 8:
                raise NotImplementedError(f"parse_jpeg: {precision}-bit samples are not implemented")
            if nf == 1:
                raise NotImplementedError("parse_jpeg: a grayscale file (1 component) is not implemented")
            if nf == 4:
                raise NotImplementedError("parse_jpeg: a file of four components (CMYK / YCCK) is not implemented")
            if nf != 3:
                raise NotImplementedError(f"parse_jpeg: {nf} components are not implemented")
            if height == 0:
                raise NotImplementedError("parse_jpeg: DNL (a height of 0 in SOF0) is not implemented")
            if width == 0:
                raise ValueError("parse_jpeg: a width of 0")
            frame = [(body[6 + 3 * c], body[7 + 3 * c] >> 4, body[7 + 3 * c] & 15, body[8 + 3 * c]) for c in range(3)]
        elif marker == 0xDA:
            break
        elif 0xE0 <= marker <= 0xEF or marker == 0xFE:
            pass                                               # APPn, COM
        else:
            raise NotImplementedError(f"parse_jpeg: the segment 0x{marker:02x} ({_OTHER_NAMES.get(marker, 'reserved')}) is not implemented")
    if frame is None:
        raise ValueError("parse_jpeg: SOS before SOF0")
    if len(body) < 1 or body[0] != 3 or len(body) != 10:
        raise NotImplementedError(f"parse_jpeg: more than one scan is not implemented (this scan holds {body[0] if body else 0} of 3 components)")
    if [body[1 + 2 * c] for c in range(3)] != [f[0] for f in frame]:
        raise NotImplementedError("parse_jpeg: a scan whose components are not in the frame's order is not implemented")
    if tuple(body[7:10]) != (0, 63, 0):
        raise NotImplementedError(f"parse_jpeg: spectral selection / successive approximation {tuple(body[7:10])} is not implemented")
    if not jfif and adobe is not None and adobe != 1:
        raise NotImplementedError(f"parse_jpeg: Adobe transform {adobe} is not implemented (YCbCr, transform 1, only)")
    if not jfif and adobe is None and bytes(f[0] for f in frame) == b"RGB":
        raise NotImplementedError("parse_jpeg: components named R, G, B (not YCbCr) are not implemented")
    sampling = [(f[1], f[2]) for f in frame]
    if sampling[0] not in _SAMPLING or sampling[1] != (1, 1) or sampling[2] != (1, 1):
        raise NotImplementedError("parse_jpeg: sampling factors " + ", ".join(f"{h}x{v}" for h, v in sampling) +
                                  " are not implemented (luma 1x1, 2x1 or 2x2 with chroma 1x1)")
    selectors = tuple((body[2 + 2 * c] >> 4, body[2 + 2 * c] & 15) for c in range(3))
    words = np.zeros(TABLE_WORDS, dtype=np.int32)
    for c in range(3):
        if frame[c][3] not in quant:
            raise ValueError(f"parse_jpeg: component {c} names quantisation table {frame[c][3]}, which the file does not define")
        words[_K["MTGS_JPEGDEC_QUANT_AT"] + 64 * c:][:64] = quant[frame[c][3]]
        td, ta = selectors[c]
        if td > 1 or ta > 1:
            raise NotImplementedError(f"parse_jpeg: Huffman table {max(td, ta)} is not implemented (a baseline file has tables 0 and 1)")
        if huffman[_SLOTS[td]] is None or huffman[_SLOTS[2 + ta]] is None:
            raise ValueError(f"parse_jpeg: component {c} names a Huffman table that the file does not define")
        words[_K["MTGS_JPEGDEC_SLOT_AT"] + 2 * c:][:2] = (td, 2 + ta)
    for slot, name in enumerate(_SLOTS):
        if huffman[name] is not None:
            _huffman_words(*huffman[name], words, slot)
    # the scan: up to the first marker that is neither a stuffed zero nor a restart marker nor a fill byte
    start = at
    found = _SCAN_END.search(data, start)
    if found is None:
        raise ValueError("parse_jpeg: the file is cut short: no EOI behind the scan")
    k, m = found.start(), found.group(1)[0]
    if m == 0xDC:
        raise NotImplementedError("parse_jpeg: DNL (the height defined after the scan) is not implemented")
    if m != 0xD9:
        raise NotImplementedError(f"parse_jpeg: more than one scan is not implemented (marker 0x{m:02x} follows the first)")
    if k == start:
        raise ValueError("parse_jpeg: an empty scan")
    return JpegInfo(height, width, _SAMPLING[sampling[0]], restart, np.stack([quant[f[3]] for f in frame]), huffman, selectors, words,
                    start, k - start)


def _bits(subsequence_bits) -> int:
    bits = SUBSEQUENCE_BITS if subsequence_bits is None else subsequence_bits
    if isinstance(bits, bool) or not isinstance(bits, int) or bits < 32 or bits > 65536 or bits % 32:
        raise ValueError(f"subsequence_bits must be a multiple of 32 in [32, 65536], got {subsequence_bits!r}")
    return bits


def sizes(info: JpegInfo, subsequence_bits: Optional[int] = None) -> int:
    """The bytes of workspace decode_jpeg needs for this file: the clean stream, the subsequence states, the coefficients, the planes"""
    ws = C.c_size_t(0)
    call("mtgs_jpegdec_sizes", info.height, info.width, _SUBSAMPLINGS[info.subsampling], info.restart_interval, info.scan_length,
         _bits(subsequence_bits), C.byref(ws))
    return ws.value


def _file_bytes(source) -> bytes:
    if isinstance(source, (bytes, bytearray, memoryview)):
        return bytes(source)
    if isinstance(source, Tensor):
        if source.dtype != torch.uint8 or source.dim() != 1 or source.is_cuda:
            raise TypeError("a file given as a tensor must be a host uint8 [n] tensor (or upload_jpeg's DeviceJpeg)")
        return source.contiguous().numpy().tobytes()
    if isinstance(source, np.ndarray):
        if source.dtype != np.uint8 or source.ndim != 1:
            raise TypeError("a file given as an array must be uint8 [n]")
        return source.tobytes()
    raise TypeError(f"source must be bytes, a host uint8 tensor or array, or a DeviceJpeg, got {type(source).__name__}")


def upload_jpeg(data, device="cuda") -> DeviceJpeg:
    """Parses the file on the host and puts its scan and its tables on the device"""
    data = _file_bytes(data)
    info = parse_jpeg(data)
    scan = np.frombuffer(data, dtype=np.uint8, count=info.scan_length, offset=info.scan_offset).copy()
    return DeviceJpeg(info, torch.from_numpy(scan).to(device), torch.from_numpy(info.tables).to(device))


def decode_jpeg(source: Union[bytes, Tensor, np.ndarray, DeviceJpeg], *, image_float: bool = False, out: Optional[Tensor] = None,
                workspace: Optional[Tensor] = None, subsequence_bits: Optional[int] = None, return_status: bool = False):
    """The pixels of a baseline JPEG file: uint8 [H, W, 3] on the device, or float32 byte / 255 (one correctly rounded division:
    get_gt_img, the rule of frame.resize_frame(image_float=True)).  `source` is the file (bytes, a host uint8 tensor or array: parsed
    and uploaded here) or a DeviceJpeg.  `out` ([H, W, 3] of the result's dtype, any non-negative strides) and `workspace` (uint8,
    at least sizes(info, subsequence_bits) bytes, 16-byte aligned) are used in place.  `subsequence_bits`: the length of the pieces
    the bit stream is decoded in (a multiple of 32; the default is the measured one).  return_status: also the device int32 [4]
    {error word, stream blocks decoded, blocks expected, synchronisation launches that changed an entry}; it lives in the
    workspace's first bytes."""
    bits = _bits(subsequence_bits)
    jpeg = source if isinstance(source, DeviceJpeg) else upload_jpeg(source)
    info = jpeg.info
    require_gpu(jpeg.scan, jpeg.tables)
    device = jpeg.scan.device
    if jpeg.scan.dtype != torch.uint8 or jpeg.scan.numel() != info.scan_length or not jpeg.scan.is_contiguous():
        raise ValueError("DeviceJpeg.scan must be the contiguous uint8 [scan_length] scan of its info")
    if jpeg.tables.dtype != torch.int32 or jpeg.tables.numel() != TABLE_WORDS or not jpeg.tables.is_contiguous() or jpeg.tables.device != device:
        raise ValueError(f"DeviceJpeg.tables must be the contiguous int32 [{TABLE_WORDS}] tables of its info, on {device}")
    dtype = torch.float32 if image_float else torch.uint8
    shape = (info.height, info.width, 3)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=device)
    elif not isinstance(out, Tensor) or tuple(out.shape) != shape or out.dtype != dtype or out.device != device:
        raise ValueError(f"out must be a {dtype} {list(shape)} tensor on {device}")
    elif any(s < 0 for s in out.stride()):
        raise ValueError(f"out must have non-negative strides, got {out.stride()}")
    if workspace is None:
        workspace = torch.empty(sizes(info, bits), dtype=torch.uint8, device=device)
    elif (not isinstance(workspace, Tensor) or workspace.dtype != torch.uint8 or workspace.dim() != 1 or not workspace.is_contiguous()
          or workspace.device != device):
        raise ValueError(f"workspace must be a contiguous uint8 [n] tensor on {device}")
    status = workspace[:4 * STATUS_WORDS].view(torch.int32)
    sy, sx, sc = out.stride()
    call("mtgs_jpegdec_decode", ptr(jpeg.scan), info.scan_length, ptr(jpeg.tables), info.height, info.width,
         _SUBSAMPLINGS[info.subsampling], info.restart_interval, bits, ptr(out), int(image_float), sy, sx, sc, ptr(status),
         ptr(workspace), workspace.numel(), stream_of(jpeg.scan))
    return (out, status) if return_status else out
