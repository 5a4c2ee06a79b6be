"""Presenting rendered frames on the device (include/mtgs_present.h, csrc/present.hip).

After get_outputs_for_camera returns, the viewer thread (custom_viewer/render_state_machine.py:174-190, 240-310) and the offline
render tool (tools/render.py:131-165) finish every frame in PyTorch and on the host: nerfstudio's apply_colormap /
apply_depth_colormap (two `float(torch.min / max)` host reads, a dozen element-wise kernels, a 256-entry colour table rebuilt from a
Python list and uploaded on EVERY call), the split view's torch.cat and column fill, `(x * 255).type(torch.uint8)`, `.cpu()`,
np.pad to the client's aspect, np.concatenate of the outputs, and F.interpolate of the depth for the viewer's compositing.  Here a
frame is at most two launches (the extrema the colormaps take from the data, then the whole frame) and the resized depth one; no
host read, and with `out=` no allocation, so a frame can be captured in a HIP graph.

    colorize(image, options)                      apply_colormap          float32 [H, W, 3]
    colorize_depth(depth, accumulation, ...)      apply_depth_colormap    float32 [H, W, 3]   (the eval image, mtgs_scene_graph.py:1100)
    viewer_frame(outputs, output_render, ...)     _send_output_to_viewer  uint8 [H + 2 ph, W + 2 pw, 3], split and padding included
    viewer_depth(depth, state, scale_ratio)       gl_z_buf_depth * viser_scale_ratio          float32 [h, w, 1]
    render_frame(outputs, names, ...)             the render tool's concatenated frame        uint8 [H, sum W, 3]

nerfstudio (colormaps.py, version 1.1.5) is not part of the reference tree: what it computes is recalled ([NS-RECALL] in SURVEY.md's
sense) and stated operation by operation in include/mtgs_present.h; tests/present_refs.py holds both a NumPy restatement of that
statement and a torch transcription of the recalled functions.  The layout arithmetic (split_index, pad_sizes, depth_size,
concat_columns) is plain Python and needs no device.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from . import _abi
from ._inputs import shape_of
from ._lib import call, ptr, require_gpu, scratch, stream_of
from .jpeg import JpegStream, encode_jpeg

_ABI = _abi.header_abi("mtgs_present.h")
_PANEL = _ABI.structs["mtgs_present_panel"]
MAX_PANELS = _ABI.constants["MTGS_PRESENT_MAX_PANELS"]
_RGB, _FLOAT, _DEPTH, _BOOL = (_ABI.constants["MTGS_PRESENT_" + k] for k in ("RGB", "FLOAT", "DEPTH", "BOOL"))
_U8_TRUNCATE, _U8_ROUND, _F32 = (_ABI.constants["MTGS_PRESENT_" + k] for k in ("U8_TRUNCATE", "U8_ROUND", "F32"))
_WS_BYTES = _ABI.constants["MTGS_PRESENT_MAX_PANELS"] * _ABI.constants["MTGS_PRESENT_STAT_BLOCKS"] * 2 * 4

SPLIT_COLOR = (0.133, 0.157, 0.192)                 # render_state_machine.py:274
DEPTH_PIXELS = {"low_move": 128, "low_static": 128, "high": 512}   # render_state_machine.py:180, squared


@dataclass(frozen=True)
class ColormapOptions:
    """nerfstudio's ColormapOptions: the same fields and defaults.  `colormap` is a name ("default" = "turbo", "gray", or a table
    matplotlib lists colours for: turbo, viridis, magma, inferno, cividis, plasma) or a float32 [256, 3] tensor on the device."""
    colormap: Union[str, Tensor] = "default"
    normalize: bool = False
    colormap_min: float = 0.0
    colormap_max: float = 1.0
    invert: bool = False


# ---- the colour tables: built once per name on the host, uploaded once per (name, device) ----------------------------------------
_TABLES: Dict[str, np.ndarray] = {}
_DEVICE_TABLES: Dict[Tuple[str, torch.device], Tensor] = {}


def _as_table(colors, what) -> np.ndarray:
    table = np.ascontiguousarray(np.asarray(colors, dtype=np.float32))
    if table.shape != (256, 3):
        raise ValueError(f"colormap {what}: a table must be [256, 3], got {list(table.shape)}")
    return table


def register_colormap(name: str, colors) -> None:
    """Names a [256, 3] table of one's own (or supplies a matplotlib one where matplotlib is not installed).  Replaces the table
    of that name; the device copies of the old one are dropped."""
    if name in ("default", "gray"):
        raise ValueError(f"register_colormap: {name!r} is reserved")
    _TABLES[name] = _as_table(colors, repr(name))
    for key in [k for k in _DEVICE_TABLES if k[0] == name]:
        del _DEVICE_TABLES[key]


def _host_table(name: str) -> np.ndarray:
    if name not in _TABLES:
        import matplotlib                       # lazily: only a named table that nobody registered needs it
        try:
            colors = matplotlib.colormaps[name].colors
        except (KeyError, AttributeError):
            raise ValueError(f"colormap {name!r}: matplotlib has no listed colormap of that name") from None
        _TABLES[name] = _as_table(colors, repr(name))
    return _TABLES[name]


def colormap_table(colormap: Union[str, Tensor], device) -> Optional[Tensor]:
    """The device table of a ColormapOptions.colormap: None for "gray", the tensor itself if one is given, otherwise the cached
    upload of the named table (one upload per name and device, ever -- the reference uploads it on every call)."""
    if isinstance(colormap, Tensor):
        if colormap.dtype != torch.float32 or tuple(colormap.shape) != (256, 3) or not colormap.is_contiguous():
            raise ValueError(f"colormap: a tensor must be contiguous float32 [256, 3], got {colormap.dtype} {list(colormap.shape)}")
        return colormap
    name = "turbo" if colormap == "default" else colormap
    if name == "gray":
        return None
    device = torch.device(device)
    key = (name, device)
    if key not in _DEVICE_TABLES:
        _DEVICE_TABLES[key] = torch.from_numpy(_host_table(name)).to(device)
    return _DEVICE_TABLES[key]


# ---- layout arithmetic: plain Python -------------------------------------------------------------------------------------------
def split_index(split_percentage: float, width: int) -> int:
    """render_state_machine.py:269-272: the first column of the split output, which is also the column of the divider"""
    return min(int(split_percentage * width), width - 1)


def pad_sizes(height: int, width: int, aspect: Optional[float]) -> Tuple[int, int]:
    """(pad_height, pad_width) added on EACH side so that the frame has the client's aspect W / H (render_state_machine.py:285-296):
    nothing unless one of them exceeds 5."""
    if aspect is None:
        return 0, 0
    pad_width = int(max(0, (aspect * height - width) // 2))
    pad_height = int(max(0, (width / aspect - height) // 2))
    return (pad_height, pad_width) if pad_width > 5 or pad_height > 5 else (0, 0)


def depth_size(height: int, width: int, state: str) -> Tuple[int, int]:
    """(h, w) of the viewer's gl_z_buf_depth (render_state_machine.py:180-188): about 128^2 pixels while moving or in a low static
    frame, 512^2 in a high one, never enlarged.  Note that the SIDES scale by the ratio of the pixel counts, as the reference's do."""
    if state not in DEPTH_PIXELS:
        raise ValueError(f"state must be one of {sorted(DEPTH_PIXELS)}, got {state!r}")
    scale = min(DEPTH_PIXELS[state] ** 2 / max(1, height * width), 1.0)
    return int(height * scale), int(width * scale)


def concat_columns(widths: Sequence[int]) -> List[int]:
    """first output column of each panel of a np.concatenate(axis=1)"""
    out, at = [], 0
    for w in widths:
        out.append(at)
        at += w
    return out


# ---- panels ------------------------------------------------------------------------------------------------------------------------
@dataclass
class _Source:
    """one output of the model on its way into a panel: what apply_colormap / apply_depth_colormap would do with it"""
    image: Tensor
    kind: int
    options: ColormapOptions
    accumulation: Optional[Tensor] = None
    near: Optional[float] = None
    far: Optional[float] = None

    @property
    def height(self):
        return self.image.shape[0]

    @property
    def width(self):
        return self.image.shape[1]


def _source(image: Tensor, options: ColormapOptions, name: str) -> _Source:
    """apply_colormap's dispatch on the channel count and dtype"""
    if not isinstance(image, Tensor) or image.dim() != 3:
        raise ValueError(f"{name} must be a [H, W, C] tensor, got {shape_of(image)}")
    if not image.is_contiguous():
        raise ValueError(f"{name} must be contiguous (shape {tuple(image.shape)}, strides {image.stride()})")
    if image.shape[0] < 1 or image.shape[1] < 1:
        raise ValueError(f"{name} must have at least one pixel, got {tuple(image.shape)}")
    channels = image.shape[-1]
    if channels == 3:
        if image.dtype != torch.float32:
            raise TypeError(f"{name}: a 3-channel image must be float32, got {image.dtype}")
        return _Source(image, _RGB, options)
    if channels == 1 and image.dtype == torch.float32:
        return _Source(image, _FLOAT, options)
    if channels == 1 and image.dtype in (torch.bool, torch.uint8):
        return _Source(image, _BOOL, options)
    if channels > 3:
        raise NotImplementedError(f"{name} has {channels} channels: the PCA colormap (apply_pca_colormap) is not implemented")
    raise NotImplementedError(f"{name}: no colormap for {channels} channel(s) of {image.dtype} (float32 [H, W, 1] or [H, W, 3], bool [H, W, 1])")


def _depth_source(depth: Tensor, accumulation, near, far, options, name="depth") -> _Source:
    s = _source(depth, options, name)
    if s.kind != _FLOAT:
        raise TypeError(f"{name} must be float32 [H, W, 1], got {depth.dtype} {tuple(depth.shape)}")
    if accumulation is not None:
        if accumulation.dtype != torch.float32 or tuple(accumulation.shape) != tuple(depth.shape) or not accumulation.is_contiguous():
            raise ValueError(f"accumulation must be contiguous float32 {tuple(depth.shape)}, got {accumulation.dtype} {tuple(accumulation.shape)}")
    return _Source(depth, _DEPTH, options, accumulation, None if near is None else float(near), None if far is None else float(far))


def _compose(sources: Sequence[_Source], places, out_h: int, out_w: int, split_column: int, fmt: int, out: Optional[Tensor]) -> Tensor:
    """places[j] = (y0, x0, h, w, src_x0) of sources[j].  The stats launch if a panel takes extrema from the data, then the frame."""
    if len(sources) > MAX_PANELS:
        raise ValueError(f"{len(sources)} panels: a frame holds at most {MAX_PANELS}")
    dtype = torch.float32 if fmt == _F32 else torch.uint8
    first = sources[0].image
    if out is not None:
        if out.dtype != dtype or tuple(out.shape) != (out_h, out_w, 3) or not out.is_contiguous() or out.device != first.device:
            raise ValueError(f"out must be contiguous {dtype} [{out_h}, {out_w}, 3] on {first.device}, got {out.dtype} {tuple(out.shape)} on {out.device}")
    tensors = [t for s in sources for t in (s.image, s.accumulation)]
    require_gpu(*tensors)
    if any(t is not None and t.device != first.device for t in tensors):
        raise ValueError("every panel's tensors must be on one device")
    table = np.zeros(len(sources), dtype=_PANEL)
    luts = []
    needs_stats = False
    for row, s, (y0, x0, h, w, src_x0) in zip(table, sources, places):
        o = s.options
        lut = colormap_table(o.colormap, first.device) if s.kind in (_FLOAT, _DEPTH) else None
        if lut is not None:
            require_gpu(lut)
        luts.append(lut)
        row["src"], row["accumulation"], row["lut"] = s.image.data_ptr(), ptr(s.accumulation) or 0, ptr(lut) or 0
        row["near_plane"] = math.nan if s.near is None else s.near
        row["far_plane"] = math.nan if s.far is None else s.far
        row["colormap_min"], row["colormap_max"] = float(o.colormap_min), float(o.colormap_max)
        row["kind"], row["normalize"], row["invert"] = s.kind, bool(o.normalize), bool(o.invert)
        row["src_h"], row["src_w"], row["src_x0"] = s.height, s.width, src_x0
        row["y0"], row["x0"], row["h"], row["w"] = y0, x0, h, w
        needs_stats |= (s.kind == _DEPTH and (s.near is None or s.far is None)) or (s.kind in (_FLOAT, _DEPTH) and bool(o.normalize))
    stream = stream_of(first)
    if out is None:
        out = torch.empty((out_h, out_w, 3), dtype=dtype, device=first.device)
    # the 16 KB of partial extrema, one per (device, stream): allocated once, so that a frame with `out=` allocates nothing
    ws = scratch(("present",), _WS_BYTES, first.device, stream) if needs_stats else None
    panels = table.ctypes.data_as(C.c_void_p)
    if needs_stats:
        call("mtgs_present_stats", len(sources), panels, ptr(ws), ws.numel(), stream)
    call("mtgs_present_compose", len(sources), panels, out_h, out_w, split_column, (C.c_float * 3)(*SPLIT_COLOR), fmt, ptr(out), ptr(ws),
         0 if ws is None else ws.numel(), stream)
    return out


def _whole(s: _Source):
    return (0, 0, s.height, s.width, 0)


# ---- the public functions ------------------------------------------------------------------------------------------------------------
def colorize(image: Tensor, options: ColormapOptions = ColormapOptions(), out: Optional[Tensor] = None) -> Tensor:
    """nerfstudio's apply_colormap: float32 [H, W, 3].  A 3-channel image is returned as it is (the reference returns the tensor
    itself), a float [H, W, 1] goes through the float colormap, a bool [H, W, 1] becomes white / black."""
    s = _source(image, options, "image")
    if s.kind == _RGB and out is None:
        return image
    return _compose([s], [_whole(s)], s.height, s.width, -1, _F32, out)


def colorize_depth(depth: Tensor, accumulation: Optional[Tensor] = None, near_plane: Optional[float] = None,
                   far_plane: Optional[float] = None, options: ColormapOptions = ColormapOptions(), out: Optional[Tensor] = None) -> Tensor:
    """nerfstudio's apply_depth_colormap: float32 [H, W, 3].  near_plane / far_plane None = the depth's min / max, taken on the
    device (the reference reads them to the host)."""
    s = _depth_source(depth, accumulation, near_plane, far_plane, options)
    return _compose([s], [_whole(s)], s.height, s.width, -1, _F32, out)


def viewer_frame(outputs: Dict[str, Tensor], output_render: str, options: ColormapOptions = ColormapOptions(),
                 split_output_render: Optional[str] = None, split_options: Optional[ColormapOptions] = None,
                 split_percentage: float = 0.5, client_aspect: Optional[float] = None, out: Optional[Tensor] = None,
                 jpeg_quality: Optional[int] = None, jpeg_out: Optional[JpegStream] = None) -> Union[Tensor, JpegStream]:
    """The uint8 frame RenderStateMachine._send_output_to_viewer hands to the client (render_state_machine.py:251-296): the
    selected output through apply_colormap; with `split_output_render` the split view (the split output from column split_index on,
    that column in SPLIT_COLOR); `(x * 255).type(torch.uint8)`; zero padding to `client_aspect` (W / H) by pad_sizes' rule.  `out`
    (uint8 [H + 2 ph, W + 2 pw, 3]) is written in place: nothing is allocated.  With `jpeg_quality` (set_background_image's
    jpeg_quality) the frame is encoded where it lies and its JpegStream is returned instead (mtgs_amd.jpeg, 4:2:0; `jpeg_out` is
    encoded into in place); None leaves everything as it is."""
    if output_render not in outputs:
        raise KeyError(f"output_render {output_render!r} is not among the outputs {sorted(outputs)}")
    a = _source(outputs[output_render], options, f"outputs[{output_render!r}]")
    H, W = a.height, a.width
    ph, pw = pad_sizes(H, W, client_aspect)
    if split_output_render is None:
        sources, places, column = [a], [(ph, pw, H, W, 0)], -1
    else:
        if split_output_render not in outputs:
            raise KeyError(f"split_output_render {split_output_render!r} is not among the outputs {sorted(outputs)}")
        b = _source(outputs[split_output_render], split_options or ColormapOptions(), f"outputs[{split_output_render!r}]")
        if (b.height, b.width) != (H, W):
            raise ValueError(f"split_output_render {split_output_render!r} is {b.height} x {b.width}, output_render {output_render!r} {H} x {W}")
        k = split_index(split_percentage, W)
        sources, places, column = [a, b], [(ph, pw, H, k, 0), (ph, pw + k, H, W - k, k)], pw + k
    frame = _compose(sources, places, H + 2 * ph, W + 2 * pw, column, _U8_TRUNCATE, out)
    return frame if jpeg_quality is None else encode_jpeg(frame, jpeg_quality, out=jpeg_out)


def viewer_depth(depth: Tensor, state: str, scale_ratio: float = 1.0, out: Optional[Tensor] = None) -> Tensor:
    """outputs["gl_z_buf_depth"] * viser_scale_ratio (render_state_machine.py:174-190, 277-279): depth [H, W, 1] resized bilinearly
    (align_corners = False) to depth_size(H, W, state), times scale_ratio: float32 [h, w, 1], on the device."""
    if not isinstance(depth, Tensor) or depth.dim() != 3 or depth.shape[-1] != 1 or depth.dtype != torch.float32:
        raise ValueError(f"depth must be float32 [H, W, 1], got {getattr(depth, 'dtype', None)} {tuple(getattr(depth, 'shape', ()))}")
    if not depth.is_contiguous():
        raise ValueError(f"depth must be contiguous (shape {tuple(depth.shape)}, strides {depth.stride()})")
    H, W = depth.shape[:2]
    h, w = depth_size(H, W, state)
    if out is not None and (out.dtype != torch.float32 or tuple(out.shape) != (h, w, 1) or not out.is_contiguous() or out.device != depth.device):
        raise ValueError(f"out must be contiguous float32 [{h}, {w}, 1] on {depth.device}, got {out.dtype} {tuple(out.shape)} on {out.device}")
    require_gpu(depth)
    if out is None:
        out = torch.empty((h, w, 1), dtype=torch.float32, device=depth.device)
    call("mtgs_present_depth_resize", H, W, ptr(depth), h, w, float(scale_ratio), ptr(out), stream_of(depth))
    return out


def render_frame(outputs: Dict[str, Tensor], rendered_output_names: Sequence[str], depth_near_plane: Optional[float] = None,
                 depth_far_plane: Optional[float] = None, options: ColormapOptions = ColormapOptions(), out: Optional[Tensor] = None,
                 jpeg_quality: Optional[int] = None, jpeg_out: Optional[JpegStream] = None) -> Union[Tensor, JpegStream]:
    """The render tool's frame (tools/render.py:131-165): every named output coloured -- a name containing "depth" through
    apply_depth_colormap with outputs["accumulation"] and the given planes, the others through apply_colormap -- and concatenated
    along the width, as uint8 [H, sum W, 3] by the rounding conversion (clip(x, 0, 1) * 255 + 0.5, truncated).  With
    `jpeg_quality` (tools/render.py:729-734, media.write_image(fmt="jpeg", quality=)) the JpegStream of that frame is returned
    instead, as from viewer_frame."""
    if len(rendered_output_names) == 0:
        raise ValueError("rendered_output_names is empty")
    if len(rendered_output_names) > MAX_PANELS:
        raise ValueError(f"rendered_output_names: {len(rendered_output_names)} panels: a frame holds at most {MAX_PANELS}")
    sources = []
    for name in rendered_output_names:
        if name not in outputs:
            raise KeyError(f"could not find {name!r} in the model outputs {sorted(outputs)}")
        if "depth" in name:
            if "accumulation" not in outputs:
                raise KeyError(f"{name!r} takes the depth colormap, which needs outputs['accumulation']")
            sources.append(_depth_source(outputs[name], outputs["accumulation"], depth_near_plane, depth_far_plane, options, f"outputs[{name!r}]"))
        else:
            sources.append(_source(outputs[name], options, f"outputs[{name!r}]"))
    H = sources[0].height
    for name, s in zip(rendered_output_names, sources):
        if s.height != H:
            raise ValueError(f"outputs[{name!r}] has {s.height} rows, outputs[{rendered_output_names[0]!r}] has {H}: panels side by side need one height")
    columns = concat_columns([s.width for s in sources])
    places = [(0, x0, H, s.width, 0) for x0, s in zip(columns, sources)]
    frame = _compose(sources, places, H, columns[-1] + sources[-1].width, -1, _U8_ROUND, out)
    return frame if jpeg_quality is None else encode_jpeg(frame, jpeg_quality, out=jpeg_out)
