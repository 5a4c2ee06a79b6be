"""Lens undistortion of a training frame on the device (include/mtgs_undistort.h, csrc/undistort.hip).

CustomInputDataset._undistort_image (mtgs/dataset/custom_dataset.py:99-152) builds cv2.initUndistortRectifyMap on the host for every
frame and runs cv2.remap up to five times: INTER_LINEAR on the image, INTER_NEAREST on an all-255 plane (the valid mask), on the ego
mask, on the panoptic and on the semantic map.  stack_RGB_point_cloud.py:53,64 does the same in front of the painting.  Here the
camera is prepared once and a frame is ONE launch that evaluates the map per pixel and stores none:

    optimal_new_camera_matrix(K, D, size, alpha=1.0) -> (K_new, roi)            host, NumPy double
    undistort_camera(K, D, size, mode="optimal" | "keep_focal_length", new_K=None) -> UndistortCamera
    undistort_plane(x, cam, interpolation="linear" | "nearest", out_dtype=None)  one plane
    undistort_frame(cam, image=None, ego_mask=None, panoptic=None, semantic=None, image_float=False) -> dict
    undistort_map(cam) -> float32 [H, W, 2]

and the way back, for the evaluation dump in image_saving_mode = "nuplan" (include/mtgs_redistort.h, csrc/redistort.hip; DESIGN.md
section 24; mtgs_amd.evaldump strings it to the JPEG encoder) -- the same camera, the roles of its two sizes swapped:

    redistort_image(image, cam, iterations=5, conversion="truncate", map=None, out=None) -> uint8 [H_raw, W_raw, C]
    redistort_map(cam, iterations=5) -> float32 [H_raw, W_raw, 2]

[RECALLED] cv2 was not available to run.  The rule is OpenCV's as recalled and is this project's DEFINITION (the header states it in
full; tests/undistort_refs.py restates it in NumPy and pins it with known answers that need no recall); nothing here claims byte
equality with OpenCV.  Because the recalled getOptimalNewCameraMatrix cannot be checked, a caller may always pass a `new_K` of its
own -- and, to the kernel, a map of its own (`_launch(..., map=)`).  Sizes are (height, width) throughout -- NOTE OpenCV's own
argument is (width, height).

NOT covered: cubic interpolation (used only in front of UniDepth, generate_dense_depth.py:198-220), more than five distortion
coefficients (rational, thin-prism, tilt), decoding PNG files, RGBA images.  adjust_brightness, which the dataset runs in front of
the undistortion and the point stack behind it, is mtgs_amd.brightness.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from ._abi import header_abi
from ._inputs import image_plane, image_size, shape_of
from ._lib import call, ptr, require_gpu

_ABI = header_abi("mtgs_undistort.h")
MAX_ITERATIONS = header_abi("mtgs_redistort.h").constants["MTGS_REDISTORT_MAX_ITERATIONS"]
_CONVERSIONS = {k: header_abi("mtgs_present.h").constants["MTGS_PRESENT_U8_" + k.upper()] for k in ("truncate", "round")}
_PLANE = _ABI.structs["mtgs_undistort_plane"]
TILE_W, TILE_H = _ABI.constants["MTGS_UNDISTORT_TILE_W"], _ABI.constants["MTGS_UNDISTORT_TILE_H"]
MAX_PLANES = _ABI.constants["MTGS_UNDISTORT_MAX_PLANES"]
MAX_SIZE = _ABI.constants["MTGS_UNDISTORT_MAX_SIZE"]
_CAM_DOUBLES = _ABI.constants["MTGS_UNDISTORT_CAM_DOUBLES"]
_LINEAR, _NEAREST, _VALID = (_ABI.constants["MTGS_UNDISTORT_" + k] for k in ("LINEAR", "NEAREST", "VALID"))
_NEAREST_DTYPES = (torch.uint8, torch.int32, torch.bool)
_LONGER = {8: "rational (k4, k5, k6)", 12: "thin-prism (s1 .. s4)", 14: "tilt (tau_x, tau_y)"}


# ---- host: the camera ----------------------------------------------------------------------------------------------------------------
def _intrinsics(K, name: str) -> np.ndarray:
    """(fx, fy, cx, cy) in double from a 3 x 3 matrix or from the four numbers"""
    k = np.asarray(K.detach().cpu().numpy() if isinstance(K, Tensor) else K, dtype=np.float64)
    if k.shape == (3, 3):
        return np.array([k[0, 0], k[1, 1], k[0, 2], k[1, 2]])
    if k.shape == (4,):
        return k.copy()
    raise ValueError(f"{name} must be a 3 x 3 matrix or (fx, fy, cx, cy), got shape {k.shape}")


def _matrix(k: np.ndarray) -> np.ndarray:
    return np.array([[k[0], 0.0, k[2]], [0.0, k[1], k[3]], [0.0, 0.0, 1.0]])


def _distortion(D) -> np.ndarray:
    """(k1, k2, p1, p2, k3) in double; four coefficients have k3 = 0, longer models are refused by name"""
    d = np.asarray(D.detach().cpu().numpy() if isinstance(D, Tensor) else D, dtype=np.float64).reshape(-1)
    if d.size in _LONGER:
        raise NotImplementedError(f"D has {d.size} coefficients: the {_LONGER[d.size]} model is not implemented, only k1, k2, p1, p2[, k3]")
    if d.size not in (4, 5):
        raise ValueError(f"D must have 4 or 5 coefficients (k1, k2, p1, p2[, k3]), got {d.size}")
    return np.concatenate([d, np.zeros(5 - d.size)])


def _size(size, name: str) -> Tuple[int, int]:
    h, w = image_size(size, name)
    if h > MAX_SIZE or w > MAX_SIZE:
        raise ValueError(f"{name} must be at most {MAX_SIZE} on a side, got {tuple(size)}")
    return h, w


def _undistort_points(k: np.ndarray, d: np.ndarray, pts: np.ndarray) -> np.ndarray:
    """[RECALLED] undistortPoints without R and P: five fixed-point iterations of the inverse model"""
    k1, k2, p1, p2, k3 = d
    x0, y0 = (pts[:, 0] - k[2]) / k[0], (pts[:, 1] - k[3]) / k[1]
    x, y = x0.copy(), y0.copy()
    for _ in range(5):
        r2 = x * x + y * y
        icdist = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
        x, y = (x0 - dx) * icdist, (y0 - dy) * icdist
    return np.stack([x, y], axis=1)


def _rectangles(k: np.ndarray, d: np.ndarray, h: int, w: int, new_k: Optional[np.ndarray] = None, n: int = 9):
    """[RECALLED] icvGetRectangles: (inner, outer) = (x, y, width, height) of the undistorted n x n grid over [0, w-1] x [0, h-1], in
    normalised coordinates or in the pixels of new_k.  inner: the largest of the left column, the smallest of the right one (and
    rows likewise); outer: the bounding box."""
    g = np.arange(n, dtype=np.float64)
    xs, ys = np.meshgrid(g * (w - 1) / (n - 1), g * (h - 1) / (n - 1))
    p = _undistort_points(k, d, np.stack([xs.ravel(), ys.ravel()], axis=1))
    if new_k is not None:
        p = p * new_k[:2] + new_k[2:]
    px, py = p[:, 0].reshape(n, n), p[:, 1].reshape(n, n)
    ix0, ix1, iy0, iy1 = px[:, 0].max(), px[:, -1].min(), py[0, :].max(), py[-1, :].min()
    ox0, ox1, oy0, oy1 = px.min(), px.max(), py.min(), py.max()
    return (ix0, iy0, ix1 - ix0, iy1 - iy0), (ox0, oy0, ox1 - ox0, oy1 - oy0)


def optimal_new_camera_matrix(K, D, size: Tuple[int, int], alpha: float = 1.0):
    """[RECALLED] cv2.getOptimalNewCameraMatrix(K, D, (w, h), alpha) without centerPrincipalPoint -> (K_new 3 x 3 double, roi =
    (x, y, width, height)).  `size` is (height, width).  A 9 x 9 grid over [0, w-1] x [0, h-1] goes through five fixed-point
    iterations of the inverse model; alpha = 1 fits the grid's bounding box to the image (every source pixel is kept), alpha = 0 the
    inner rectangle (no invalid pixel is left), anything between interpolates the four intrinsics; the roi is the inner rectangle
    in the new camera's pixels through ceil (corner) and floor (extent), clipped to the image.  K is used as given: the half-pixel
    bookkeeping is undistort_camera's."""
    k, d = _intrinsics(K, "K"), _distortion(D)
    h, w = _size(size, "size")
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"alpha must be in [0, 1], got {alpha!r}")
    if h < 2 or w < 2:
        raise ValueError(f"size must be at least 2 x 2 to fit a camera, got {tuple(size)}")
    inner, outer = _rectangles(k, d, h, w)
    fit = lambda r: np.array([(w - 1) / r[2], (h - 1) / r[3], -((w - 1) / r[2]) * r[0], -((h - 1) / r[3]) * r[1]])
    new_k = fit(inner) * (1.0 - alpha) + fit(outer) * alpha
    x, y, rw, rh = _rectangles(k, d, h, w, new_k)[0]
    x0, y0 = int(np.ceil(x)), int(np.ceil(y))
    x1, y1 = x0 + int(np.floor(rw)), y0 + int(np.floor(rh))
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, w), min(y1, h)
    roi = (x0, y0, x1 - x0, y1 - y0) if x1 > x0 and y1 > y0 else (0, 0, 0, 0)
    return _matrix(new_k), roi


@dataclass(frozen=True)
class UndistortCamera:
    """One camera's undistortion, built once.  `params` is the DEVICE double[13] the kernels read (fx, fy, cx - 0.5, cy - 0.5 of
    the source, the same four of the new camera, k1, k2, p1, p2, k3); `new_K` (3 x 3 double, half pixel included) is what goes into
    the Cameras object; `roi` = (x, y, width, height); source_size and size are (height, width)."""
    params: Tensor
    K: np.ndarray
    D: np.ndarray
    new_K: np.ndarray
    roi: Tuple[int, int, int, int]
    source_size: Tuple[int, int]
    size: Tuple[int, int]
    mode: str

    @property
    def device(self):
        return self.params.device


def undistort_camera(K, D, size: Tuple[int, int], mode: str = "optimal", new_K=None, out_size: Optional[Tuple[int, int]] = None,
                     device="cuda") -> UndistortCamera:
    """The camera of `_undistort_image` for a source of `size` = (height, width).  K (3 x 3 or (fx, fy, cx, cy)) and the returned
    new_K are in the dataset's convention, pixel centres at +0.5: cx and cy are reduced by 0.5 before the map and the new cx', cy'
    increased by 0.5 again (custom_dataset.py:107-109, :131-132).  mode "optimal": new_K = optimal_new_camera_matrix of the reduced
    K, alpha = 1 [RECALLED]; "keep_focal_length": new_K = K, roi (0, 0, w, h).  A `new_K` of the caller's (same convention as K)
    replaces either; its roi is the whole image.  out_size: the destination size, the source size as in the reference when None.
    The scalars are uploaded with a blocking copy: build the camera before capturing a HIP graph."""
    if mode not in ("optimal", "keep_focal_length"):
        raise ValueError(f"mode must be 'optimal' or 'keep_focal_length', got {mode!r}")
    k, d = _intrinsics(K, "K"), _distortion(D)
    h, w = _size(size, "size")
    oh, ow = (h, w) if out_size is None else _size(out_size, "out_size")
    half = np.array([0.0, 0.0, 0.5, 0.5])
    k_map = k - half
    if new_K is not None:
        new_map, roi = _intrinsics(new_K, "new_K") - half, (0, 0, ow, oh)
    elif mode == "optimal":
        m, roi = optimal_new_camera_matrix(k_map, d, (h, w), 1.0)
        new_map = _intrinsics(m, "new_K")
    else:
        new_map, roi = k_map.copy(), (0, 0, w, h)
    host = np.concatenate([k_map, new_map, d])
    assert host.shape == (_CAM_DOUBLES,)
    params = torch.empty(_CAM_DOUBLES, dtype=torch.float64, device=device)
    params.copy_(torch.from_numpy(host))              # a blocking copy: complete before anything is captured
    return UndistortCamera(params, _matrix(k), d, _matrix(new_map + half), roi, (h, w), (oh, ow), mode)


# ---- device: the planes --------------------------------------------------------------------------------------------------------------
def _record(src: Optional[Tensor], dst: Tensor, op: int, channels: int = 1, out_float: bool = False) -> tuple:
    """one mtgs_undistort_plane in the struct's member order: src [h, w, C] in its own strides, dst contiguous"""
    return (0 if src is None else src.data_ptr(), dst.data_ptr(), (0, 0, 0) if src is None else tuple(src.stride()), op,
            1 if src is None else src.element_size(), channels, int(out_float))


def _launch(cam: UndistortCamera, records, stream, map: Optional[Tensor] = None) -> None:
    (h, w), (oh, ow) = cam.source_size, cam.size
    if len(records) > MAX_PLANES:
        raise ValueError(f"a launch takes at most {MAX_PLANES} planes, got {len(records)}")
    table = np.array(records, dtype=_PLANE)                 # HOST; copied into the launch before the call returns
    call("mtgs_undistort_frame", h, w, oh, ow, ptr(cam.params), ptr(map), len(records), table.ctypes.data, stream)


def _as_bytes(v: Tensor) -> Tensor:
    return v.view(torch.uint8) if v.dtype == torch.bool else v


def _check_cam(cam) -> None:
    if not isinstance(cam, UndistortCamera):
        raise TypeError(f"cam must be an UndistortCamera (undistort_camera), got {type(cam).__name__}")


def _check_plane(x, name: str, cam: UndistortCamera, interpolation: str, out_dtype=None):
    """(view [h, w, C], came as [h, w], dtype of the result) of one source plane, or the refusal"""
    if interpolation not in ("linear", "nearest"):
        hint = ": cubic is used only in front of UniDepth and is not implemented" if interpolation == "cubic" else ""
        raise ValueError(f"interpolation must be 'linear' or 'nearest', got {interpolation!r}{hint}")
    if interpolation == "nearest":
        v, flat = image_plane(x, name, _NEAREST_DTYPES)
        allowed = (v.dtype,)
    else:
        if isinstance(x, Tensor) and x.dim() == 3 and x.shape[2] == 4:
            raise NotImplementedError(f"{name} has 4 channels: RGBA images are not implemented (nuPlan frames are RGB)")
        v, flat = image_plane(x, name, (torch.uint8,), channels=(1, 3))
        allowed = (torch.uint8, torch.float32)
    if tuple(v.shape[:2]) != cam.source_size:
        raise ValueError(f"{name} must be {cam.source_size[0]} x {cam.source_size[1]}, the camera's source size, got {tuple(x.shape)}")
    if v.device != cam.device:
        raise RuntimeError(f"cam is on {cam.device}, {name} on {v.device}")
    out_dtype = v.dtype if out_dtype is None else out_dtype
    if out_dtype not in allowed:
        raise ValueError(f"out_dtype of a {interpolation} undistortion of {v.dtype} must be {' or '.join(map(str, allowed))}, got {out_dtype}")
    return v, flat, out_dtype


def _plane_record(v: Tensor, cam: UndistortCamera, interpolation: str, out_dtype):
    out = torch.empty(cam.size + (v.shape[2],), dtype=out_dtype, device=v.device)
    if interpolation == "linear":
        return out, _record(v, out, _LINEAR, v.shape[2], out_dtype == torch.float32)
    return out, _record(_as_bytes(v), _as_bytes(out), _NEAREST, v.shape[2])


def undistort_plane(x: Tensor, cam: UndistortCamera, interpolation: str = "linear", out_dtype=None) -> Tensor:
    """cv2.remap of one plane through the camera's map, by the project's rule [RECALLED].  x is [h, w] or [h, w, C] in any strides,
    also negative ones (a BGR image is rgb.flip(-1)).  "linear": uint8 with 1 or 3 channels, 8-bit INTER_LINEAR with five fractional
    bits; out_dtype torch.float32 gives byte / 255 as one correctly rounded division.  "nearest": uint8, int32 or bool with 1 to 3
    channels.  Outside the source the value is 0.  The result has x's rank and is contiguous."""
    _check_cam(cam)
    v, flat, out_dtype = _check_plane(x, "x", cam, interpolation, out_dtype)
    require_gpu(v)
    out, record = _plane_record(v, cam, interpolation, out_dtype)
    _launch(cam, [record], torch.cuda.current_stream(v.device).cuda_stream)
    return out[..., 0] if flat else out


def undistort_frame(cam: UndistortCamera, image: Optional[Tensor] = None, ego_mask: Optional[Tensor] = None,
                    panoptic: Optional[Tensor] = None, semantic: Optional[Tensor] = None, image_float: bool = False) -> Dict[str, Tensor]:
    """A whole frame in ONE launch:
        image       linear, uint8 [H, W, C] (float32 byte / 255 with image_float), when an image is given
        valid_mask  bool [H, W, 1]: the nearest source pixel is inside the source (`return_mask`), and, with an ego mask (uint8 or
                    bool, nonzero on the ego vehicle), the ego mask is 0 there (`_get_ego_mask` joined as get_data_and_camera does)
        panoptic    nearest, uint8 [H, W, 3]; semantic: nearest, uint8 [H, W] or [H, W, 1] as given
    valid_mask, panoptic and semantic feed frame.frame_masks(valid=...) unchanged; cam.new_K goes into the Cameras object."""
    _check_cam(cam)
    given = {"image": (image, "linear"), "panoptic": (panoptic, "nearest"), "semantic": (semantic, "nearest")}
    checked = {key: _check_plane(x, key, cam, how, torch.float32 if (key == "image" and image_float) else None)
               for key, (x, how) in given.items() if x is not None}
    ego = None
    if ego_mask is not None:
        ego = _as_bytes(_check_plane(ego_mask, "ego_mask", cam, "nearest")[0])
        if ego.dtype != torch.uint8 or ego.shape[2] != 1:
            raise ValueError(f"ego_mask must be uint8 or bool with one channel, got {ego_mask.dtype} {tuple(ego_mask.shape)}")
    if cam.device.type != "cuda":
        raise RuntimeError(f"mtgs_amd: cam must live on the HIP device (torch device 'cuda'); got {cam.device}. There is no CPU fallback.")
    valid = torch.empty(cam.size + (1,), dtype=torch.bool, device=cam.device)
    out, records = {"valid_mask": valid}, [_record(ego, valid.view(torch.uint8), _VALID)]
    for key, (v, flat, out_dtype) in checked.items():
        res, record = _plane_record(v, cam, given[key][1], out_dtype)
        out[key] = res[..., 0] if flat else res
        records.append(record)
    _launch(cam, records, torch.cuda.current_stream(cam.device).cuda_stream)
    return out


def undistort_map(cam: UndistortCamera) -> Tensor:
    """float32 [H, W, 2] = (mapx, mapy): the map the frame launch evaluates per pixel and never stores, for tests and for callers
    that want it (initUndistortRectifyMap(K, D, None, K', size, CV_32FC2) in the closed form of the header)"""
    _check_cam(cam)
    require_gpu(cam.params)
    out = torch.empty(cam.size + (2,), dtype=torch.float32, device=cam.device)
    call("mtgs_undistort_map", cam.size[0], cam.size[1], ptr(cam.params), ptr(out), torch.cuda.current_stream(cam.device).cuda_stream)
    return out


# ---- the way back: a rendered frame into the raw camera (include/mtgs_redistort.h) --------------------------
def _check_iterations(iterations) -> int:
    if isinstance(iterations, bool) or not isinstance(iterations, int) or not 0 <= iterations <= MAX_ITERATIONS:
        raise ValueError(f"iterations must be an integer in [0, {MAX_ITERATIONS}], got {iterations!r}")
    return iterations


def _check_redistort_map(map, cam: UndistortCamera) -> None:
    want = cam.source_size + (2,)
    if not isinstance(map, Tensor) or map.dtype != torch.float32 or tuple(map.shape) != want or not map.is_contiguous():
        got = f"{map.dtype} {tuple(map.shape)}" if isinstance(map, Tensor) else type(map).__name__
        raise ValueError(f"map must be a contiguous float32 {want} tensor (redistort_map), got {got}")
    if map.device != cam.device:
        raise RuntimeError(f"cam is on {cam.device}, map on {map.device}")


def _launch_redistort(cam: UndistortCamera, src: int, src_float: bool, strides, channels: int, out: Tensor, iterations: int,
                      conversion: str, map: Optional[Tensor], stream) -> None:
    """mtgs_redistort_frame on a source given as its base address and its (row, column, channel) strides in elements"""
    (h, w), (oh, ow) = cam.size, cam.source_size            # the roles are swapped: the new camera's image is read, the raw one written
    call("mtgs_redistort_frame", h, w, oh, ow, ptr(cam.params), iterations, ptr(map), src, int(src_float), _CONVERSIONS[conversion],
         *strides, channels, ptr(out), stream)


def redistort_map(cam: UndistortCamera, iterations: int = 5) -> Tensor:
    """float32 [H_raw, W_raw, 2] = (mapx, mapy): where each pixel of the RAW image lies in the undistorted one
    (initInverseRectificationMap(K, D, None, K', size) as `iterations` fixed-point iterations of the inverse lens model, in the form
    of include/mtgs_redistort.h [RECALLED]).  Pass it to redistort_image(map=) to read the map instead of evaluating it."""
    _check_cam(cam)
    iterations = _check_iterations(iterations)
    require_gpu(cam.params)
    out = torch.empty(cam.source_size + (2,), dtype=torch.float32, device=cam.device)
    call("mtgs_redistort_map", cam.source_size[0], cam.source_size[1], ptr(cam.params), iterations, ptr(out),
         torch.cuda.current_stream(cam.device).cuda_stream)
    return out


def redistort_image(image: Tensor, cam: UndistortCamera, iterations: int = 5, conversion: str = "truncate", map: Optional[Tensor] = None,
                    out: Optional[Tensor] = None) -> Tensor:
    """invert_distortion (mtgs/utils/camera_utils.py:340-356) on the device, by the project's rule [RECALLED]: `image`, uint8 or
    float32 [H, W, C] (C = 1 or 3, any strides) in the geometry of cam.size -- a rendered frame -- becomes uint8 [H_raw, W_raw, C] in
    the raw camera's geometry (cam.source_size), ONE launch.  `cam` is undistort_camera's, unchanged: it holds exactly the camera pair
    invert_distortion builds.  float32 is converted tap by tap as encode_jpeg converts ("truncate" is the evaluation dump's
    (x * 255).astype(uint8), "round" adds 0.5 first), then sampled with the 8-bit linear rule of undistort_plane; outside the image
    the value is 0.  `iterations` in [0, MAX_ITERATIONS]: 5 is the recalled rule and is up to 0.82 px off at the corners of a
    nuPlan-like lens (20: 2.2e-7 px; the header has the table); 0 is the plain change of camera.  `map` (redistort_map's, or the
    caller's own) is read instead of evaluating the iteration; `out` is written in place."""
    _check_cam(cam)
    iterations = _check_iterations(iterations)
    if conversion not in _CONVERSIONS:
        raise ValueError(f"conversion must be 'truncate' or 'round', got {conversion!r}")
    if isinstance(image, Tensor) and image.dim() == 3 and image.shape[2] == 4:
        raise NotImplementedError("image has 4 channels: RGBA images are not implemented (rendered frames are RGB)")
    if not isinstance(image, Tensor) or image.dim() != 3:
        raise ValueError(f"image must be [H, W, C], got {shape_of(image)}")
    v, _ = image_plane(image, "image", (torch.uint8, torch.float32), channels=(1, 3))
    if tuple(v.shape[:2]) != cam.size:
        raise ValueError(f"image must be {cam.size[0]} x {cam.size[1]}, the camera's size, got {tuple(image.shape)}")
    if v.device != cam.device:
        raise RuntimeError(f"cam is on {cam.device}, image on {v.device}")
    if map is not None:
        _check_redistort_map(map, cam)
    want = cam.source_size + (v.shape[2],)
    if out is not None:
        if not isinstance(out, Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != want or not out.is_contiguous() or out.device != v.device:
            got = f"{out.dtype} {tuple(out.shape)} on {out.device}" if isinstance(out, Tensor) else type(out).__name__
            raise ValueError(f"out must be a contiguous uint8 {want} tensor on {v.device}, got {got}")
    require_gpu(v)
    if out is None:
        out = torch.empty(want, dtype=torch.uint8, device=v.device)
    _launch_redistort(cam, v.data_ptr(), v.dtype == torch.float32, v.stride(), v.shape[2], out, iterations, conversion, map,
                      torch.cuda.current_stream(v.device).cuda_stream)
    return out


__all__ = ["optimal_new_camera_matrix", "undistort_camera", "undistort_plane", "undistort_frame", "undistort_map", "UndistortCamera",
           "redistort_map", "redistort_image", "TILE_W", "TILE_H", "MAX_PLANES", "MAX_SIZE", "MAX_ITERATIONS"]
