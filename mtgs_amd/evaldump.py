"""The evaluation image dump on the device: CustomPipeline._save_images
(mtgs/scene_model/custom_pipeline.py:91-143) takes every evaluated frame to the host (`.cpu().numpy() * 255.0`, `astype(uint8)`), in
mode "nuplan" bends it back into the raw camera with invert_distortion (cv2, mtgs/utils/camera_utils.py:340-356), and saves it with
Pillow at its defaults.  Here the frame stays where it was rendered until it is a file:

    eval_dump(image, mode, gt_image=None, cam=None, iterations=5, quality=75, subsampling="4:2:0", map=None) -> {name: JpegStream}
    eval_dump_paths(mode, travel_id, cam_name, cam_idx, raw_path) -> {name: relative path}                      host only

    mode                    streams
    "sequential"            rendered
    "sequential_with_gt"    rendered, gt_processed
    "nuplan"                rendered = encode_jpeg(redistort_image(image, cam, ...))

Every stream is encode_jpeg(conversion="truncate"): the bytes Pillow writes for (x * 255).astype(uint8).  JpegStream.tobytes() is the
one host read per file.  The re-distortion is the project's rule [RECALLED] (include/mtgs_redistort.h): nothing claims OpenCV's
bytes, and at the default 5 iterations the map is up to 0.82 px off at the corners of a nuPlan-like lens (20 iterations: 2.2e-7 px).
Writing the files, the directories and the `_gt.jpg` symbolic link stays the caller's: eval_dump_paths says where.
"""
from __future__ import annotations

from pathlib import Path
from typing import Dict, Optional

from torch import Tensor

from .jpeg import JpegStream, encode_jpeg
from .undistort import UndistortCamera, redistort_image

MODES = ("sequential", "sequential_with_gt", "nuplan")


def _check_mode(mode) -> None:
    if mode not in MODES:
        raise ValueError(f"mode must be one of {', '.join(repr(m) for m in MODES)}, got {mode!r}")


def eval_dump(image: Tensor, mode: str, gt_image: Optional[Tensor] = None, cam: Optional[UndistortCamera] = None, iterations: int = 5,
              quality: int = 75, subsampling: str = "4:2:0", map: Optional[Tensor] = None) -> Dict[str, JpegStream]:
    """The files of one evaluated frame as JPEG streams on the device.  `image` (and `gt_image`) are what get_image_metrics_and_images
    puts into images_dict: float32 [H, W, 3] in [0, 1] (uint8 is taken as it is).  "nuplan" needs `cam` (undistort_camera of the raw
    camera at full resolution) and an image of cam.size; `iterations` and `map` are redistort_image's.  The default evaluates the
    map inside the launch: profiles/redistort.txt has both forms."""
    _check_mode(mode)
    if mode == "nuplan":
        if cam is None:
            raise ValueError("mode 'nuplan' needs cam, the UndistortCamera of the raw camera (undistort_camera)")
        if gt_image is not None:
            raise ValueError("mode 'nuplan' writes the rendered frame only: gt_image must be None")
        raw = redistort_image(image, cam, iterations=iterations, conversion="truncate", map=map)
        return {"rendered": encode_jpeg(raw, quality, subsampling)}
    if cam is not None or map is not None:
        raise ValueError(f"cam and map belong to mode 'nuplan', got mode {mode!r}")
    if mode == "sequential_with_gt" and gt_image is None:
        raise ValueError("mode 'sequential_with_gt' needs gt_image")
    if mode == "sequential" and gt_image is not None:
        raise ValueError("mode 'sequential' writes the rendered frame only: gt_image must be None")
    out = {"rendered": encode_jpeg(image, quality, subsampling, conversion="truncate")}
    if mode == "sequential_with_gt":
        out["gt_processed"] = encode_jpeg(gt_image, quality, subsampling, conversion="truncate")
    return out


def eval_dump_paths(mode: str, travel_id=None, cam_name: Optional[str] = None, cam_idx: Optional[int] = None, raw_path=None) -> Dict[str, str]:
    """Where _save_images writes, relative to its output path.  The sequential modes need travel_id, cam_name (the stem of the
    camera's ego-mask file name) and cam_idx; "sequential_with_gt" and "nuplan" need raw_path, the raw image's file.
        "sequential"          rendered      traversal_{travel_id}/{cam_name}/{cam_idx}_rendered.jpg
        "sequential_with_gt"  + gt_processed   .../{cam_idx}_gt_processed.jpg
                              + gt             .../{cam_idx}_gt.jpg, a symbolic link to gt_target = the absolute raw_path
        "nuplan"              rendered      the last three parts of raw_path: {log}/{camera}/{token}.jpg"""
    _check_mode(mode)
    if mode == "nuplan":
        if raw_path is None:
            raise ValueError("mode 'nuplan' needs raw_path")
        parts = Path(raw_path).parts[-3:]
        if len(parts) < 3:
            raise ValueError(f"raw_path must end in {{log}}/{{camera}}/{{token}}.jpg, got {str(raw_path)!r}")
        return {"rendered": "/".join(parts)}
    for name, value in (("travel_id", travel_id), ("cam_name", cam_name), ("cam_idx", cam_idx)):
        if value is None:
            raise ValueError(f"mode {mode!r} needs {name}")
    folder = f"traversal_{travel_id}/{cam_name}"
    out = {"rendered": f"{folder}/{cam_idx}_rendered.jpg"}
    if mode == "sequential_with_gt":
        if raw_path is None:
            raise ValueError("mode 'sequential_with_gt' needs raw_path")
        out["gt_processed"] = f"{folder}/{cam_idx}_gt_processed.jpg"
        out["gt"] = f"{folder}/{cam_idx}_gt.jpg"
        out["gt_target"] = str(Path(raw_path).absolute())                  # as the reference: nothing is resolved or normalised
    return out


__all__ = ["eval_dump", "eval_dump_paths", "MODES"]
