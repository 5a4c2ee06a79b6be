"""MTGS's per-step image metrics on the device (csrc/metrics.hip): the colour-corrected PSNR, the PSNR and the lidar depth errors
that mtgs_scene_graph.py's get_metrics_dict computes on every training step and for every evaluation image.

    cc = color_correct(pred * mask, gt * mask)            # mtgs/utils/pnsr.py color_correct, mask applied as in the MTGS call
    m = image_metrics(pred, gt, mask, pred_depth=d, lidar_depth=ld)
    m["psnr"], m["cc_psnr"], m["depth_RMSE"], m["depth_absRel"], m["depth_delta1"]      # 0-dim fp32 device tensors

Forward only, no host reads (graph-capturable), bitwise reproducible.  The SSIM metric takes the loss's arguments
(use_ssim_on_raw_rgb=True): reuse mtgs_amd.loss.masked_ssim.  LPIPS (AlexNet) is mtgs_amd.lpips, re-exported here: `lpips`, `LpipsWeights`, and
image_metrics(..., lpips_weights=w)["lpips"].  The DINOv2 similarity is mtgs_amd.dino, re-exported here: `dino_similarity`, `DinoWeights`,
and image_metrics(..., dino_weights=w)["dinov2_sim"].
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
from torch import Tensor

from ._inputs import as_f32, image_pair
from ._lib import call, ptr, require_gpu, stream_of, workspace
from .dino import DinoWeights, dino_similarity
from .lpips import LpipsWeights, lpips

_EPS = 0.5 / 255


def _workspace(P: int, num_iters: int, dev) -> Tensor:
    return workspace("mtgs_metrics_workspace_bytes", P, num_iters, device=dev, dtype=torch.uint8)


def color_correct(img: Tensor, ref: Tensor, mask: Optional[Tensor] = None, num_iters: int = 5, eps: float = _EPS) -> Tensor:
    """The reference's color_correct(img * mask, ref * mask) (or color_correct(img, ref) without a mask) on [H, W, 3] images.
    If any fit is singular (a Cholesky pivot <= 1e-12 of its diagonal entry) or not finite, returns img * mask unchanged."""
    if num_iters < 0:
        raise ValueError(f"num_iters must be >= 0, got {num_iters}")
    img_c, ref_c, mask_c = image_pair(img, ref, mask, ("img", "ref"))
    H, W = img_c.shape[:2]
    out = torch.empty_like(img_c)
    if H * W == 0:
        return out
    ws = _workspace(H * W, num_iters, img_c.device)
    call("mtgs_color_correct", H * W, int(num_iters), float(eps), ptr(img_c), ptr(ref_c), ptr(mask_c), ptr(out),
         ptr(ws), ws.numel(), stream_of(img_c))
    return out


def image_metrics(pred: Tensor, gt: Tensor, mask: Optional[Tensor] = None, *, color_corrected: bool = True,
                  pred_depth: Optional[Tensor] = None, lidar_depth: Optional[Tensor] = None,
                  lpips_weights: Optional[LpipsWeights] = None, dino_weights: Optional[DinoWeights] = None) -> Dict[str, Tensor]:
    """get_metrics_dict's device metrics under MTGS's keys, as 0-dim fp32 tensors on pred's device:
    psnr = MaskedPSNR(data_range=1.0)(gt, pred, mask); cc_psnr (color_corrected) = the same of color_correct(pred * mask,
    gt * mask), without writing the corrected image; depth_RMSE, depth_absRel, depth_delta1 (both depths given) over the pixels
    with 0.1 < lidar < 80 and the mask.  Empty selections give nan, a zero error gives inf (as torch).
    lpips (lpips_weights given) = lpips(pred, gt, mask, weights=lpips_weights), LPIPS(normalize=True) of gt * mask and pred * mask.
    dinov2_sim (dino_weights given) = dino_similarity(pred, gt, mask, weights=dino_weights), DINOv2Similarity.similarity(pred, gt, mask)."""
    if (pred_depth is None) != (lidar_depth is None):
        raise ValueError("pred_depth and lidar_depth must be given together")
    pred_c, gt_c, mask_c = image_pair(pred, gt, mask)
    require_gpu(pred_depth, lidar_depth)
    H, W = pred_c.shape[:2]
    P = H * W
    depths = None
    if pred_depth is not None:
        if pred_depth.numel() != P or lidar_depth.numel() != P:
            raise ValueError(f"depths must have H * W = {P} elements, got {pred_depth.numel()} and {lidar_depth.numel()}")
        depths = (as_f32(pred_depth, H, W), as_f32(lidar_depth, H, W))
    num_iters = 5 if color_corrected else 0
    if P == 0:
        out = torch.full((5,), float("nan"), dtype=torch.float32, device=pred_c.device)
    else:
        out = torch.empty(5, dtype=torch.float32, device=pred_c.device)
        ws = _workspace(P, num_iters, pred_c.device)
        call("mtgs_image_metrics", P, num_iters, _EPS, ptr(pred_c), ptr(gt_c), ptr(mask_c),
             ptr(depths[0]) if depths else None, ptr(depths[1]) if depths else None, ptr(out), ptr(ws), ws.numel(), stream_of(pred_c))
    res = {"psnr": out[0]}
    if color_corrected:
        res["cc_psnr"] = out[1]
    if depths is not None:
        res.update(depth_RMSE=out[2], depth_absRel=out[3], depth_delta1=out[4])
    if lpips_weights is not None:
        res["lpips"] = lpips(pred, gt, mask, weights=lpips_weights)
    if dino_weights is not None:
        res["dinov2_sim"] = dino_similarity(pred, gt, mask, weights=dino_weights)
    return res
