#!/usr/bin/env python3
"""BASELINE configs[4] in miniature, on synthetic data (no nuPlan road block can reach the GPU box): an MTGS-style
training iteration -- shared static nodes with per-traversal appearance (a multi-colour background node with T
traversals + a vanilla road node), one camera / traversal per step, node activations -> rasterization (RGB+ED,
antialiased, absgrad) -> background composite -> 0.8 L1 + 0.2 (1 - masked SSIM) -> backward -> densification
statistics -> Adam -- run two ways on the same parameters:

  chain : the PyTorch operator chains MTGS runs around the drop-in rasterizer (exp / normalize / sigmoid / cat / SH op /
          clamp; SSIM as 5 grouped convolutions x 2; masked-tensor statistics), i.e. MTGS unchanged on this library;
  fused : mtgs_amd.nodes.node_gaussians, mtgs_amd.loss.masked_l1 / masked_ssim, mtgs_amd.densify.update_statistics.

Prints the per-iteration GPU time of both and checks that they compute the same loss.  `--steps` > 0 also trains
(fused) and prints the loss curve.
"""
import argparse
import json
import math
import os
import sys
import time
from pathlib import Path

# A TRAINER opts into the tight tile lists (mtgs_amd.tight_lists: same pixels and gradients, shorter lists): rasterization()'s own
# default is gsplat's lists.  Process-wide here (every thread of this script, the `--dp` ranks are processes); MTGS_TIGHT_LISTS=0
# runs the script on gsplat's lists.
os.environ.setdefault("MTGS_TIGHT_LISTS", "1")

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from mtgs_amd import rasterization, spherical_harmonics  # noqa: E402
from mtgs_amd.densify import update_statistics, update_statistics_all  # noqa: E402
from mtgs_amd.loss import (combine_losses, depth_ncc_loss, depth_normal_loss, inverse_depth_l1, masked_l1, masked_ssim,  # noqa: E402
                           output_head, scale_regularizers, tv_loss)
from mtgs_amd.nodes import camera_space_normals, node_gaussians  # noqa: E402
from mtgs_amd.synthetic import make_camera  # noqa: E402


FRAMES = 40   # frames of an object's pose parameters


def make_nodes(n_bg, n_road, T, seed, dev, n_objects=0, object_size=3000, clear=0.0):
    """clear > 0: nothing within that many metres (in the ground plane) of the cameras' position, the origin -- as on a road
    block, where the cameras ride on a car and nothing is splatted a metre in front of the lens."""
    g = torch.Generator().manual_seed(seed)
    def place(n, extent, y0):
        m = (torch.rand(n, 3, generator=g) * 2 - 1) * torch.tensor(extent) + torch.tensor([0.0, y0, 0.0])
        if clear > 0:
            r = m[:, [0, 2]].norm(dim=-1, keepdim=True).clamp_min(1e-6)
            m[:, [0, 2]] = m[:, [0, 2]] * torch.clamp(clear / r, min=1.0)
        return m
    def base(n, extent, y0):
        return {"means": place(n, extent, y0),
                "scales": torch.log(torch.exp(torch.rand(n, 3, generator=g) * (math.log(0.25) - math.log(0.03)) + math.log(0.03))),
                "quats": torch.randn(n, 4, generator=g), "opacities": torch.randn(n, 1, generator=g) + 1.0,
                "features_dc": (torch.rand(n, 3, generator=g) - 0.5) / 0.2820947917738781}
    bg = base(n_bg, (40.0, 6.0, 40.0), 0.0)
    bg["features_rest"] = 0.05 * torch.randn(n_bg, T, 15, 3, generator=g)
    bg["features_adapters"] = 0.1 * torch.randn(n_bg, T, 3, generator=g)
    road = base(n_road, (40.0, 0.2, 40.0), 1.6)
    road["features_rest"] = 0.05 * torch.randn(n_road, 15, 3, generator=g)
    nodes = {"background": bg, "road": road}
    for i in range(n_objects):   # rigid object nodes (rigid_node.py): Gaussians in the object frame + one pose per frame
        n = max(1, int(object_size * (0.3 + 1.4 * torch.rand(1, generator=g).item())))
        ob = base(n, (1.0, 0.8, 2.2), 0.0)
        ob["scales"] = ob["scales"] - 0.7
        ob["features_rest"] = 0.05 * torch.randn(n, 15, 3, generator=g)
        centre = (torch.rand(3, generator=g) * 2 - 1) * torch.tensor([30.0, 0.0, 30.0]) + torch.tensor([0.0, 0.8, 0.0])
        drift = torch.linspace(0, 1, FRAMES)[:, None] * torch.tensor([0.0, 0.0, 3.0])
        ob["instance_trans"] = centre + drift
        ob["instance_quats"] = torch.tensor([1.0, 0.0, 0.3, 0.0]) * (1.0 + 0.2 * torch.rand(FRAMES, 1, generator=g)) \
            + 0.05 * torch.randn(FRAMES, 4, generator=g)
        nodes[f"object_{i}"] = ob
    return {name: {k: v.to(dev) for k, v in p.items()} for name, p in nodes.items()}


def quat_to_rotmat(q):   # wxyz, mtgs utils.quat_to_rotmat (no normalisation)
    w, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                        2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(3, 3)


def quat_mult(a, b):     # mtgs utils.quat_mult
    w1, x1, y1, z1 = a.unbind(-1)
    w2, x2, y2, z2 = b.unbind(-1)
    return torch.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                        w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], -1)


def frame_of(t):
    if isinstance(t, torch.Tensor):      # the traversal as a device word (one graph for every traversal): the frame on the device too
        return ((7 * t + 3) % FRAMES).to(torch.int32)
    return (7 * t + 3) % FRAMES


def gaussians_chain(P, c2w, t, n):
    """VanillaGaussianSplattingModel / MultiColorGaussianSplattingModel / RigidSubModel.get_gaussians, operator by operator."""
    out = {"means": [], "scales": [], "quats": [], "opacities": [], "rgbs": []}
    for name, p in P.items():
        if "features_adapters" in p:
            dc, rest = p["features_dc"] + p["features_adapters"][:, t, :], p["features_rest"][:, t, :, :]
        else:
            dc, rest = p["features_dc"], p["features_rest"]
        colors = torch.cat((dc[:, None, :], rest), dim=1)
        means, quats = p["means"], p["quats"] / p["quats"].norm(dim=-1, keepdim=True)
        if "instance_quats" in p:   # get_object_pose (rigid_node.py:139-144) + rigid_node.py:205-216
            f = frame_of(t)
            iq, it = p["instance_quats"][f] / p["instance_quats"][f].norm(dim=-1, keepdim=True), p["instance_trans"][f]
            means = means @ quat_to_rotmat(iq).T + it
            quats = quat_mult(iq[None], quats)
        viewdirs = means.detach() - c2w[..., :3, 3]
        viewdirs = viewdirs / viewdirs.norm(dim=-1, keepdim=True)
        rgbs = torch.clamp(spherical_harmonics(n, viewdirs, colors) + 0.5, 0.0, 1.0)
        out["means"].append(means); out["scales"].append(torch.exp(p["scales"]))
        out["quats"].append(quats)
        out["opacities"].append(torch.sigmoid(p["opacities"]).squeeze(-1)); out["rgbs"].append(rgbs)
    return {k: torch.cat(v, 0) for k, v in out.items()}


def gaussians_fused(P, c2w, t, n, deferred=False):
    from mtgs_amd.nodes import collect_gaussians
    return collect_gaussians([dict(p, traversal_index=t) if "features_adapters" in p else
                              (dict(p, frame_idx=frame_of(t)) if "instance_quats" in p else p) for p in P.values()], c2w, n, 3,
                             deferred_colors=deferred)


def normals_chain(gs, c2w):
    """MTGSSceneModel._get_gaussian_camera_space_normals (mtgs_scene_graph.py:526-545), operator by operator."""
    normals = F.one_hot(torch.argmin(gs["scales"], dim=-1), num_classes=3).float()
    normals = torch.bmm(quat_to_rotmat_n(gs["quats"]), normals[:, :, None]).squeeze(-1)
    normals = F.normalize(normals, dim=1)
    viewdirs = -gs["means"].detach() + c2w.detach()[..., :3, 3]
    viewdirs = viewdirs / viewdirs.norm(dim=-1, keepdim=True)
    neg = (normals * viewdirs).sum(-1) < 0
    normals[neg] = -normals[neg]
    return normals @ c2w.squeeze(0)[:3, :3]


def quat_to_rotmat_n(quat):   # mtgs utils.quat_to_rotmat, batched
    w, x, y, z = torch.unbind(quat, dim=-1)
    mat = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                       2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=-1)
    return mat.reshape(quat.shape[:-1] + (3, 3))


def head_chain(render, alpha, bg, E, normals):
    """mtgs_scene_graph.py:672-690 + LearnableExposureRGBModel.forward (appearance.py:73-87), operator by operator."""
    rgb = torch.clamp(render[..., :3] + (1 - alpha) * bg, 0.0, 1.0).squeeze(0)
    app = torch.clamp(rgb.matmul(E[:3, :3]) + E[None, None, :3, 3], 0, 1) if E is not None else None
    d = render[..., -1:]
    depth = torch.where(alpha > 0, d, d.detach().max()).squeeze(0)
    normal = None
    if normals:
        nm = render[..., 3:6].squeeze(0)
        normal = (nm / nm.norm(dim=-1, keepdim=True) + 1) / 2
    return rgb, app, depth, normal


def ncc_chain(pred_depth, gt_depth, patch_size=32, stride=16, mask=None):
    """calculate_depth_ncc_loss (mtgs/utils/geometric_loss.py:322-348), operator by operator."""
    pred_depth, gt_depth = pred_depth.squeeze(-1), gt_depth.squeeze(-1)
    pad = patch_size // 2
    mask = mask.squeeze(-1).float()
    pp = F.unfold(pred_depth[None, None], kernel_size=patch_size, padding=pad, stride=stride)
    gp = F.unfold(gt_depth[None, None], kernel_size=patch_size, padding=pad, stride=stride)
    mp = F.unfold(mask[None, None], kernel_size=patch_size, padding=pad, stride=stride)
    valid = mp.all(dim=1).squeeze(0)
    pp, gp = pp[:, :, valid], gp[:, :, valid]
    pc, gc = pp - pp.mean(dim=1, keepdim=True), gp - gp.mean(dim=1, keepdim=True)
    ps = torch.sqrt((pc ** 2).mean(dim=1, keepdim=True) + 1e-8)
    gs = torch.sqrt((gc ** 2).mean(dim=1, keepdim=True) + 1e-8)
    return 1 - ((pc / ps) * (gc / gs)).mean(dim=1).mean()


def depth_normals_chain(depth, K):
    """normal_from_depth_image -> @ diag(1,-1,-1) -> (1 + n) / 2 as MTGS runs it (mtgs_scene_graph.py:915-929; the intrinsics
    read to the host, the back-projection through the inverse of an identity, pcd_to_normal's slices, cross, normalize, pad)"""
    K = K.reshape(3, 3)
    fx, fy, cx, cy = K[0, 0].item(), K[1, 1].item(), K[0, 2].item(), K[1, 2].item()
    H, W = depth.shape[0], depth.shape[1]
    d = depth.detach().float().reshape(-1)
    uv = torch.stack(torch.meshgrid(torch.arange(W, device=d.device), torch.arange(H, device=d.device), indexing="xy"), -1)
    uv = (uv + 0.5).view(-1, 2).float()
    P = torch.stack([(uv[:, 0] - cx) * d / fx, (uv[:, 1] - cy) * d / fy, d], dim=-1)
    c2w = torch.eye(4, device=d.device)
    P = (P @ torch.linalg.inv(c2w[:3, :3]) + c2w[:3, 3]).view(H, W, 3)
    a = P[1:-1, 2:] - P[1:-1, :-2]
    b = P[:-2, 1:-1] - P[2:, 1:-1]
    n = F.normalize(torch.cross(a, b, dim=-1), p=2, dim=-1)
    n = F.pad(n.permute(2, 0, 1), (1, 1, 1, 1), mode="constant").permute(1, 2, 0)
    return (1 + n @ torch.diag(n.new_tensor([1, -1, -1]))) / 2


def _win(dev):
    c = torch.arange(11, dtype=torch.float) - 5
    g = torch.exp(-(c ** 2) / (2 * 1.5 ** 2))
    return (g / g.sum())[None, None].repeat(3, 1, 1, 1).to(dev)


def ssim_chain(gt, pred, mask, win):
    X, Y = gt.permute(2, 0, 1)[None], pred.permute(2, 0, 1)[None]
    m = mask.permute(2, 0, 1).unsqueeze(0).expand_as(X)[..., 5:-5, 5:-5]
    f = lambda x: F.conv2d(F.conv2d(x, win.transpose(2, 3), groups=3), win, groups=3)
    mu1, mu2 = f(X), f(Y)
    s1, s2, s12 = f(X * X) - mu1.pow(2), f(Y * Y) - mu2.pow(2), f(X * Y) - mu1 * mu2
    smap = ((2 * mu1 * mu2 + 1e-4) / (mu1.pow(2) + mu2.pow(2) + 1e-4)) * ((2 * s12 + 9e-4) / (s1 + s2 + 9e-4))
    return torch.masked_select(smap, m).mean()


def stats_chain(stats, radii, absgrad, sizes, W, H):
    start = 0
    for (gn, vc, m2), n in zip(stats, sizes):
        grads = (absgrad[0, start:start + n] * absgrad.new_tensor([W, H]) * 0.5).norm(dim=-1)
        r = radii[0, start:start + n]
        vis = r > 0
        vc[vis] += 1; gn[vis] += grads[vis]; m2[vis] = torch.maximum(m2[vis], r[vis].float())
        start += n


VISFIRST = {"on": False, "cs": None, "normals": True, "geometry_rows": False}     # --visfirst: colours of the visible Gaussians only; the last frame's ColorSource
ROWLAZY = {"on": False, "opt": None}     # --row-lazy: exact row-lazy Adam for the colour parameters (needs --visfirst --optimizer fused)
LAZY = {"on": False}                     # --lazy-adam: exact lazy Adam for the per-traversal tensors (needs --visfirst)
ALL_ROWS = {}                            # n -> int32 zeros [n]: a row map that selects every row (catch_up_rows)
DPROWS = {"on": False}                   # --dp-rows: the sparse exchange hands ROWS to the optimizer (no dense gradient on any rank)
REGS = {"on": False}                     # --regularizers: the 2D and sharp-shape terms on the collected scales
GEOM = {"on": False}                     # --device-geometry-losses: the depth normal term and the regularisers on the device
LAST = {"info": {}}                      # the device scalars of the last rasterization's `info` (graph mode: overflow flag and counts)


def at(x, t):
    """x[t] for a host traversal index; for an int32 DEVICE scalar (one captured iteration for every traversal) the row is
    gathered on the device: x is then a stacked tensor [T, ...]."""
    if isinstance(t, torch.Tensor):
        return x.index_select(0, t.view(1))[0]
    return x[t]


def iteration(P, cam, gt, mask, fused, stats, win, W, H, n=3, shipped=None):
    """shipped = None: RGB only (the path + L1 + SSIM).  shipped = dict(exposure=[T,3,4] parameter, bg=[3], gt_depth, gt_normal
    per camera): the option set of config/MTGS.py -- predict_normals (7 blended channels), the exposure model, the lidar
    inverse-depth L1, the depth NCC and the normal L1 (mtgs_scene_graph.py:856-894, 897-936)."""
    vm, K, c2w, t = cam
    vf = fused and VISFIRST["on"]
    gs = gaussians_fused(P, c2w, t, n, deferred=vf) if fused else gaussians_chain(P, c2w, t, n)
    colors = gs["rgbs"]
    VISFIRST["cs"] = gs.get("color_source") if vf else None
    if vf:      # the densification statistics from the compact gradient rows: no dense absgrad / means2d gradient is written
        VISFIRST["cs"].want_grad_rows = True
        VISFIRST["cs"].geometry_rows = VISFIRST["geometry_rows"] and not any("instance_quats" in p for p in P.values())
    if shipped and vf and VISFIRST["normals"]:
        # the camera-space normals of the VISIBLE Gaussians only, inside the rasterization (channels 3..5 after the colours)
        VISFIRST["cs"].camera_normals = c2w.reshape(-1, 4)[:3].to(torch.float32).contiguous()
        colors = None
    elif shipped:
        colors = camera_space_normals(gs["quats"], gs["scales"], gs["means"], c2w, rgbs=colors) if fused else \
            torch.cat([colors, normals_chain(gs, c2w)], dim=-1)       # (visibility first: rgbs = None -> the normals alone)
    if VISFIRST["cs"] is not None and ROWLAZY["on"]:
        VISFIRST["cs"].optimizer = ROWLAZY["opt"]      # the coefficient rows this frame sees are caught up before they are read
        VISFIRST["cs"].touch_first = bool(TOUCH["on"])         # (--touch-first on / auto: train_loop's policy per stretch)
    render, alpha, info = rasterization(gs["means"], gs["quats"], gs["scales"], gs["opacities"], colors, vm, K, W, H,
                                        packed=False, render_mode="RGB+ED", rasterize_mode="antialiased", absgrad=True,
                                        **({"color_source": VISFIRST["cs"]} if vf else {}))
    LAST["info"] = {k: info[k] for k in ("overflow", "n_visible", "n_intersections") if k in info}   # (not `info` itself: its
    #   means2d would keep this iteration's autograd graph -- and its AccumulateGrad nodes -- alive into the next capture)
    if not vf:
        info["means2d"].retain_grad()
    if shipped:
        E, bg = at(shipped["exposure"], t), shipped["bg"]
        rgb, app, depth, normal = output_head(render, alpha, bg, E, depth=True, normal_channel=3) if fused else \
            head_chain(render, alpha, bg, E, True)
        gt_d, gt_n = at(shipped["gt_depth"], t), at(shipped["gt_normal"], t)
        if fused:
            l1 = masked_l1(gt, app, mask)
            loss_d, dmask = inverse_depth_l1(depth, gt_d, mask, 0.1, 80.0, 1e-5)     # :849-858, 875-879: the mask is a by-product
            if GEOM["on"]:      # normal_supervision = 'depth': the target from batch["depth"], the depth-range mask (:912-935)
                loss_n = depth_normal_loss(normal, gt_d, K, mask, 0.1, 50.0, tv=True)
            else:
                loss_n = masked_l1(gt_n, normal, mask) + tv_loss(normal)                 # :931-934
        else:
            dmask = (gt_d > 0.1) & (gt_d < 80) & mask
            inv_gt, inv_pred = 1 / (gt_d + 1e-5), 1 / (depth + 1e-5)
            l1 = torch.abs(gt - app)[mask.squeeze(-1)].mean()
            loss_d = torch.abs(inv_gt - inv_pred)[dmask].mean()
            nmask = mask.squeeze(-1)
            if GEOM["on"]:
                gt_n, nmask = depth_normals_chain(gt_d, K), ((gt_d > 0.1) & (gt_d < 50) & mask).squeeze(-1)
            loss_n = torch.abs(gt_n - normal)[nmask].mean() + \
                torch.mean(torch.abs(normal[:, :-1, :] - normal[:, 1:, :])) + torch.mean(torch.abs(normal[:-1, :, :] - normal[1:, :, :]))
        ssim = masked_ssim(gt, rgb, mask) if fused else ssim_chain(gt, rgb, mask, win)     # use_ssim_on_raw_rgb
        ncc = depth_ncc_loss(depth, gt_d, 32, 16, mask=dmask) if fused else ncc_chain(depth, gt_d, 32, 16, mask=dmask)   # :886-894
        # pixels nothing was splatted on have a 0/0 normal; MTGS adds the term only when it is finite (mtgs_scene_graph.py:939)
        if os.environ.get("MTGS_LOSS_DEBUG"):
            print("terms: l1 %.4f ssim %.4f depth %.4f normal %.4f ncc %.4f | n_vis %d alpha mean %.3f" % (
                float(l1), float(ssim), float(loss_d), float(loss_n), float(ncc), int((info["radii"] > 0).sum()), float(alpha.mean())))
        if fused:      # 0.8 l1 + 0.2 (1 - ssim) + 0.5 depth + 0.1 normal (when finite) + 0.1 ncc, one launch
            loss = combine_losses([l1, ssim, loss_d, loss_n, ncc], [0.8, -0.2, 0.5, 0.1, 0.1], constant=0.2, drop_if_not_finite=(3,))
        else:
            loss_n = torch.where(torch.isfinite(loss_n), loss_n, torch.zeros_like(loss_n))
            loss = 0.8 * l1 + 0.2 * (1 - ssim) + 0.5 * loss_d + 0.1 * loss_n + 0.1 * ncc
    else:
        rgb = torch.clamp(render[0, ..., :3] + (1 - alpha[0]) * 0.0, 0.0, 1.0)          # black background (mtgs_scene_graph.py:672-676)
        l1 = masked_l1(gt, rgb, mask) if fused else torch.abs(gt - rgb)[mask.squeeze(-1)].mean()
        ssim = masked_ssim(gt, rgb, mask) if fused else ssim_chain(gt, rgb, mask, win)
        loss = 0.8 * l1 + 0.2 * (1 - ssim)
    if GEOM["on"] and fused:
        two_d, sharp = scale_regularizers(gs["scales"], two_d=True, max_ratio=10.0)       # (one pass each way for both)
        loss = loss + two_d + 1.0 * sharp
    elif REGS["on"] or GEOM["on"]:
        # the terms of get_loss_dict that reach the Gaussians OUTSIDE the rasterization (mtgs_scene_graph.py:936-939, 969-981:
        # two_d_gaussians and sharp_shape_reg_lambda = 1.0 in config/MTGS.py:114-118): a dense gradient on the collected scales --
        # with --geometry-rows the optimizer steps scales with this .grad PLUS the rasterization's rows
        sc = gs["scales"]
        two_d = torch.min(sc, dim=1, keepdim=True)[0].mean()
        srt, _ = torch.sort(sc, dim=-1, descending=True)
        sharp = (torch.maximum(srt[..., 0] / srt[..., 1], torch.tensor(10.0, device=sc.device)) - 10.0).mean()
        loss = loss + two_d + 1.0 * sharp
    loss.backward()
    if os.environ.get("MTGS_LOSS_DEBUG") and vf and VISFIRST["cs"].rows is not None:
        rows_ = VISFIRST["cs"].rows
        nv_ = int((info["radii"] > 0).sum())
        print("touched: %d of %d visible rows have a non-zero colour gradient" % (int((rows_[:nv_] != 0).any(1).sum()), nv_))
    sizes = [p["means"].shape[0] for p in P.values()]
    with torch.no_grad():
        if vf:
            from mtgs_amd.densify import update_statistics_rows
            cs = VISFIRST["cs"]
            update_statistics_rows([tuple(s) for s in stats], info["radii"], cs.grad_rows, cs.grad_row_ids, W, H,
                                   n_vis_dev=cs.grad_row_count)
        elif fused and len(stats) > 2:   # scene graph with object nodes: one launch for all of them
            update_statistics_all([tuple(s) for s in stats], info["radii"], info["means2d"].absgrad, W, H)
        elif fused:
            start = 0
            for s, n_ in zip(stats, sizes):
                update_statistics(*s, info["radii"], info["means2d"].absgrad, W, H, start=start)
                start += n_
        else:
            stats_chain(stats, info["radii"], info["means2d"].absgrad, sizes, W, H)
    return loss.detach()


def iteration_sparse_dp(P, cam, gt, mask, stats, win, W, H, ex, n=3, shipped=None, opt=None):
    """The fused iteration of one rank under view-parallel data parallelism with the SPARSE gradient exchange
    (mtgs_amd.dist.SparseGradExchange with per-traversal colour routing) instead of a dense all-reduce of every parameter
    gradient: the node kernels hand out the activated geometry and the RAW SH colours of every Gaussian; the exchange
    renders, its backward leaves 64-byte wire rows, finish() returns the SUMS over all ranks of the gradients with respect
    to the activated geometry and to the SH coefficients (every sender's colour factor in its own traversal's slice); the
    geometry sums go back through the node activations (one launch), the coefficient sums ARE the gradients of
    features_dc / features_adapters / features_rest.  Statistics from the compact rows.
    shipped: the option set of config/MTGS.py.  Its three normal channels are a function of THIS rank's camera, so their
    gradient is folded into the quaternion gradient of the wire rows on the sender (mtgs_normals_bwd_rows, via the
    exchange's rows_hook) before the rows are exchanged; the exposure parameters are replicated and all-reduced densely.
    opt (a FusedAdam; --dp-rows, static nodes): ROWS all the way -- finish(rows=True) returns the sums as rows of the union of the
    ranks' visible sets, the geometry rows go through the node activations' VJP per row (mtgs_node_bwd_rows), and every
    parameter takes its gradient through FusedAdam.set_row_gradient: features_adapters / features_rest one slice per traversal
    some rank rendered (row-lazy: the step touches those rows only), features_dc the coefficient-0 sum over all ranks.  No
    dense [N, .] gradient -- in particular no [N, T, K, 3] -- exists on any rank."""
    from mtgs_amd._lib import call, ptr, stream_of
    from mtgs_amd.densify import update_statistics_rows
    from mtgs_amd.nodes import collect_gaussians
    vm, K, c2w, t = cam
    if opt is not None:
        # the node kernels read slice t of the per-traversal tensors for EVERY Gaussian (the sender evaluates SH before it knows
        # what its camera sees): slice t is brought up to date in place first -- the zero-gradient steps its rows missed, bit-
        # identically; the other T - 1 slices stay lazy.  (Next: visibility-first colours under the exchange, as --visfirst.)
        items = []
        for p in P.values():
            if "features_adapters" in p:
                every = ALL_ROWS.get(p["means"].shape[0])
                if every is None or every.device != p["means"].device:
                    every = ALL_ROWS[p["means"].shape[0]] = torch.zeros(p["means"].shape[0], dtype=torch.int32, device=p["means"].device)
                items += [(p["features_adapters"], every, t), (p["features_rest"], every, t)]
        opt.catch_up_rows(items)
    det = lambda p: {k: (v.detach() if k.startswith("features") else v) for k, v in p.items()}   # no colour gradient through the nodes
    gs = collect_gaussians([dict(det(p), traversal_index=t) if "features_adapters" in p else
                            (dict(det(p), frame_idx=frame_of(t)) if "instance_quats" in p else det(p)) for p in P.values()], c2w, n, 3,
                           raw_colors=True)
    leaves = {k: gs[k].detach().requires_grad_(True) for k in ("means", "quats", "scales", "opacities")}
    cam_pos = c2w[..., :3, 3].reshape(3)
    colors = gs["rgbs"].detach()
    ex.rows_hook = None
    if shipped:
        with torch.no_grad():
            colors = camera_space_normals(leaves["quats"], leaves["scales"], leaves["means"], c2w, rgbs=colors)     # [N, 6]
        c2w_f = c2w.reshape(-1)[:12].to(torch.float32).contiguous()

        def hook(G, row_stride, vis_ids, n_vis):      # v_normals = colour channels 3..5 of the compact rows (column 8 + 3)
            call("mtgs_normals_bwd_rows", n_vis, ptr(vis_ids), ptr(leaves["quats"]), ptr(leaves["scales"]), ptr(leaves["means"]),
                 ptr(c2w_f), ptr(G), row_stride, 8 + 3, ptr(ex.rows), stream_of(G))
        ex.rows_hook = hook
    render, alpha, info = ex.rasterization(leaves["means"], leaves["quats"], leaves["scales"], leaves["opacities"], colors,
                                           vm, K, W, H, cam_pos, traversal=t)
    if shipped:
        E, bg = shipped["exposure"][t], shipped["bg"]
        rgb, app, depth, normal = output_head(render, alpha, bg, E, depth=True, normal_channel=3)
        gt_d, gt_n = shipped["gt_depth"][t], shipped["gt_normal"][t]
        loss_d, dmask = inverse_depth_l1(depth, gt_d, mask, 0.1, 80.0, 1e-5)
        loss_n = masked_l1(gt_n, normal, mask) + tv_loss(normal)
        loss = combine_losses([masked_l1(gt, app, mask), masked_ssim(gt, rgb, mask), loss_d, loss_n,
                               depth_ncc_loss(depth, gt_d, 32, 16, mask=dmask)], [0.8, -0.2, 0.5, 0.1, 0.1], constant=0.2,
                              drop_if_not_finite=(3,))
    else:
        rgb = torch.clamp(render[0, ..., :3] + (1 - alpha[0]) * 0.0, 0.0, 1.0)
        loss = 0.8 * masked_l1(gt, rgb, mask) + 0.2 * (1 - masked_ssim(gt, rgb, mask))
    loss.backward()
    with torch.no_grad():
        update_statistics_rows([tuple(s) for s in stats], info["radii"], ex.grad_rows, ex.vis_ids, W, H, n_vis=ex.n_vis)
    if opt is not None:
        if any("instance_quats" in p for p in P.values()):
            raise NotImplementedError("--dp-rows: static nodes (a rigid node reduces a pose gradient over its Gaussians)")
        sizes = [p["means"].shape[0] for p in P.values()]
        starts = [sum(sizes[:i]) for i in range(len(sizes))]
        shared = [(st, st + n_i) for st, n_i, p in zip(starts, sizes, P.values()) if "features_adapters" not in p]
        R = ex.finish(leaves["means"], n, rows=True, all_colour_ranges=shared)
        tab_dev, n_nodes, _keep = gs["node_table"]
        prow = torch.empty((R["geo_rows"].shape[0], 12), dtype=torch.float32, device=R["geo_rows"].device)
        call("mtgs_node_bwd_rows", n_nodes, ptr(tab_dev), ptr(R["geo_ids"]), ptr(R["geo_totals"]), R["geo_rows"].shape[0],
             ptr(R["geo_rows"]), 16, ptr(prow), stream_of(prow))
        for st, n_i, p in zip(starts, sizes, P.values()):
            ro = R["geo_row_of"][st:st + n_i]
            for k, col in (("means", 0), ("scales", 3), ("quats", 6), ("opacities", 10)):
                opt.set_row_gradient(p[k], prow, ro, col)
            opt.set_row_gradient(p["features_dc"], R["geo_rows"], ro, 11)
            if "features_adapters" in p:
                for t_, (rows_t, ro_t) in R["coef"].items():
                    opt.set_row_gradient(p["features_adapters"], rows_t, ro_t[st:st + n_i], 0, slice_index=t_)
                    opt.set_row_gradient(p["features_rest"], rows_t, ro_t[st:st + n_i], 3, slice_index=t_)
            else:
                rows_a, ro_a = R["coef_all"]
                opt.set_row_gradient(p["features_rest"], rows_a, ro_a[st:st + n_i], 3)
        return loss.detach()
    g_means, g_quats, g_scales, g_opac, g_coeffs = ex.finish(leaves["means"], n)          # sums over all ranks
    torch.autograd.backward([gs["means"], gs["quats"], gs["scales"], gs["opacities"]], [g_means, g_quats, g_scales, g_opac])
    start = 0
    for p in P.values():
        n_i = p["means"].shape[0]
        gc = g_coeffs[start:start + n_i]                                                  # [n_i, T, 16, 3]
        p["features_dc"].grad = gc[:, :, 0].sum(1)
        if "features_adapters" in p:       # per-traversal appearance: every traversal's slice from ITS cameras only
            p["features_adapters"].grad = gc[:, :, 0].contiguous()
            p["features_rest"].grad = gc[:, :, 1:].contiguous()
        else:
            p["features_rest"].grad = gc[:, :, 1:].sum(1)
        start += n_i
    return loss.detach()


def iteration_nograd(P, cam, gt, mask, stats, win, W, H, shipped):
    """the loss of `iteration` without backward / statistics (debug aid)"""
    vm, K, c2w, t = cam
    gs = gaussians_fused(P, c2w, t, 3)
    colors = camera_space_normals(gs["quats"], gs["scales"], gs["means"], c2w, rgbs=gs["rgbs"]) if shipped else gs["rgbs"]
    render, alpha, _ = rasterization(gs["means"], gs["quats"], gs["scales"], gs["opacities"], colors, vm, K, W, H, packed=False,
                                     render_mode="RGB+ED", rasterize_mode="antialiased")
    rgb = torch.clamp(render[0, ..., :3], 0.0, 1.0)
    return 0.8 * masked_l1(gt, rgb, mask) + 0.2 * (1 - masked_ssim(gt, rgb, mask))


def refine_device(P, stats, opt_state_of, step, seed, growth=0.02, cfg=None, lazy_opt=None, scene=False):
    """Densification of every static node with mtgs_amd.densify.refine_gaussians (csrc/refine.hip): the reference's rules
    (vanilla_gaussian_splatting.py:476-699) on the device, Adam moments following their rows, samples from a generator keyed
    by (seed, step, Gaussian index) -- identical on every rank of a data-parallel run.  The gradient threshold is set per
    node to the (1 - growth) quantile of the average screen-space gradient so that the synthetic scene refines at a steady
    rate (the statistics are all-reduced before, so every rank computes the same threshold).
    cfg (mtgs_amd.densify.RefineConfig): FIXED thresholds instead -- the reference's control values (config/MTGS.py:59-71),
    with the screen-space gradient threshold scaled ONCE for the synthetic scene (--converge): what refines is then decided
    by the training state, and fewer Gaussians qualify as the model converges; the opacity reset of refinement_after
    (:555-572) runs on the reference's schedule.
    lazy_opt (a FusedAdam with row-lazy parameters): NO flush before the rows move -- the `last` stamps travel with their rows
    like the moments do (refine_gaussians(extras=...)), and only the Gaussians that get children or a duplicate, whose current
    values the new rows copy, are caught up first (before_rows -> FusedAdam.catch_up_rows).  swap[...] then carries
    (last, hist) for the next optimizer's set_row_lazy.
    scene (--refine-scene): EVERY node, the rigid object nodes included, in one pass of mtgs_amd.densify.refine_scene -- one host
    synchronisation and a fixed number of launches whatever the number of nodes; the per-frame pose parameters of an object node
    (instance_quats / instance_trans) are no per-Gaussian tensors and stay as they are.
    Returns (added, culled, {old parameter id: (old, new parameter, new moments | None, (last, hist) | None)})."""
    from dataclasses import replace
    from mtgs_amd.densify import NodeRefine, RefineConfig, refine_gaussians, refine_scene, reset_opacities
    added = culled = 0
    swap = {}
    fixed = cfg
    jobs = []
    for (name, p), st in zip(list(P.items()), stats):
        if "instance_quats" in p:
            if not scene:
                continue
            p = {k: v for k, v in p.items() if not k.startswith("instance_")}       # (the per-Gaussian tensors of a rigid node)
        if fixed is None:
            avg = st[0] / st[1]
            thr = float(torch.quantile(avg[:: max(1, avg.numel() // 1_000_000)], 1.0 - growth))
            cfg = RefineConfig(densify_grad_thresh=max(thr, 1e-12), densify_size_thresh=0.12, cull_alpha_thresh=0.02, refine_every=20,
                               reset_alpha_every=10 ** 6, split_screen_size=1e9, cull_screen_size=1e9, clone_sample_means=False)
        moments = {k: (opt_state_of(v)["exp_avg"], opt_state_of(v)["exp_avg_sq"]) for k, v in p.items()
                   if opt_state_of(v) and "exp_avg" in opt_state_of(v)}
        n_old = p["means"].shape[0]
        lazy = {k: lazy_opt.row_lazy_state(v) for k, v in p.items()
                if lazy_opt is not None and hasattr(lazy_opt, "row_lazy_state") and lazy_opt.row_lazy_state(v) is not None}
        extras = {"last:" + k: stt[0].view(n_old, -1) for k, stt in lazy.items()}

        def before_rows(parents, p=p, lazy=lazy, n_old=n_old):
            m = torch.where(parents, 0, -1).to(torch.int32).contiguous()
            items = []
            for k, stt in lazy.items():
                T_k = stt[0].numel() // max(n_old, 1)
                items += [(p[k], m, (t_ if T_k > 1 else None)) for t_ in range(T_k)]
            lazy_opt.catch_up_rows(items)
        jobs.append((name, p, st, cfg, moments, extras, lazy, before_rows))

    if scene:
        # the caller gates the step (densify_from); the reset follows the reference's schedule only with fixed thresholds, as below
        nodes = [NodeRefine({k: v.detach() for k, v in p.items()}, tuple(st),
                            replace(cfg, densify_from_iter=0, stop_split_at=max(cfg.stop_split_at, step + 1),
                                    reset_alpha_every=cfg.reset_alpha_every if fixed is not None else 10 ** 9),
                            seed, moments=moments or None, extras=extras or None)
                 for _, p, st, cfg, moments, extras, _, _ in jobs]
        hooks = [(j[7] if j[6] else None) for j in jobs]

        def before_all(masks):
            for hook, m in zip(hooks, masks):
                if hook is not None and m is not None:
                    hook(m)
        results = refine_scene(nodes, step, before_rows=before_all if any(hooks) else None)
    else:
        results = []
        for name, p, st, cfg, moments, extras, lazy, before_rows in jobs:
            new, new_m, info = refine_gaussians({k: v.detach() for k, v in p.items()}, tuple(st), cfg, step, seed,
                                                moments=moments or None, extras=extras or None,
                                                before_rows=before_rows if lazy else None)
            if fixed is not None and step % (cfg.reset_alpha_every * cfg.refine_every) == cfg.refine_every:
                reset_opacities(new["opacities"], cfg, new_m.get("opacities") if new_m else None)
            results.append((new, new_m, info))
    for (name, p, st, cfg, moments, extras, lazy, _), res in zip(jobs, results):
        if res is None:                              # (an empty node)
            continue
        new, new_m, info = res
        n_new = info["n_after"]
        for k, v in p.items():
            q = new[k].requires_grad_(True)
            carry = (info["extras"]["last:" + k].reshape(-1).contiguous(), lazy[k][1]) if k in lazy else None
            swap[id(v)] = (v, q, new_m.get(k) if new_m else None, carry)
            new[k] = q
        P[name] = dict(new, **{k: v for k, v in P[name].items() if k.startswith("instance_")})
        added += info["n_children"] + info["n_dups"]
        culled += info["n_before"] - info["n_old_kept"]
        dev = new["means"].device
        st[0], st[1], st[2] = torch.zeros(n_new, device=dev), torch.ones(n_new, device=dev), torch.zeros(n_new, device=dev)
    return added, culled, swap


LR_SETS = {
    # the harness's own (rounds 1-3): one rate per kind of parameter
    "harness": {"features_dc": 2e-2, "features_rest": 2e-2, "features_adapters": 2e-2, "opacities": 5e-2, "means": 1e-4, "scales": 1e-4,
                "quats": 1e-4, "instance_quats": 1e-4, "instance_trans": 1e-4, "exposure": 1e-4},
    # the groups of config/MTGS.py:121-181 (means 8e-4 -> 8e-6 exponentially, features_dc 2.5e-3, features_rest 2.5e-3 / 20,
    # opacities 5e-2, scales 5e-3, quats 1e-3), scaled ONCE for a run of a few hundred steps instead of 30 000: the colour rates
    # x 4 (the synthetic colours start 0.3 off), everything else as shipped
    "reference": {"features_dc": 1e-2, "features_rest": 1e-2 / 20, "features_adapters": 1e-2, "opacities": 5e-2, "means": 8e-4,
                  "scales": 5e-3, "quats": 1e-3, "instance_quats": 1e-3, "instance_trans": 8e-4, "exposure": 1e-3},
}
LR = {"set": "harness"}
REFINE_SCENE = {"on": False}      # --refine-scene: refine_device through mtgs_amd.densify.refine_scene, object nodes included


def make_optimizer(kind, P, shipped=None, capturable=False):
    """One optimizer over every parameter group.  kind = "fused": mtgs_amd.optim.FusedAdam (one launch per step, csrc/adam.hip);
    "torch": torch.optim.Adam(foreach=True), what nerfstudio builds per group (custom_trainer.py:115-136).  One group per kind of
    parameter, as the reference's `{node}.{type}.{param}` groups (learning rates: LR_SETS)."""
    rates = LR_SETS[LR["set"]]
    by_kind = {}
    for p in P.values():
        for k, v in p.items():
            by_kind.setdefault(k, []).append(v)
    if shipped:
        by_kind["exposure"] = [shipped["exposure"]]
    if LR["set"] == "harness":      # (the original three groups, in the original parameter order: same training as rounds 1-3)
        extra = [shipped["exposure"]] if shipped else []
        geo = [p[k] for p in P.values() for k in p if not k.startswith("features") and k != "opacities"]
        groups = [{"params": [p[k] for p in P.values() for k in p if k.startswith("features")], "lr": 2e-2},
                  {"params": [p["opacities"] for p in P.values()], "lr": 5e-2},      # config/MTGS.py: opacities 0.05
                  {"params": geo + extra, "lr": 1e-4}]
    else:
        groups = [{"params": v, "lr": rates[k], "name": k} for k, v in by_kind.items()]
    if kind == "fused":
        from mtgs_amd.optim import FusedAdam
        opt = FusedAdam(groups, eps=1e-15)
        if LAZY["on"]:      # exact lazy Adam: a step touches the rendered traversal's slice of the per-traversal tensors only
            for p in P.values():
                for k in ("features_rest", "features_adapters"):
                    if k in p and p[k].dim() == (4 if k == "features_rest" else 3) and "features_adapters" in p:
                        opt.set_lazy_slices(p[k])
        return opt
    return torch.optim.Adam(groups, eps=1e-15, foreach=True, capturable=capturable)


def enable_dp_rows(opt, P, carry=None):
    """--dp-rows: the per-traversal colour tensors are row-lazy (a step touches the rows of the slices some rank rendered; the
    other slices and rows decay lazily, bit-identically to stepping them).  Call on a new optimizer after its state is in place."""
    if not DPROWS["on"]:
        return opt
    kw = lambda q: dict(zip(("last", "hist"), carry[id(q)])) if (carry and carry.get(id(q))) else {}
    for p in P.values():
        if "features_adapters" in p:
            a, r = p["features_adapters"], p["features_rest"]
            opt.set_row_lazy(a, traversals=a.shape[1], **kw(a))
            opt.set_row_lazy(r, traversals=r.shape[1], **kw(r))
    return opt


def enable_row_lazy(opt, P, carry=None):
    """--row-lazy: the colour parameters (read for the visible Gaussians only under --visfirst) are stepped for the visible
    rows of the rendered traversal alone.  Call on a new optimizer AFTER its state is in place (refinement); carry {id(parameter):
    (last, hist)}: the stamps a refinement moved with their rows and the history of the previous optimizer (no flush)."""
    if not ROWLAZY["on"] or not hasattr(opt, "set_row_lazy"):
        return opt
    kw = lambda q: dict(zip(("last", "hist"), carry[id(q)])) if (carry and carry.get(id(q))) else {}
    for p in P.values():
        opt.set_row_lazy(p["features_dc"], **kw(p["features_dc"]))
        if "features_adapters" in p:
            a = p["features_adapters"]
            opt.set_row_lazy(a, traversals=a.shape[1] if a.dim() == 3 else None, **kw(a))
        r = p["features_rest"]
        if r.shape[-2] > 0:
            opt.set_row_lazy(r, traversals=r.shape[1] if r.dim() == 4 else None, **kw(r))
    ROWLAZY["opt"] = opt
    return opt


TOUCH = {"on": False, "mode": "off"}   # ColorSource.touch_first for the frames to come (--touch-first; auto: decided per stretch)
ANY = "any traversal"      # key of the one graph that serves every traversal (train_loop(one_graph=True))


def train_loop(P, cams, targets, mask, win, W, H, steps, refine_every, shipped=None, world=1, rank=0, accumulate=1, seed=7,
               log=print, sparse=False, optimizer="fused", graph=False, refine_cfg=None, poll_every=16, means_lr_final=None,
               timing_from=None, densify_from=0, steady=None, first_cap_scale=1.0, one_graph=False):
    """Adam on the fused iteration (MTGSSceneModel.get_outputs -> get_loss_dict -> backward -> optimizers.step ->
    update_submodel_statistics / after_train / refinement_after every refine_every steps: mtgs_scene_graph.py:547-708, 806-987,
    1157-1183; vanilla_gaussian_splatting.py:448-577).  world > 1: view-parallel data parallelism (one process per rank, camera
    (step * world + rank) % T, ONE dense all-reduce of every gradient per step, statistics all-reduced before each
    refinement, refinement identical on every rank).  accumulate = K in ONE process: the K cameras of a step rendered one
    after the other with the gradients accumulated -- the single-process statement of the same training step
    (parity for C4 is defined against it).

    No step waits for the host: the losses go to a device-side history that is read at the refinements and at the end.

    graph = True (single process, one camera per step): the loop TRAINS THROUGH HIP GRAPHS.  Between two refinements N is
    fixed; the first time a traversal's camera comes up in such a stretch its iteration runs once eagerly under
    mtgs_amd.graph_mode (that IS the training step) and is captured right after (torch.cuda.graph: nothing executes), every
    later step of that traversal is FusedAdam.advance() + one graph launch.  Capacities: the first stretch renders every
    traversal once without fixed capacities (the size plan learns n_vis / M of this scene), later stretches scale the largest
    counts their predecessor saw on the device by the growth of N.  The graphs OR the frames' `info["overflow"]` flags into one
    device word that the host polls every `poll_every` steps through a pinned copy and an event it only QUERIES; on overflow
    the graphs are dropped, every traversal renders one frame the ordinary way (exact sizes, the size plan updated) and is
    captured again with larger capacities.  A refinement ends the stretch: flush the row-lazy state, refine on the device (the
    one host synchronisation: the new N), new optimizer with the moved moments, new graphs.
    one_graph = True (with graph; visibility-first colours and row-lazy colour parameters, static nodes): the traversal is an
    int32 DEVICE scalar -- the camera, the targets and the exposure row are gathered from stacked tensors inside the graph, the
    optimizer's peek / step read the slice from that word (mtgs_adam_group.sub_index_dev), the rigid nodes' frame of the step is a
    device word too (mtgs_node_desc.frame_dev) -- so a stretch captures ONE graph instead of one per traversal (MTGS trains with 8
    traversals: 7 captures fewer behind every refinement).
    refine_cfg: RefineConfig with fixed thresholds (refine_device), None = the per-refinement quantile of rounds 1-3.
    densify_from: GaussianSplattingControlConfig.densify_from_iter -- no refinement (and no statistics reset) up to that step.
    means_lr_final: the reference's exponential decay of the position learning rate (config/MTGS.py:124-129) over `steps`.
    Returns (loss curve, N after every refinement)."""
    import mtgs_amd
    from mtgs_amd import dist as mdist
    from mtgs_amd import wrapper
    T = len(cams)
    dev = next(iter(P.values()))["means"].device
    if graph and (world > 1 or accumulate > 1 or optimizer != "fused" or LAZY["on"]):
        raise ValueError("graph training: one process, one camera per step, the fused optimizer, no --lazy-adam")

    if one_graph:
        if not (graph and VISFIRST["on"] and ROWLAZY["on"]):
            raise ValueError("one_graph: graph training with --visfirst --row-lazy")
        t_dev = torch.zeros((), dtype=torch.int32, device=dev)
        cam_all = [torch.stack([cm[j] for cm in cams]).contiguous() for j in range(3)]          # viewmats, Ks, camera_to_worlds
        gt_all = torch.stack(list(targets)).contiguous()
        shipped_all = None if shipped is None else dict(shipped, gt_depth=torch.stack(list(shipped["gt_depth"])).contiguous(),
                                                        gt_normal=torch.stack(list(shipped["gt_normal"])).contiguous())

    def make_opt():
        return make_optimizer(optimizer, P, shipped)

    def touch_policy(after_reset=False):
        """ColorSource.touch_first for the next stretch: one more pass of the compositing decisions (about one forward) finds the
        Gaussians a frame composites FROM, and the optimizer's peek / step, the SH evaluation and the normals leave the others
        alone -- worth it when most visible Gaussians are hidden (an opaque scene: 2-9 % carry a gradient), not while the model is
        translucent (right after an opacity reset; a perturbed start).  Measured on the last frame's gradient rows."""
        cs = VISFIRST["cs"]
        if not (ROWLAZY["on"] and cs is not None and cs.rows is not None) or TOUCH["mode"] != "auto":
            return
        n_vis = int((cs.row_of >= 0).sum())
        frac = float((cs.rows[:n_vis, 0:3] != 0).any(1).sum()) / max(n_vis, 1)
        TOUCH["on"] = (frac < 0.35) and not after_reset
        log(f"touch-first {'on' if TOUCH['on'] else 'off'}: {100 * frac:.1f} % of the {n_vis} visible Gaussians carry a gradient"
            + (" (opacity reset: off for this stretch)" if after_reset else ""))

    opt = enable_dp_rows(enable_row_lazy(make_opt(), P), P)
    mk = lambda: [[torch.zeros(p["means"].shape[0], device=p["means"].device), torch.ones(p["means"].shape[0], device=p["means"].device),
                   torch.zeros(p["means"].shape[0], device=p["means"].device)] for p in P.values()]
    stats = mk()
    sizes = []
    group = max(world, accumulate)
    sparse = sparse and world > 1
    mk_ex = lambda: mdist.SparseGradExchange(sum(p["means"].shape[0] for p in P.values()), 16, next(iter(P.values()))["means"].device,
                                             traversals=T) if sparse else None
    ex = mk_ex()
    loss_hist = torch.zeros(max(steps, 1), dtype=torch.float32, device=dev)     # (no per-step host read of the loss)

    def set_lrs(i):
        if means_lr_final is None:
            return
        for g in opt.param_groups:
            if g.get("name") == "means":     # ExponentialDecaySchedulerConfig(lr_final, max_steps): lr0 * (lr_final / lr0) ** (i / steps)
                lr0 = LR_SETS[LR["set"]]["means"]
                g["lr"] = lr0 * (means_lr_final / lr0) ** (i / max(steps, 1))

    # ---- graph training: the capture / replay / overflow / re-capture manager is mtgs_amd.graphs.GraphedIteration (one stretch
    # between two refinements per set of graphs, one memory pool for the run); this loop supplies the iteration body and the hooks
    n_active = [0]       # tensors the optimizer steps (known once an optimizer has run a step: capture without warm-up needs it)
    GI = None
    debug = bool(os.environ.get("MTGS_TRAIN_DEBUG"))
    phase_ms, tick_t = {}, [time.perf_counter()]

    def tick(name):      # MTGS_TRAIN_DEBUG=1: where the wall time goes (synchronising: not for timing runs)
        if debug:
            torch.cuda.synchronize()
            now = time.perf_counter()
            phase_ms[name] = phase_ms.get(name, 0.0) + (now - tick_t[0]) * 1e3
            tick_t[0] = now

    def body(c):
        opt.zero_grad(set_to_none=True)
        if c is ANY:       # the traversal of the device word: everything that depends on it is gathered on the device
            cam = tuple(at(x, t_dev) for x in cam_all) + (t_dev,)
            loss = iteration(P, cam, at(gt_all, t_dev), mask, True, stats, win, W, H, shipped=shipped_all)
        else:
            loss = iteration(P, cams[c], targets[c], mask, True, stats, win, W, H, shipped=shipped)
        if VISFIRST["cs"] is not None:
            VISFIRST["cs"].apply_to(opt)
        opt.step()
        return loss

    if graph:
        from mtgs_amd.graphs import GraphedIteration
        GI = GraphedIteration(lambda c: (body(c), LAST["info"]), n_keys=T,
                              size_key=lambda: (1, sum(p["means"].shape[0] for p in P.values()), W, H), device=dev,
                              before_replay=lambda: opt.advance(),      # this step's {lr / bc1, sqrt(bc2), t}: one small copy in front of the launch
                              on_capacities=lambda: touch_policy(), can_skip_warmup=lambda: n_active[0] > 0, poll_every=poll_every,
                              first_cap_scale=first_cap_scale, tight_lists=None, log=log, tick=tick,
                              snapshot_host_state=(lambda: opt.host_state()) if hasattr(opt, "host_state") else None,
                              restore_host_state=(lambda s: opt.set_host_state(s)) if hasattr(opt, "host_state") else None)

    def graph_step(c):
        key = c
        if one_graph and GI.caps is not None:      # one graph for every traversal: the traversal goes in through the device word
            t_dev.fill_(c)
            key = ANY
        warm = GI.counts["warmups"]
        loss = GI.step(key)
        if GI.counts["warmups"] > warm:
            n_active[0] = len(opt._active)
        return loss

    t_start = None
    i_start = 0
    steady_ev = []           # GPU time per step over a window without refinements (steady = (first step, last step))
    # (the clock starts behind the one-time start-up: the first few eager steps -- allocator, size plan, lazy initialisation --
    #  and, when training through graphs, the first capture of every traversal; every later re-capture and every refinement is
    #  inside the measured span)
    t_from = min(2 * T if graph else 3, steps - 1) if timing_from is None else min(timing_from, steps - 1)
    for i in range(steps):
        if i == t_from:       # wall clock per step after the first few (allocator, size plan, lazy init)
            torch.cuda.synchronize()
            t_start, i_start = time.perf_counter(), i
        set_lrs(i)
        if steady and i in steady:
            steady_ev.append(torch.cuda.Event(enable_timing=True))
            steady_ev[-1].record()
        if graph:
            loss_hist[i].copy_(graph_step(i % T))
            GI.poll(i)
        else:
            if i == T and world == 1 and accumulate == 1:
                touch_policy()
            opt.zero_grad(set_to_none=True)
            losses = []
            for a in range(accumulate):
                c = (i * group + (rank if world > 1 else a)) % T
                if sparse:
                    losses.append(iteration_sparse_dp(P, cams[c], targets[c], mask, stats, win, W, H, ex, shipped=shipped,
                                                      opt=opt if DPROWS["on"] else None))
                else:
                    if LAZY["on"]:
                        opt.prepare(c)
                    losses.append(iteration(P, cams[c], targets[c], mask, True, stats, win, W, H, shipped=shipped))
            loss = torch.stack(losses).sum()
            params = [q for g in opt.param_groups for q in g["params"]]
            if world > 1:
                if not sparse:
                    mdist.all_reduce_grads(params)
                elif shipped:                       # the replicated non-Gaussian parameters (exposure): a few floats
                    mdist.all_reduce_grads([shipped["exposure"]])
                torch.distributed.all_reduce(loss)
            loss_hist[i].copy_(loss / group)
            if VISFIRST["cs"] is not None and accumulate == 1 and world == 1:
                VISFIRST["cs"].apply_to(opt)
            opt.step()
        if refine_every and (i + 1) % refine_every == 0 and densify_from < i + 1 < steps:     # (refinement_after: step <= densify_from_iter returns)
            tick("other")
            if world > 1:   # every rank must see the same statistics (vis_counts starts at ONE: counted once)
                mdist.all_reduce_stats([t for s in stats for t in s[:2]], [s[2] for s in stats],
                                       sum_init=[v for _ in stats for v in (0.0, 1.0)])
            before = sum(p["means"].shape[0] for p in P.values())
            if LAZY["on"]:
                opt.flush()                   # (slice-lazy tensors: every slice up to date before rows move)
            # row-lazy tensors are NOT flushed: their `last` stamps move with the rows, only the parents of new rows are caught up
            params = [q for g in opt.param_groups for q in g["params"]]
            state = {id(q): opt.state.get(q) for q in params}
            tick("flush")
            added, culled, swap = refine_device(P, stats, lambda q: state.get(id(q)), i + 1, seed, cfg=refine_cfg,
                                                lazy_opt=opt if (ROWLAZY["on"] or DPROWS["on"]) else None, scene=REFINE_SCENE["on"])
            tick("refine_device")
            old_opt, opt = opt, make_opt()
            carry = {}
            for old_id, (old, new_p, mom, lz) in swap.items():
                st_o = state.get(old_id)
                if st_o and mom is not None:
                    opt.state[new_p] = {"step": st_o["step"], "exp_avg": mom[0], "exp_avg_sq": mom[1]}
                if lz is not None and st_o:
                    carry[id(new_p)] = lz
            for grp in opt.param_groups:      # untouched parameters (object nodes, exposure) keep their whole state
                for q in grp["params"]:
                    if q not in opt.state and state.get(id(q)):
                        opt.state[q] = state[id(q)]
            enable_row_lazy(opt, P, carry)
            enable_dp_rows(opt, P, carry)
            if hasattr(opt, "inherit_layout"):
                opt.inherit_layout(old_opt)
            del old_opt
            sizes.append(sum(p["means"].shape[0] for p in P.values()))
            if world > 1 and os.environ.get("MTGS_DIST_BACKEND") == "gloo":
                torch.cuda.empty_cache()      # (the ranks of a gloo run SHARE one GPU: hand the old tensors' blocks back to the other ranks)
            ex = mk_ex()                      # N changed: new send buffers and visibility maps
            touch_policy(after_reset=refine_cfg is not None and
                         (i + 1) % (refine_cfg.reset_alpha_every * refine_cfg.refine_every) == refine_cfg.refine_every)
            if graph:                         # new parameters: new graphs, capacities scaled by the growth of N
                GI.after_refinement(before, sizes[-1])
            log(f"step {i + 1}: refine {before} -> {sizes[-1]} Gaussians (+{added} -{culled})")
            tick("new optimizer")
    if debug:
        tick("other")
        log("debug phases ms:", json.dumps({k: round(v, 1) for k, v in phase_ms.items()}))
    if LAZY["on"] or ROWLAZY["on"] or DPROWS["on"]:
        opt.flush()
    torch.cuda.synchronize()
    if t_start is not None and steps > i_start:
        ms = (time.perf_counter() - t_start) / (steps - i_start) * 1e3
        ph = {k: round(v, 3) for k, v in ex.phases_ms().items()} if ex is not None else {}
        log(f"timing: {ms:.2f} ms per step (wall, refinements{' and graph captures' if graph else ''} included) world {world} "
            f"accumulate {accumulate} exchange {'sparse' if sparse else ('dense' if world > 1 else 'none')} optimizer {optimizer} "
            f"phases_ms {json.dumps(ph)}" + (f" graph {json.dumps(GI.counts)}" if graph else ""))
    if len(steady_ev) == 2:
        log(f"steady: {steady_ev[0].elapsed_time(steady_ev[1]) / (steady[1] - steady[0]):.3f} ms per step between steps {steady[0]} and {steady[1]} (GPU events)")
    if graph and GI.overflowed():
        log("note: a graph frame overflowed its capacities after the last poll")
    if graph:
        GI.close()
    return loss_hist[:steps].tolist(), sizes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-background", type=int, default=1_600_000)
    ap.add_argument("--n-road", type=int, default=400_000)
    ap.add_argument("--traversals", type=int, default=3)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--height", type=int, default=540)
    ap.add_argument("--objects", type=int, default=0, help="rigid object nodes (per-frame pose parameters) in the scene graph")
    ap.add_argument("--object-size", type=int, default=3000)
    ap.add_argument("--shipped", action="store_true", help="the option set of config/MTGS.py: predict_normals (7 blended channels), "
                    "exposure model, inverse-depth and normal losses")
    ap.add_argument("--steps", type=int, default=0)
    ap.add_argument("--refine-every", type=int, default=0, help="with --steps: densify (duplicate / split / cull) every so many steps")
    ap.add_argument("--refine-scene", action="store_true", help="with --refine-every: refine EVERY node, the object nodes included, in one "
                    "pass of mtgs_amd.densify.refine_scene instead of one refine_gaussians call per static node")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", choices=["both", "fused", "chain"], default="both", help="profiling aid: time one variant only")
    ap.add_argument("--dp", action="store_true", help="with --steps: view-parallel data parallelism under torch.distributed.run "
                    "(one camera per rank and step, dense gradient all-reduce, rank-identical refinement)")
    ap.add_argument("--dp-exchange", choices=["dense", "sparse"], default="dense", help="with --dp: dense all-reduce of every "
                    "parameter gradient, or the sparse factored exchange of mtgs_amd.dist")
    ap.add_argument("--accumulate", type=int, default=1, help="with --steps: cameras per step in ONE process (gradient accumulation)")
    ap.add_argument("--optimizer", choices=["none", "torch", "fused"], default=None, help="the optimizer step: torch.optim.Adam(foreach) "
                    "or mtgs_amd.optim.FusedAdam (one launch).  Timing runs (--only / --graph / default) leave it out unless "
                    "given; --steps trains with the fused one unless told otherwise")
    ap.add_argument("--visfirst", action="store_true", help="visibility first: node kernels geometry-only, SH + clamp for the VISIBLE "
                    "Gaussians inside the rasterizer's front end, coefficient gradients as compact rows into the fused Adam")
    ap.add_argument("--lazy-adam", action="store_true", help="with --visfirst --optimizer fused: the per-traversal tensors' other "
                    "slices are left untouched by a step and caught up (bit-identically) before their traversal is rendered again")
    ap.add_argument("--dense-normals", action="store_true", help="with --visfirst --shipped: the camera-space normals of EVERY Gaussian "
                    "as extra colour channels (mtgs_amd.nodes.camera_space_normals) instead of the visible ones inside the rasterization")
    ap.add_argument("--geometry-rows", action="store_true", help="with --visfirst --optimizer fused (static nodes): the geometry gradients "
                    "stay rows of the visible Gaussians all the way to the optimizer (mtgs_node_bwd_rows): no dense expansion, no dense "
                    "node backward")
    ap.add_argument("--row-lazy", action="store_true", help="with --visfirst --optimizer fused: exact row-lazy Adam -- the colour "
                    "parameters are stepped for the VISIBLE rows of the rendered traversal only and a row is caught up (bit-identically) "
                    "right before the forward reads it (mtgs_amd.optim.FusedAdam.set_row_lazy)")
    ap.add_argument("--graph", action="store_true", help="fused iteration captured as ONE HIP graph per traversal "
                    "(torch.cuda.graph + mtgs_amd.graph_mode): wall time per iteration vs its GPU time")
    ap.add_argument("--train-graph", action="store_true", help="with --steps: TRAIN through HIP graphs (one per traversal, re-captured "
                    "after every refinement, overflow polled without a host wait; train_loop(graph=True))")
    ap.add_argument("--touch-first", choices=("off", "on", "auto"), default="off", help="with --visfirst --row-lazy: ColorSource.touch_first "
                    "(one more pass of the compositing decisions flags the Gaussians a frame composites from; peek / SH / normals for those "
                    "alone); auto: per stretch, on while fewer than 35 %% of the visible Gaussians carry a gradient and no opacity reset "
                    "has just happened")
    ap.add_argument("--one-graph", action="store_true", help="with --train-graph --visfirst --row-lazy: the traversal is a DEVICE word, "
                    "one graph per stretch serves every traversal (train_loop(one_graph=True))")
    ap.add_argument("--converge", action="store_true", help="with --steps: the training problem with something to learn and the "
                    "reference's refinement rules -- the model starts from a SUBSET of the true Gaussians with perturbed positions, "
                    "shapes, opacities and colours; fixed thresholds of config/MTGS.py:59-71 (screen-space gradient threshold scaled once, "
                    "--grad-thresh), clone_sample_means, opacity culling at 0.005; the reference's learning-rate groups (LR_SETS)")
    ap.add_argument("--grad-thresh", type=float, default=None, help="with --converge: densify_grad_thresh (the reference's 0.001 is for "
                    "nuPlan images; default: scaled once for the synthetic scene)")
    ap.add_argument("--drop", type=float, default=0.1, help="with --converge: fraction of the true Gaussians the model starts without")
    ap.add_argument("--poll-every", type=int, default=16)
    ap.add_argument("--dp-rows", action="store_true", help="with --dp --dp-exchange sparse --optimizer fused: the exchange's sums stay "
                    "ROWS of the union of the ranks' visible sets all the way into the optimizer (SparseGradExchange.finish(rows=True), "
                    "mtgs_node_bwd_rows, FusedAdam.set_row_gradient with one slice per rendered traversal; the colour tensors row-lazy)")
    ap.add_argument("--regularizers", action="store_true", help="add MTGS's '2D reg' and 'Sharp Shape Reg' terms on the collected scales "
                    "(mtgs_scene_graph.py:936-939, 969-981): loss terms that reach the Gaussians outside the rasterization")
    ap.add_argument("--device-geometry-losses", action="store_true", help="with --shipped: MTGS's depth-supervised normal term "
                    "(the target from each camera's gt_depth as batch['depth'], the depth-range mask) and the '2D reg' / 'Sharp Shape "
                    "Reg' terms, on the device (mtgs_amd.loss.depth_normal_loss, scale_regularizers) in the fused iteration")
    ap.add_argument("--first-cap-scale", type=float, default=1.0, help="with --train-graph (tests): scale of the first graphs' capacities; "
                    "< 1 makes their frames overflow, which the loop must notice and repair")
    ap.add_argument("--steady", type=int, nargs=2, default=None, help="with --steps: also report the time per step between these two steps")
    ap.add_argument("--size-thresh", type=float, default=0.2, help="with --converge: RefineConfig.densify_size_thresh (config/MTGS.py:65)")
    ap.add_argument("--cull-alpha", type=float, default=0.005, help="with --converge: RefineConfig.cull_alpha_thresh (config/MTGS.py:63)")
    ap.add_argument("--clear-radius", type=float, default=None, help="no Gaussians within this many metres of the cameras (ground plane); "
                    "default 6 with --converge (3 sigma of the largest Gaussian then stays below split_screen_size = 100 px), else 0")
    ap.add_argument("--split-screen-size", type=float, default=100.0, help="with --converge: RefineConfig.split_screen_size (config/MTGS.py:70)")
    ap.add_argument("--densify-from", type=int, default=None, help="densify_from_iter (config/MTGS.py:57: 5 x refine_every, the default "
                    "with --converge; 0 otherwise)")
    ap.add_argument("--trace-refinements", action="store_true", help="print the loss around every refinement")
    args = ap.parse_args()
    REFINE_SCENE["on"] = args.refine_scene
    if args.visfirst and (args.accumulate > 1 or args.dp):
        raise SystemExit("--visfirst hands the gradients to the optimizer as rows of ONE frame: not with --accumulate > 1 or --dp "
                         "(the sparse exchange has its own row path)")
    if args.train_graph and not args.steps:
        raise SystemExit("--train-graph needs --steps")
    VISFIRST["on"] = bool(args.visfirst)
    TOUCH["mode"], TOUCH["on"] = args.touch_first, args.touch_first == "on"
    REGS["on"] = bool(args.regularizers)
    GEOM["on"] = bool(args.device_geometry_losses)
    if GEOM["on"] and not args.shipped:
        raise SystemExit("--device-geometry-losses needs --shipped (the normal term of the shipped option set)")
    if GEOM["on"] and args.dp and args.dp_exchange == "sparse":
        raise SystemExit("--device-geometry-losses: not with --dp-exchange sparse (its iteration keeps the precomputed target)")
    DPROWS["on"] = bool(args.dp_rows)
    if args.dp_rows and not (args.dp and args.dp_exchange == "sparse" and args.optimizer in (None, "fused")):
        raise SystemExit("--dp-rows needs --dp --dp-exchange sparse and the fused optimizer")
    VISFIRST["normals"] = not args.dense_normals
    VISFIRST["geometry_rows"] = bool(args.geometry_rows)
    if args.geometry_rows and not (args.visfirst and args.optimizer in (None, "fused")):
        raise SystemExit("--geometry-rows needs --visfirst and the fused optimizer")
    LAZY["on"] = bool(args.lazy_adam)
    ROWLAZY["on"] = bool(args.row_lazy)
    if ROWLAZY["on"] and not (args.visfirst and args.optimizer in (None, "fused")) or (ROWLAZY["on"] and LAZY["on"]):
        raise SystemExit("--row-lazy needs --visfirst and the fused optimizer (and replaces --lazy-adam)")
    if args.lazy_adam and not (args.visfirst and args.optimizer in (None, "fused")):
        raise SystemExit("--lazy-adam needs --visfirst and the fused optimizer")
    if args.visfirst and args.optimizer == "torch":
        raise SystemExit("--visfirst hands the colour gradients over as rows: --optimizer fused (or none)")
    dev = torch.device("cuda")
    W, H, T = args.width, args.height, args.traversals
    truth = make_nodes(args.n_background, args.n_road, T, 0, dev, args.objects, args.object_size,
                       clear=(6.0 if args.converge else 0.0) if args.clear_radius is None else args.clear_radius)
    cams = []
    for t in range(T):
        vm, K = make_camera(W, H, yaw_deg=20.0 * t)
        cams.append((vm.to(dev), K.to(dev), torch.inverse(vm)[:, :3, :].to(dev), t))
    win = _win(dev)
    with torch.no_grad():
        targets = []
        for cam in cams:
            gs = gaussians_fused(truth, cam[2], cam[3], 3)
            r, a, _ = rasterization(gs["means"], gs["quats"], gs["scales"], gs["opacities"], gs["rgbs"], cam[0], cam[1], W, H,
                                    packed=False, render_mode="RGB", rasterize_mode="antialiased")
            targets.append(r[0].clamp(0, 1))
    mask = torch.ones(H, W, 1, dtype=torch.bool, device=dev)
    mask[: H // 8] = False                                                            # e.g. ego-vehicle / sky mask
    shipped = None
    if args.shipped:
        bg = torch.zeros(3, device=dev)
        gt_depth, gt_normal = [], []
        with torch.no_grad():
            for cam in cams:
                gs = gaussians_fused(truth, cam[2], cam[3], 3)
                col = camera_space_normals(gs["quats"], gs["scales"], gs["means"], cam[2], rgbs=gs["rgbs"])
                r, a, _ = rasterization(gs["means"], gs["quats"], gs["scales"], gs["opacities"], col, cam[0], cam[1], W, H,
                                        packed=False, render_mode="RGB+ED", rasterize_mode="antialiased")
                _, _, d, nrm = output_head(r, a, bg, None, depth=True, normal_channel=3)
                gt_depth.append(d); gt_normal.append(torch.nan_to_num(nrm, nan=0.5))
        ge = torch.Generator().manual_seed(11)      # (seeded on the host: every rank of a data-parallel run starts from the same model)
        shipped = {"exposure": (torch.eye(3, 4, device=dev)[None].repeat(T, 1, 1) + 0.02 * torch.randn(T, 3, 4, generator=ge).to(dev)).requires_grad_(True),
                   "bg": bg, "gt_depth": gt_depth, "gt_normal": gt_normal}
    g = torch.Generator().manual_seed(5)
    if args.converge:
        # something to learn: a random subset of the true Gaussians (the holes are what densification has to fill), positions
        # off by half a standard deviation of the Gaussian itself, shapes, opacities and colours perturbed
        LR["set"] = "reference"
        P = {}
        for name, p in truth.items():
            n = p["means"].shape[0]
            keep = (torch.rand(n, generator=g) >= args.drop).to(dev) if "instance_quats" not in p else torch.ones(n, dtype=torch.bool, device=dev)
            rn = lambda v, sd: (sd * torch.randn(v.shape, generator=g)).to(dev)
            q = {}
            for k, v in p.items():
                if k in ("instance_quats", "instance_trans"):
                    q[k] = v.clone()
                    continue
                w = v[keep]
                if k == "means":
                    w = w + rn(w, 0.5) * torch.exp(p["scales"][keep])
                elif k == "scales":
                    w = w + rn(w, 0.2)
                elif k == "quats":
                    w = w + rn(w, 0.1)
                elif k == "opacities":
                    w = w + rn(w, 0.5)
                else:
                    w = w + rn(w, 0.3)
                q[k] = w.contiguous().clone().requires_grad_(True)
            for k in ("instance_quats", "instance_trans"):
                if k in q:
                    q[k].requires_grad_(True)
            P[name] = q
    else:
        P = {name: {k: (v + (0.3 * torch.randn(v.shape, generator=g)).to(dev) * (k in ("features_dc", "features_rest", "features_adapters"))
                        ).clone().requires_grad_(True) for k, v in p.items()} for name, p in truth.items()}
    params = [v for p in P.values() for v in p.values()] + ([shipped["exposure"]] if shipped else [])
    mk_stats = lambda: [[torch.zeros(p["means"].shape[0], device=dev), torch.ones(p["means"].shape[0], device=dev),
                         torch.zeros(p["means"].shape[0], device=dev)] for p in P.values()]

    # (the chain-vs-fused comparison below runs both variants on the SAME parameters: no optimizer there)
    opt_kind = args.optimizer if (args.optimizer not in (None, "none") and (args.graph or args.only != "both")) else None

    def timed(fused):
        stats = mk_stats()
        opt = enable_row_lazy(make_optimizer(opt_kind, P, shipped), P) if opt_kind else None
        def one(i):
            for q in params:
                q.grad = None
            if opt is not None and LAZY["on"]:
                opt.prepare(i % T)
            loss = iteration(P, cams[i % T], targets[i % T], mask, fused, stats, win, W, H, shipped=shipped)
            if opt is not None:
                if VISFIRST["cs"] is not None:
                    VISFIRST["cs"].apply_to(opt)
                opt.step()
            return loss
        for i in range(3):
            loss = one(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()          # wall clock: with many nodes the host, not the GPU, sets the pace
        for i in range(args.reps):
            one(i)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.reps * 1e3, float(one(0)), stats

    def graphed():
        """The fused iteration as ONE graph launch per traversal: static camera / target tensors; the gradients are the
        tensors the captured backward assigned (`grads_of[t]`, static addresses inside graph t's memory pool -- what an
        optimizer would be pointed at after a replay).  Returns (wall ms, GPU ms, eager wall ms, loss check)."""
        import mtgs_amd
        from mtgs_amd import wrapper
        stats = mk_stats()
        grads_of = {}
        opt = enable_row_lazy(make_optimizer(opt_kind, P, shipped, capturable=True), P) if opt_kind else None

        def body(t):
            for q in params:
                q.grad = None
            loss = iteration(P, cams[t], targets[t], mask, True, stats, win, W, H, shipped=shipped)
            if opt is not None:
                if VISFIRST["cs"] is not None:
                    VISFIRST["cs"].apply_to(opt)
                opt.step()
            return loss

        def replay(t):
            if opt_kind == "fused":
                if LAZY["on"]:
                    opt.prepare(t)     # slice t of the per-traversal tensors caught up with the steps it missed (eager launch)
                opt.advance(active_slice=t if LAZY["on"] else None)   # this step's {lr / bc1, sqrt(bc2)}: one small copy
            graphs[t].replay()

        prep = (lambda t: opt.prepare(t)) if (opt is not None and LAZY["on"]) else (lambda t: None)   # (never inside graph_mode:
        #   its staging buffers are handed out in a fixed sequence; the catch-up is an eager launch in front of a frame)
        eager_loss = []
        for t in range(T):                                     # also teaches the size plan this scene's (n_vis, M)
            prep(t)
            eager_loss.append(float(body(t)))
        torch.cuda.synchronize()
        if os.environ.get("MTGS_TORCH_PROFILE"):      # development: which operators the iteration launches, by count
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                for i in range(4):
                    prep(i % T)
                    body(i % T)
                torch.cuda.synchronize()
            print(prof.key_averages().table(sort_by="count", row_limit=45, max_name_column_width=60))
        t0 = time.perf_counter()
        for i in range(args.reps):
            prep(i % T)
            body(i % T)
        torch.cuda.synchronize()
        eager_ms = (time.perf_counter() - t0) / args.reps * 1e3
        n_all = sum(p["means"].shape[0] for p in P.values())
        n_vis, M = wrapper._size_plan.seen[(1, n_all, W, H)]
        caps = (int(1.3 * n_vis) + 4096, int(1.3 * M) + 65536)
        graphs, losses, modes, flags = [], [], [], []
        side = torch.cuda.Stream()
        for t in range(T):
            gm = mtgs_amd.graph_mode(*caps)
            prep(t)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side), gm:                    # warm-up on the capture stream (allocator, lazy init)
                body(t)
            torch.cuda.current_stream().wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with gm, torch.cuda.graph(g):
                losses.append(body(t))
            grads_of[t] = [q.grad for q in params]
            graphs.append(g); modes.append(gm)
        graph_loss = []
        for t in range(T):
            replay(t)
            torch.cuda.synchronize()
            graph_loss.append(float(losses[t]))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for i in range(args.reps):
            replay(i % T)
        e1.record()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / args.reps * 1e3
        return wall, e0.elapsed_time(e1) / args.reps, eager_ms, eager_loss, graph_loss, caps

    if args.graph:
        wall, gpu, eager_ms, l_e, l_g, caps = graphed()
        print(f"fused iteration, {W}x{H}{' shipped options' if shipped else ''}: eager {eager_ms:.3f} ms wall -> one graph launch "
              f"{wall:.3f} ms wall ({gpu:.3f} ms between GPU events); capacities {caps}; loss eager {l_e} graph {l_g}")
        if not opt_kind:      # (with an optimizer in the loop the parameters move between the eager pass and the replays)
            assert all(abs(a - b) <= 1e-4 * max(1.0, abs(a)) for a, b in zip(l_e, l_g)), (l_e, l_g)
        else:
            assert all(math.isfinite(v) for v in l_g), (l_e, l_g)
        return
    if args.only != "both" and not args.steps:
        t1, l1, _ = timed(args.only == "fused")
        print(f"{args.only}: {t1:.2f} ms per iteration, loss {l1:.6f}")
        return
    if args.only == "both":
      tc, lc, sc = timed(False)
      tf, lf, sf = timed(True)
      n_all = sum(p["means"].shape[0] for p in P.values())
      print(f"{n_all} Gaussians in {len(P)} nodes ({T} traversals), {W}x{H}: iteration (fwd + loss + bwd + statistics) "
            f"chain {tc:.2f} ms -> fused {tf:.2f} ms ({tc / tf:.2f}x); loss chain {lc:.6f} fused {lf:.6f}")
      assert abs(lc - lf) <= (2e-4 if shipped else 2e-5) * max(1.0, abs(lc)), (lc, lf)
      for a, b in zip(sc, sf):
          assert torch.allclose(a[1], b[1]) and torch.allclose(a[2], b[2])
    if args.steps:
        rank, world = 0, 1
        if args.dp:
            from mtgs_amd import dist as mdist
            rank, _, world = mdist.init_from_env()
        log = print if rank == 0 else (lambda *a, **k: None)
        refine_cfg = None
        if args.converge:
            from mtgs_amd.densify import RefineConfig
            # config/MTGS.py:59-71 as shipped, but: the gradient threshold scaled once for this scene (nuPlan's 0.001 is for real
            # images at 30 000 steps), refine_every from the command line
            refine_cfg = RefineConfig(refine_every=max(args.refine_every, 1), densify_grad_thresh=args.grad_thresh or 4e-4,
                                      split_screen_size=args.split_screen_size, cull_alpha_thresh=args.cull_alpha,
                                      densify_size_thresh=args.size_thresh)
        curve, sizes = train_loop(P, cams, targets, mask, win, W, H, args.steps, args.refine_every, shipped=shipped, world=world,
                                  rank=rank, accumulate=args.accumulate, log=log, sparse=args.dp_exchange == "sparse",
                                  optimizer=args.optimizer if args.optimizer in ("torch", "fused") else "fused",
                                  graph=args.train_graph, one_graph=args.one_graph, refine_cfg=refine_cfg, poll_every=args.poll_every,
                                  means_lr_final=8e-6 if args.converge else None,
                                  steady=tuple(args.steady) if args.steady else None, first_cap_scale=args.first_cap_scale,
                                  densify_from=(5 * args.refine_every if args.converge else 0) if args.densify_from is None else args.densify_from)
        if args.trace_refinements and args.refine_every:
            for r in range(args.refine_every, args.steps, args.refine_every):
                pts = [r - 2 * T, r - T, r, r + T, r + 2 * T, r + 4 * T, r + 8 * T]
                log(f"around step {r}: " + " ".join(f"{q}:{sum(curve[q:q + T]) / T:.4f}" for q in pts if 0 <= q and q + T <= len(curve)))
        k = max(1, args.steps // 8)
        log("loss:", " ".join(f"{sum(curve[j:j + k]) / len(curve[j:j + k]):.4f}" for j in range(0, args.steps, k)))
        n_now = sum(p["means"].shape[0] for p in P.values())
        if args.dp:
            t = torch.tensor([n_now, -n_now], device=dev)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            assert int(t[0]) == n_now and int(-t[1]) == n_now, "N differs between the ranks"
            log(f"{world} ranks: N = {n_now} on every rank after {len(sizes)} refinements")
            torch.distributed.destroy_process_group()
        if args.converge:
            # training has to WORK here: the loss falls through the refinements (mean of the last tenth against the first tenth)
            k10 = max(1, args.steps // 10)
            first, last = sum(curve[:k10]) / k10, sum(curve[-k10:]) / k10
            log(f"converge: loss {first:.4f} -> {last:.4f} ({last / first:.2f}x) through {len(sizes)} refinements, N {sizes}")
            assert all(math.isfinite(c) for c in curve), curve[-5:]
            if args.steps >= 100:
                assert last < 0.7 * first, (first, last)
        elif args.refine_every:
            # the synthetic scene starts from the TRUE geometry and the reference's duplication is not image-preserving (a
            # clone doubles its parent's contribution until the opacities adapt), so every refinement perturbs a correct
            # model: the run checks that N can change under the fused path (tables, statistics, optimizer state) and
            # that training keeps working
            assert all(math.isfinite(c) for c in curve), curve[-5:]
            if args.steps >= 60:      # (shorter runs end right behind a refinement)
                assert min(curve) < 0.7 * curve[0] and curve[-1] < 1.5 * curve[0], curve[-5:]
        else:
            assert sum(curve[-T:]) < 0.7 * sum(curve[:T]), "training did not reduce the loss"


if __name__ == "__main__":
    main()
