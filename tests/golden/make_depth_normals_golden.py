#!/usr/bin/env python3
"""Golden vectors for mtgs_amd.loss.normals_from_depth / depth_normal_loss, produced in the build container by the REFERENCE's
own functions: mtgs/utils/geometric_loss.py and mtgs/utils/camera_utils.py are imported by path, with empty stand-ins for
cv2, torchmetrics.image and pyquaternion (imported at module level there, not used by these functions).  MTGS's depth
normal term (mtgs_scene_graph.py:912-935) is then run as written:

    gt_normal = normal_from_depth_image(depth, fx, fy, cx, cy, (W, H), c2w=eye(4), smooth=False)
    gt_normal = (1 + gt_normal @ diag([1, -1, -1])) / 2
    m         = ((depth > 0.1) & (depth < 50) & mask).squeeze(-1)
    loss      = |gt_normal - pred|[m].mean() + TVLoss()(pred)          (gradient with respect to pred from autograd)

in float32 as MTGS runs it, and in float64: get_means3d_backproj converts to float32 whatever it gets, so the f64 run
restates its back-projection in f64 and hands it to the reference's pcd_to_normal.  The f32-vs-f64 gap of the target is
stored per case as the tolerance floor.  Writes tests/golden/depth_normals_ref.npz (inputs + outputs only)."""
import importlib.util
import sys
import types
from pathlib import Path

import numpy as np
import torch

REF = Path("/root/reference/mtgs/utils")
for name, attrs in (("cv2", ()), ("torchmetrics", ()),
                    ("torchmetrics.image", ("MultiScaleStructuralSimilarityIndexMeasure", "StructuralSimilarityIndexMeasure")),
                    ("pyquaternion", ("Quaternion",)), ("mtgs", ()), ("mtgs.utils", ())):
    mod = types.ModuleType(name)
    for a in attrs:
        setattr(mod, a, object)
    sys.modules.setdefault(name, mod)


def load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


cam = load("mtgs.utils.camera_utils", REF / "camera_utils.py")
geo = load("mtgs.utils.geometric_loss", REF / "geometric_loss.py")

g = torch.Generator().manual_seed(3)


def normals32(depth, K):
    H, W = depth.shape[:2]
    n = geo.normal_from_depth_image(depths=depth.detach(), fx=float(K[0, 0]), fy=float(K[1, 1]), cx=float(K[0, 2]),
                                    cy=float(K[1, 2]), img_size=(W, H), c2w=torch.eye(4, dtype=torch.float), device="cpu")
    n = n @ torch.diag(n.new_tensor([1, -1, -1]))
    return (1 + n) / 2


def normals64(depth, K):
    """the same chain in f64: get_means3d_backproj's arithmetic restated (it forces f32), then the reference's pcd_to_normal"""
    H, W = depth.shape[:2]
    d = depth.to(torch.float64).reshape(-1)
    uv = cam.get_camera_coords((W, H)).to(torch.float64)
    K = K.to(torch.float64)
    P = torch.empty((H * W, 3), dtype=torch.float64)
    P[:, 0] = (uv[:, 0] - K[0, 2]) * d / K[0, 0]
    P[:, 1] = (uv[:, 1] - K[1, 2]) * d / K[1, 1]
    P[:, 2] = d
    P = P @ torch.linalg.inv(torch.eye(3, dtype=torch.float64)) + torch.zeros(3, dtype=torch.float64)
    n = geo.pcd_to_normal(P.view(H, W, 3))
    n = n @ torch.diag(n.new_tensor([1, -1, -1]))
    return (1 + n) / 2


def loss_and_grad(gt_normal, depth, pred, mask):
    pred = pred.clone().requires_grad_(True)
    m = ((depth > 0.1) & (depth < 50) & mask).squeeze(-1)
    loss = torch.abs(gt_normal - pred)[m].mean() + geo.TVLoss()(pred)
    loss.backward()
    return loss.detach(), pred.grad


def plane_depth(H, W, K, n, off):
    """depth of the plane n . X = off seen through pixel centres"""
    u = torch.arange(W, dtype=torch.float64) + 0.5
    v = torch.arange(H, dtype=torch.float64) + 0.5
    rx = ((u - float(K[0, 2])) / float(K[0, 0]))[None, :]
    ry = ((v - float(K[1, 2])) / float(K[1, 1]))[:, None]
    return (off / (n[0] * rx + n[1] * ry + n[2])).float()[..., None]


def intrinsics(W, H):
    return torch.tensor([[0.9 * W + 0.25, 0.0, W / 2 - 0.75], [0.0, 0.85 * W + 0.5, H / 2 + 0.5], [0.0, 0.0, 1.0]])


def smooth_depth(H, W, lo, hi):
    y = torch.linspace(0, 1, H)[:, None]
    x = torch.linspace(0, 1, W)[None, :]
    d = lo + (hi - lo) * (0.5 + 0.3 * torch.sin(5 * x + 2 * y) * torch.cos(3 * y))
    return (d + 0.01 * torch.rand(H, W, generator=g))[..., None]


cases = {}
H, W = 24, 32
K = intrinsics(W, H)
cases["plane"] = (plane_depth(H, W, K, (0.1, -0.9, 0.4), 2.0), K, None)
d = plane_depth(H, W, K, (0.05, 0.2, 1.0), 6.0)
d[:, W // 2:] += 9.0
d[H // 3:, :] *= 1.0 + 0.01 * torch.arange(W)[None, :, None]
cases["step"] = (d, K, None)
d = smooth_depth(H, W, 2.0, 40.0)
pick = torch.rand(H, W, 1, generator=g)
d[pick < 0.1] = 0.0
d[(pick >= 0.1) & (pick < 0.15)] = 80.0
d[(pick >= 0.15) & (pick < 0.18)] = -3.0
d[(pick >= 0.18) & (pick < 0.21)] = 0.1
d[(pick >= 0.21) & (pick < 0.24)] = 50.0
cases["zeros_range"] = (d, K, None)
d = smooth_depth(H, W, 3.0, 20.0)
d[5, 7] = float("nan")
d[11, 20] = float("inf")
d[17, 3] = -float("inf")
cases["nonfinite"] = (d, K, None)
H2, W2 = 17, 23
K2 = intrinsics(W2, H2)
cases["odd"] = (smooth_depth(H2, W2, 1.0, 30.0), K2, None)
cases["mask"] = (smooth_depth(H, W, 2.0, 60.0), K, torch.rand(H, W, 1, generator=g) > 0.4)
cases["tiny"] = (smooth_depth(2, 5, 1.0, 5.0), intrinsics(5, 2), None)

out = {}
for name, (depth, K, mask) in cases.items():
    H, W = depth.shape[:2]
    m = torch.ones(H, W, 1, dtype=torch.bool) if mask is None else mask
    pred = torch.rand(H, W, 3, generator=g)
    n32 = normals32(depth, K)
    n64 = normals64(depth, K)
    fin = torch.isfinite(n64) & torch.isfinite(n32.double())
    assert torch.equal(torch.isnan(n32), torch.isnan(n64)), name
    gap = float((n32.double() - n64)[fin].abs().max()) if fin.any() else 0.0
    l32, g32 = loss_and_grad(n32, depth, pred, m)
    l64, g64 = loss_and_grad(n64, depth.double(), pred.double(), m)
    out[f"{name}_depth"] = depth.numpy()
    out[f"{name}_K"] = K.numpy()
    out[f"{name}_mask"] = m.numpy()
    out[f"{name}_pred"] = pred.numpy()
    out[f"{name}_normals32"] = n32.numpy()
    out[f"{name}_normals64"] = n64.numpy()
    out[f"{name}_gap"] = np.float64(gap)
    out[f"{name}_loss32"] = np.float64(l32)
    out[f"{name}_loss64"] = np.float64(l64)
    out[f"{name}_grad32"] = g32.numpy()
    out[f"{name}_grad64"] = g64.numpy()
    print(f"{name:12s} {H}x{W}: loss f32 {float(l32):.7f} f64 {float(l64):.7f}  normal gap {gap:.2e}  "
          f"selected {int(((depth > 0.1) & (depth < 50) & m).sum())}")
out["cases"] = np.array(list(cases))
dst = Path(__file__).resolve().parent / "depth_normals_ref.npz"
np.savez_compressed(dst, **out)
print(dst, dst.stat().st_size, "bytes")
