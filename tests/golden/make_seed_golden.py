#!/usr/bin/env python3
"""Golden vectors for mtgs_amd.seed (knn_distances / seed_gaussians), produced in the build container.

Neighbour distances: scikit-learn's NearestNeighbors(n_neighbors=k + 1, metric="euclidean") exactly as
VanillaGaussianSplattingModel.k_nearest_sklearn calls it (vanilla_gaussian_splatting.py:372-390), first column dropped, cast
to float32.  Per-point seeding: the lines of populate_modules (:129-172) run as written on the CPU in float32, with the
REFERENCE's RGB2SH, rotate_vector_to_vector and matrix_to_quaternion imported by path from gaussian_model/utils.py; the
normals -> quaternion chain is also run in float64, and the f32-vs-f64 gap is stored as the tolerance floor, with the margin
of every row to a matrix_to_quaternion branch boundary.  Writes tests/golden/seed_ref.npz (inputs + outputs only)."""
import importlib.util
from pathlib import Path

import numpy as np
import torch
from sklearn.neighbors import NearestNeighbors

REF = Path("/root/reference/mtgs/scene_model/gaussian_model/utils.py")
spec = importlib.util.spec_from_file_location("ref_gaussian_utils", REF)
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)

rng = np.random.default_rng(11)


def knn(x, k):
    d, _ = NearestNeighbors(n_neighbors=k + 1, algorithm="auto", metric="euclidean").fit(x).kneighbors(x)
    return d[:, 1:].astype(np.float32)


def street(n_ground, n_facade, n_far):
    ground = np.stack([rng.uniform(0, 200, n_ground), rng.uniform(-4, 4, n_ground), rng.normal(0, 0.02, n_ground)], -1)
    side = rng.choice([-8.0, 8.0], n_facade)
    facade = np.stack([rng.uniform(0, 200, n_facade), side + rng.normal(0, 0.05, n_facade), rng.uniform(0, 15, n_facade)], -1)
    far = np.array([600.0, 300.0, 20.0]) + rng.normal(0, 30.0, (n_far, 3))
    return rng.permutation(np.concatenate([ground, facade, far])).astype(np.float32)


def shell(n, radius):
    theta, phi = rng.uniform(0, 2 * np.pi, n), rng.uniform(np.pi / 4, np.pi / 2, n)
    return (radius * np.stack([np.sin(phi) * np.cos(theta), np.sin(phi) * np.sin(theta), np.cos(phi)], -1)).astype(np.float32)


def with_duplicates(x):
    """60 exact copies of existing points; point 7 ends up present four times"""
    src = np.concatenate([[7, 7, 7], rng.integers(0, x.shape[0], 57)])
    return np.concatenate([x, x[src]])[rng.permutation(x.shape[0] + 60)]


out, cases = {}, {}
st = street(1300, 650, 50)
cases["street"] = (st, 3)
cases["duplicates"] = (with_duplicates(st), 3)
sky = shell(1500, 2000.0)
cases["sky"] = (sky, 3)
plane = np.stack([rng.uniform(-50, 50, 1500), rng.uniform(-20, 20, 1500), np.full(1500, 1.25)], -1).astype(np.float32)
cases["plane"] = (plane, 3)
t = rng.uniform(0, 300, 800)
cases["line"] = (np.stack([t, np.full(800, -3.0), np.full(800, 0.5)], -1).astype(np.float32), 3)
cases["offset"] = ((street(1000, 450, 50).astype(np.float64) + np.array([1e5, -1e5, 1e5])).astype(np.float32), 3)
cluster = np.concatenate([rng.normal(0, 0.5, (3000, 3)), rng.uniform(-400, 400, (30, 3))])
cases["outliers"] = (rng.permutation(cluster).astype(np.float32), 3)
cases["n4"] = (rng.normal(0, 1, (4, 3)).astype(np.float32), 3)
cases["sky_k1"] = (sky, 1)
cases["sky_k8"] = (sky, 8)

for name, (x, k) in cases.items():
    d = knn(x, k)
    if name not in ("sky_k1", "sky_k8"):
        out[f"{name}_xyz"] = x
    out[f"{name}_k"] = np.int64(k)
    out[f"{name}_dist"] = d
    print(f"{name:12s} N={x.shape[0]:5d} k={k} zeros={int((d == 0).sum()):4d} min>0 {d[d > 0].min():.3e} max {d.max():.3e}")
out["knn_cases"] = np.array(list(cases))
out["sky_k1_xyz_from"] = np.array("sky")
out["sky_k8_xyz_from"] = np.array("sky")

# ---- seed_gaussians: populate_modules as written ----------------------------------------------------------------------
N = 1200
xyz = street(800, 370, 30)
xyz[11:14] = xyz[10]                                   # one point present four times: mean distance 0, scale -inf
rgb = rng.integers(0, 256, (N, 3)).astype(np.float32)
rgb[0], rgb[1] = (0, 255, 128), (255, 0, 1)
normals = rng.normal(0, 1, (N, 3))
normals *= rng.uniform(0.2, 3.0, (N, 1)) / np.linalg.norm(normals, axis=1, keepdims=True)
special = np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 0]], np.float64)
normals[:special.shape[0]] = special
normals = normals.astype(np.float32)
points_3d = {"xyz": torch.from_numpy(xyz), "rgb": torch.from_numpy(rgb), "normals": torch.from_numpy(normals)}

distances = torch.from_numpy(knn(xyz, 3))
avg_dist = distances.mean(dim=-1, keepdim=True)
opacities = torch.logit(0.1 * torch.ones(N, 1))
dc_sh = ref.RGB2SH(points_3d["rgb"] / 255)
dc_logit = torch.logit(points_3d["rgb"] / 255, eps=1e-10)
scales = torch.log(avg_dist.repeat(1, 3))
scales[:, 2] = torch.log((avg_dist / 10)[:, 0])


def quats_of(normals_seed):
    normals_seed = normals_seed / torch.norm(normals_seed, dim=-1, keepdim=True)
    mat = ref.rotate_vector_to_vector(
        torch.tensor([0, 0, 1], dtype=normals_seed.dtype, device=normals_seed.device).repeat(normals_seed.shape[0], 1), normals_seed)
    return ref.matrix_to_quaternion(mat), mat


q32, _ = quats_of(points_3d["normals"].float())
torch.set_default_dtype(torch.float64)     # rotate_vector_to_vector writes torch.eye(3) of the default dtype into its result
q64, m64 = quats_of(points_3d["normals"].double())
torch.set_default_dtype(torch.float32)
assert torch.equal(torch.isnan(q32), torch.isnan(q64))
fin = torch.isfinite(q64).all(dim=1)
# distance of every row to a decision of matrix_to_quaternion that the row reaches: the sign of the trace, and, where the trace
# is not clearly positive, the three comparisons of diagonal entries
d0, d1, d2 = m64[:, 0, 0], m64[:, 1, 1], m64[:, 2, 2]
trace = d0 + d1 + d2
diag = torch.stack([(d0 - d1).abs(), (d0 - d2).abs(), (d1 - d2).abs()], dim=1).min(dim=1).values
margin = torch.where(trace > 1e-4, trace.abs(), torch.minimum(trace.abs(), diag))
unit = points_3d["normals"].double() / torch.norm(points_3d["normals"].double(), dim=-1, keepdim=True)
c64 = unit[:, 2]
well = fin & (margin > 1e-4) & ~((c64 > -1) & (c64 < -0.999))
gap = float((q32.double() - q64)[well].abs().max())
print(f"seed: N={N} -inf scales {int(torch.isinf(scales).any(dim=1).sum())}  quat gap {gap:.2e}  near a branch {int((fin & (margin <= 1e-4)).sum())}  "
      f"near the antipode {int(((c64 > -1) & (c64 < -0.999)).sum())}  opacity {float(opacities[0, 0])!r}")
out.update(seed_xyz=xyz, seed_rgb=rgb.astype(np.uint8), seed_normals=normals, seed_dist=distances.numpy(), seed_scales=scales.numpy(),
           seed_dc_sh=dc_sh.numpy(), seed_dc_logit=dc_logit.numpy(), seed_opacities=opacities.numpy(), seed_quats32=q32.numpy(),
           seed_quats64=q64.numpy(), seed_gap=np.float64(gap), seed_branch_margin=margin.numpy(), seed_c64=c64.numpy(),
           seed_special_rows=np.int64(special.shape[0]), C0=np.float64(0.28209479177387814))
dst = Path(__file__).resolve().parent / "seed_ref.npz"
np.savez_compressed(dst, **out)
print(dst, dst.stat().st_size, "bytes")
