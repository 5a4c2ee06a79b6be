"""Writes tests/golden/lidar_ref.npz: the inputs of one paint case and one depth case with the outputs of the reference's OWN code
for them, so that the pin on get_rgb_point_cloud, get_semantic_point_cloud and _get_depth_from_lidar travels without the
reference.  Inputs and recorded results only; no line of the reference is copied: at generation time
mtgs/utils/nuplan_pointcloud.py is imported by path, and get_semantic_point_cloud (nuplan_scripts/utils/nuplan_utils_custom.py)
and CustomInputDataset._get_depth_from_lidar (mtgs/dataset/custom_dataset.py) are cut out of their files with `ast`, the method's
annotations stripped, and called with a stand-in `self` and a stand-in camera and with points= so that no file is read.

    paint/points float32 [N, 3]   paint/lidar2imgs float64 [3, 4, 4]   paint/images uint8 [3, 37, 53, 3] (BGR)   paint/masks uint8 [3, 37, 53, 1]
    paint/rgb float64 [N, 3]   paint/labels int32 [N]   paint/fov bool [N]   paint/count int32 [N] (the reference one camera at a time)
    paint/rgb_max_diff float64: the largest |reference - tests.lidar_refs| of rgb on this machine
    depth/points float32 [M, 3]   depth/lidar2cam float32 [4, 4]   depth/K float32 [3, 3]   depth/image float32 [37, 53, 1]

The maker asserts that tests/lidar_refs.py reproduces the reference on these inputs: fov, count, labels, the set of hit pixels and
the depth values exactly.  A seed that puts a point on a decision boundary where the summation order of the reference's matrix
product matters fails that assertion: choose another.

Run from the repository root: python tests/golden/make_lidar_golden.py /path/to/MTGS [--seed S]"""
import argparse
import ast
import importlib.util
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
H, W, N_PAINT, N_DEPTH = 37, 53, 6000, 6000
YAWS = (0.0, 40.0, 160.0)        # half a field of view is 41 degrees: cameras 0 and 1 overlap, 81..119 and 201..319 degrees see nothing


def cut(path: Path, name: str, namespace: dict):
    """the function or method `name` of the file, compiled by itself without its annotations"""
    tree = ast.parse(path.read_text())
    fn = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == name)
    fn.returns = None
    for a in fn.args.args + fn.args.kwonlyargs:
        a.annotation = None
    module = ast.fix_missing_locations(ast.Module(body=[fn], type_ignores=[]))
    exec(compile(module, str(path), "exec"), namespace)
    return namespace[name]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference", type=Path, help="a checkout of OpenDriveLab/MTGS")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    from tests import lidar_refs as R

    spec = importlib.util.spec_from_file_location("ref_nuplan_pointcloud", a.reference / "mtgs" / "utils" / "nuplan_pointcloud.py")
    ref_pc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_pc)
    ref_semantic = cut(a.reference / "nuplan_scripts" / "utils" / "nuplan_utils_custom.py", "get_semantic_point_cloud", {"np": np, "torch": torch})
    ref_depth = cut(a.reference / "mtgs" / "dataset" / "custom_dataset.py", "_get_depth_from_lidar", {"np": np, "load_lidar": None})

    rng = np.random.default_rng(a.seed)
    out = {}
    # ---- paint --------------------------------------------------------------------------------------------------------------------
    pts = R.sweep(rng, N_PAINT)
    mats = np.stack([R.camera(y, 30.0, rng.uniform(-0.5, 0.5, 3), W, H)[0] for y in YAWS])
    images = rng.integers(0, 256, (len(YAWS), H, W, 3), dtype=np.uint8)
    masks = rng.integers(0, 20, (len(YAWS), H, W, 1), dtype=np.uint8)
    rgb, fov = ref_pc.get_rgb_point_cloud(pts, mats, list(images))
    labels, fov_s = ref_semantic(pts, mats, masks)
    count = sum(ref_pc.get_rgb_point_cloud(pts, mats[c:c + 1], [images[c]])[1].astype(np.int32) for c in range(len(YAWS)))
    mine = R.paint_points(pts, mats, images, masks, "bgr")
    assert np.array_equal(fov, fov_s) and np.array_equal(mine.fov, fov) and np.array_equal(mine.count, count), "fov or count differ: another seed"
    assert np.array_equal(mine.labels, labels), "labels differ: another seed"
    diff = float(np.abs(mine.rgb - rgb).max())
    assert diff <= 1e-10, diff
    shares = [float((count == k).mean()) for k in range(3)]
    assert min(shares) > 0.1, shares
    out.update({"paint/points": pts, "paint/lidar2imgs": mats, "paint/images": images, "paint/masks": masks, "paint/rgb": rgb,
                "paint/labels": labels.astype(np.int32), "paint/fov": fov, "paint/count": count.astype(np.int32),
                "paint/rgb_max_diff": np.float64(diff)})
    # ---- depth --------------------------------------------------------------------------------------------------------------------
    pts_d = R.sweep(rng, N_DEPTH)
    _, E, K = R.camera(20.0, 30.0, rng.uniform(-0.5, 0.5, 3), W, H)
    E32, K32 = E.astype(np.float32), K.astype(np.float32)
    stand_in = SimpleNamespace(_dataparser_outputs=SimpleNamespace(lidar_to_cams=[torch.from_numpy(E32)], lidar_filenames=[None]))
    camera = SimpleNamespace(height=torch.tensor(H), width=torch.tensor(W), get_intrinsics_matrices=lambda: torch.from_numpy(K32))
    camera.reshape = lambda shape: camera
    image = ref_depth(stand_in, 0, camera, points=pts_d)
    got, winner = R.depth_image(pts_d, E32, K32, W, H, return_index=True)
    assert image.dtype == np.float32 and image.shape == (H, W, 1)
    assert np.array_equal((image != 0)[..., 0], winner >= 0), "the hit pixels differ: another seed"
    assert np.array_equal(image, got), "depth values differ: another seed"
    hits = int((winner >= 0).sum())
    out.update({"depth/points": pts_d, "depth/lidar2cam": E32, "depth/K": K32, "depth/image": image})
    path = Path(__file__).resolve().parent / "lidar_ref.npz"
    np.savez_compressed(path, **out)
    print(f"paint: N={N_PAINT} seen by 0/1/2+ cameras {shares[0]:.2f}/{shares[1]:.2f}/{1 - shares[0] - shares[1]:.2f}, rgb max diff {diff:.3g}; "
          f"depth: {hits} of {H * W} pixels hit; {path.stat().st_size} bytes")


if __name__ == "__main__":
    main()
