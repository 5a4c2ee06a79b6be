"""Writes tests/golden/stack_ref.npz: three frames of one traversal (sweeps, boxes, cameras) with the outputs of the reference's OWN
code for them, so that the pin on extract_frame_background_instance_lidar, InstanceObject.points_ego,
accumulate_background_box_point and the per-frame filtering of StackRGBPointCloud travels without the reference.  Inputs and
recorded results only; no line of the reference is copied: at generation time the functions and classes of
nuplan_scripts/utils/stack_point_cloud_utils.py and get_semantic_point_cloud (nuplan_scripts/utils/nuplan_utils_custom.py) are cut
out of their files with `ast` and mtgs/utils/nuplan_pointcloud.py is imported by path, as tests/golden/make_lidar_golden.py does.
The per-frame steps of stack_RGB_point_cloud.py:93-126 (concatenate the background and every instance's points_ego, paint them, keep
the rows the cameras see, group by group) are driven from here with those functions.

    f{0,1,2}/points float32 [N, 3]   boxes float64 [B, 7]   names, tokens str [B]   lidar2global, lidar2imgs float64   (inputs)
    images uint8 [3, 37, 53, 3] (BGR)   masks uint8 [3, 37, 53, 1]                   (one set of images for the three frames)
    f*/pose, f*/inverse float64 [B, 4, 4]: InstanceObject.pose and its np.linalg.inv (NaN for a skipped class)
    f*/raw_sizes int64 [B + 1]: points of the background and of every box before the cameras; f*/dropped: points lost in margins
    f*/bg_points, bg_rgb, bg_labels; f*/sizes int64 [B]; f*/inst_points (box frame), inst_rgb, inst_labels in box order
    stack/xyz (global), stack/labels: the background after `< 10`; stack/tokens, stack/sizes: the tracks that have points
    box_frame_max_diff, rgb_max_diff, global_max_diff: the largest |reference - tests.stack_refs| on this machine

The maker asserts that tests/stack_refs.py reproduces the reference's decisions exactly (the background set, every group's size and
order, fov, labels), that the traversal's colours and instance clouds are the per-frame ones concatenated, and that the inputs
exercise the rule.  A seed that puts a point on a boundary where the summation order of the reference's matrix product decides fails
an assertion: choose another.

Run from the repository root: python tests/golden/make_stack_golden.py /path/to/MTGS [--seed S]"""
import argparse
import ast
import importlib.util
import os
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
H, W, N_FRAME, N_BOXES, FRAMES = 37, 53, 1500, 21, 3
YAWS = (0.0, 40.0, 160.0)


def cut(path: Path, names, namespace: dict):
    """the top-level functions and classes `names` of the file, compiled by themselves without their annotations"""
    body = [n for n in ast.parse(path.read_text()).body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names]
    assert {n.name for n in body} == set(names), names
    for node in body:
        for fn in (n for n in ast.walk(node) if isinstance(n, ast.FunctionDef)):
            fn.returns = None
            for a in fn.args.args + fn.args.kwonlyargs:
                a.annotation = None
    exec(compile(ast.fix_missing_locations(ast.Module(body=body, type_ignores=[])), str(path), "exec"), namespace)
    return namespace


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference", type=Path, help="a checkout of OpenDriveLab/MTGS")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    from mtgs_amd.stack import box_matrices
    from tests import lidar_refs, stack_refs as R

    ref = cut(a.reference / "nuplan_scripts" / "utils" / "stack_point_cloud_utils.py",
              ["InstanceObjectTrack", "InstanceObject", "padding_column", "split_points", "extract_frame_background_instance_lidar",
               "accumulate_box_point", "accumulate_background_point", "accumulate_background_box_point", "transform_points_lidar2global"],
              {"np": np, "torch": torch, "os": os, "TORCH_DEVICE": "cpu", "load_lidar": None, "NUPLAN_SENSOR_ROOT": None})
    semantic = cut(a.reference / "nuplan_scripts" / "utils" / "nuplan_utils_custom.py", ["get_semantic_point_cloud"],
                   {"np": np, "torch": torch})["get_semantic_point_cloud"]
    spec = importlib.util.spec_from_file_location("ref_nuplan_pointcloud", a.reference / "mtgs" / "utils" / "nuplan_pointcloud.py")
    ref_pc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_pc)

    rng = np.random.default_rng(a.seed)
    images = rng.integers(0, 256, (len(YAWS), H, W, 3), dtype=np.uint8)
    masks = rng.integers(0, 20, (len(YAWS), H, W, 1), dtype=np.uint8)
    base = R.boxes_on_the_ring(rng, N_BOXES)
    base[N_BOXES - 1, :2] = [80.0, 5.0]                            # a track no point reaches
    all_names = np.array(["vehicle"] * N_BOXES, dtype="<U16")
    all_names[[6, 7]] = ["traffic_cone", "barrier"]
    all_tokens = np.array([f"track{i:02d}" for i in range(N_BOXES)])
    out = {"images": images, "masks": masks}
    infos, mine, inputs = [], [], []
    diffs = {"box_frame": 0.0, "rgb": 0.0, "global": 0.0}
    seen = {"dropped": 0, "earlier_owner": 0}
    for f in range(FRAMES):
        present = np.ones(N_BOXES, dtype=bool)
        present[4] = f != 1                                        # a track absent from the middle frame
        boxes = base[present].copy()
        boxes[:, :2] += [0.4 * f, -0.3 * f]                        # the scene moves as a whole: the overlaps stay
        names, tokens = all_names[present], all_tokens[present]
        pts = R.sweep_with_boxes(rng, N_FRAME, boxes[:-1])                 # none for the last track
        l2g = R.lidar2global(rng, f)
        mats = np.stack([lidar_refs.camera(y + 5.0 * f, 30.0, rng.uniform(-0.5, 0.5, 3), W, H)[0] for y in YAWS])
        B = len(boxes)
        # ---- the reference: :91, then :93-126 driven from here
        info = {"track_tokens": list(tokens), "gt_boxes": boxes, "gt_names": list(names), "lidar2global": l2g,
                "gt_velocity": np.zeros((B, 2)), "frame_idx": f}
        bi = info["back_instance_info"] = ref["extract_frame_background_instance_lidar"](info, l2g=False, points=pts)
        objects = bi["instance"]
        raw_bg = bi["background_points"]
        raw_sizes = np.array([len(raw_bg)] + [len(objects[t].points) if t in objects else 0 for t in tokens])
        ego = {t: o.points_ego for t, o in objects.items()}
        raw_q = {t: o.points.copy() for t, o in objects.items()}
        all_points = np.concatenate([raw_bg] + [ego[t] for t in objects])
        group = np.concatenate([np.zeros(len(raw_bg))] + [np.full(len(ego[t]), i + 1.0) for i, t in enumerate(objects)])
        rgb, fov = ref_pc.get_rgb_point_cloud(all_points, mats, list(images))
        labels, fov_sem = semantic(all_points, mats, masks)
        keep = (group == 0) & fov & fov_sem
        bi["background_points"], bi["background_RGBs"], bi["background_sem_labels"] = all_points[keep], rgb[keep], labels[keep]
        for i, (t, o) in enumerate(objects.items()):
            keep = (group == i + 1) & fov & fov_sem
            o.points, o.rgbs, o.sem_labels = o.points[fov[group == i + 1]], rgb[keep], labels[keep]
        # ---- the restatement on the same inputs, with the product's matrices
        include = np.array([n not in R.SKIP_CLASSES for n in names])
        lidar2box, box2lidar, _ = box_matrices(boxes)
        pose = np.full((B, 4, 4), np.nan)
        inverse = np.full((B, 4, 4), np.nan)
        for b, t in enumerate(tokens):
            if t in objects:
                pose[b], inverse[b] = objects[t].pose, np.linalg.inv(objects[t].pose)
        assert np.array_equal(pose[include], box2lidar[include]) and np.array_equal(inverse[include], lidar2box[include])
        assert set(objects) == set(tokens[include]) and list(objects) == list(tokens[include])
        s = R.split_sweep(pts, boxes, lidar2box, include)
        assert np.array_equal(np.diff(s.offsets)[: B + 1], raw_sizes), "group sizes differ: another seed"
        assert R.ulp_equal(s.points[: s.offsets[1]], raw_bg), "the background differs: another seed"
        for b, t in enumerate(tokens):
            if t in objects:
                got = s.points[s.offsets[1 + b]: s.offsets[2 + b]]
                if len(got):
                    diffs["box_frame"] = max(diffs["box_frame"], float(np.abs(got - raw_q[t]).max()))
        fr = R.stack_frame(pts, boxes, lidar2box, box2lidar, include, mats, images, masks, "bgr")
        sizes = np.array([len(objects[t].points) if t in objects else 0 for t in tokens])
        assert np.array_equal(np.diff(fr.offsets), np.concatenate([[len(bi["background_points"])], sizes])), "fov differs: another seed"
        ref_points = np.concatenate([bi["background_points"]] + [objects[t].points for t in objects])
        ref_rgb = np.concatenate([bi["background_RGBs"]] + [objects[t].rgbs for t in objects])
        ref_labels = np.concatenate([bi["background_sem_labels"]] + [objects[t].sem_labels for t in objects]).astype(np.int32)
        assert np.array_equal(fr.labels, ref_labels), "labels differ: another seed"
        assert R.ulp_equal(fr.points[: fr.offsets[1]], bi["background_points"])
        diffs["box_frame"] = max(diffs["box_frame"], float(np.abs(fr.points - ref_points).max()))
        diffs["rgb"] = max(diffs["rgb"], float(np.abs(fr.rgb - ref_rgb).max()))
        # what the inputs exercise
        seen["dropped"] += int((s.slot == -1).sum())
        x = pts.astype(np.float64)
        for b in np.nonzero(include)[0]:
            q = np.abs(R.apply34(lidar2box[b], x))
            inside = (q <= boxes[b, 3:6] / 2).all(1)
            seen["earlier_owner"] += int((inside & (s.slot != 1 + b) & (s.slot != 0)).sum())
        nb = int(fr.offsets[1])
        pre = f"f{f}/"
        out.update({pre + "points": pts, pre + "boxes": boxes, pre + "names": names, pre + "tokens": tokens, pre + "lidar2global": l2g,
                    pre + "lidar2imgs": mats, pre + "pose": pose, pre + "inverse": inverse, pre + "raw_sizes": raw_sizes.astype(np.int64),
                    pre + "dropped": np.int64((s.slot == -1).sum()), pre + "bg_points": ref_points[:nb], pre + "bg_rgb": ref_rgb[:nb],
                    pre + "bg_labels": ref_labels[:nb], pre + "sizes": sizes.astype(np.int64), pre + "inst_points": ref_points[nb:],
                    pre + "inst_rgb": ref_rgb[nb:], pre + "inst_labels": ref_labels[nb:]})
        infos.append(info)
        mine.append(fr)
        inputs.append((list(tokens), include, l2g))
    # ---- the traversal: accumulate_background_box_point(l2g=True) and :157-160
    frame_rgb = [i["back_instance_info"]["background_RGBs"] for i in infos]
    frame_labels = [i["back_instance_info"]["background_sem_labels"] for i in infos]
    frame_objects = [i["back_instance_info"]["instance"] for i in infos]
    background_track, instance_track = ref["accumulate_background_box_point"](infos, l2g=True)
    xyz, rgb, labels = background_track["accu_global"]
    below = labels < 10
    xyz, rgb, labels = xyz[below], rgb[below], labels[below]
    got = R.accumulate(mine, [t for t, _, _ in inputs], [i for _, i, _ in inputs], [g for _, _, g in inputs])
    assert np.array_equal(got.background[2], labels.astype(np.int32)) and 0 < below.sum() < len(below), "labels on both sides of 10"
    assert R.ulp_equal(rgb, np.concatenate([c[l < 10] for c, l in zip(frame_rgb, frame_labels)]))
    diffs["global"] = float(np.abs(got.background[0] - xyz).max())
    diffs["rgb"] = max(diffs["rgb"], float(np.abs(got.background[1] - rgb).max()))
    with_points = [t for t, tr in instance_track.items() if tr.accu_points.shape[0] > 0]
    assert list(got.instances) == with_points and len(with_points) < len(instance_track), "a track without a point"
    for t in with_points:
        parts = [o[t] for o in frame_objects if t in o]
        assert R.ulp_equal(instance_track[t].accu_points, np.concatenate([o.points for o in parts]))
        assert R.ulp_equal(instance_track[t].accu_rgbs, np.concatenate([o.rgbs for o in parts]))
        assert got.instances[t][0].shape == instance_track[t].accu_points.shape
        diffs["box_frame"] = max(diffs["box_frame"], float(np.abs(got.instances[t][0] - instance_track[t].accu_points).max()))
        diffs["rgb"] = max(diffs["rgb"], float(np.abs(got.instances[t][1] - instance_track[t].accu_rgbs).max()))
    assert seen["dropped"] > 0 and seen["earlier_owner"] > 0, seen
    assert any(n in R.SKIP_CLASSES for n in all_names) and "track04" in with_points and "track20" not in with_points
    assert diffs["box_frame"] < 1e-12 and diffs["rgb"] < 1e-10 and diffs["global"] < 1e-8, diffs
    out.update({"stack/xyz": xyz, "stack/labels": labels.astype(np.int32), "stack/tokens": np.array(with_points),
                "stack/sizes": np.array([instance_track[t].accu_points.shape[0] for t in with_points], dtype=np.int64),
                "box_frame_max_diff": np.float64(diffs["box_frame"]), "rgb_max_diff": np.float64(diffs["rgb"]),
                "global_max_diff": np.float64(diffs["global"])})
    path = Path(__file__).resolve().parent / "stack_ref.npz"
    np.savez_compressed(path, **out)
    print(f"{FRAMES} frames of {N_FRAME} points, {N_BOXES} tracks: dropped {seen['dropped']}, owned by an earlier box {seen['earlier_owner']}, "
          f"background {len(xyz)} rows, {len(with_points)} tracks with points; max diffs {diffs}; {path.stat().st_size} bytes")


if __name__ == "__main__":
    main()
