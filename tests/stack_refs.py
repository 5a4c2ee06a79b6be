"""The rule and the arithmetic of include/mtgs_stack.h restated in NumPy, in exactly their operation order: every product and sum is
an element-wise fp64 operation of its own (no matmul, so no BLAS summation order).  `split_sweep` is the per-point rule of
extract_frame_background_instance_lidar, `stack_frame` the per-frame painting and field-of-view filter of
stack_RGB_point_cloud.py:93-126 (with tests/lidar_refs.paint_points), `accumulate` the traversal of
accumulate_background_box_point and :157-160.  tests/golden/make_stack_golden.py checks this restatement against the reference's own
functions and records the result in tests/golden/stack_ref.npz; tests/test_stack_host.py checks it against that record and
tests/test_gpu_stack.py checks the kernels against it, bit for bit."""
from pathlib import Path
from typing import Dict, NamedTuple

import numpy as np

from tests import lidar_refs

GOLDEN = Path(__file__).resolve().parent / "golden" / "stack_ref.npz"
SKIP_CLASSES = ("traffic_cone", "barrier", "czone_sign")


class Split(NamedTuple):
    points: np.ndarray      # float64 [N, 3]: background rows, box-frame rows of box 0, 1, ..., zeros for the dropped
    offsets: np.ndarray     # int64 [B + 2]
    slot: np.ndarray        # int32 [N]: 0 background, 1 + b, -1 dropped


class Frame(NamedTuple):
    points: np.ndarray      # float64 [M, 3]: the rows some camera sees; background in the lidar frame, instances in the box frame
    rgb: np.ndarray
    labels: np.ndarray      # int32 [M]
    offsets: np.ndarray     # int64 [B + 2]
    slot: np.ndarray


class Stacked(NamedTuple):
    background: tuple       # (xyz, rgb, labels)
    instances: Dict[str, tuple]


def _f64(a):
    return np.asarray(a).astype(np.float64)


def apply34(m, x):
    """rows 0..2 of m applied to the points x [N, 3]: ((m_k0 x + m_k1 y) + m_k2 z) + m_k3"""
    return np.stack([lidar_refs.row34(m[k], x) for k in range(3)], -1)


def split_sweep(points, boxes, lidar2box, include=None, fill_scale=0.25) -> Split:
    x, boxes = _f64(points).reshape(-1, 3), _f64(boxes).reshape(-1, 7)
    N, B = x.shape[0], boxes.shape[0]
    tight, inflated = boxes[:, 3:6] / 2, (boxes[:, 3:6] + fill_scale) / 2
    slot = np.zeros(N, dtype=np.int32)
    q = np.zeros((N, 3))
    free = np.ones(N, dtype=bool)
    with np.errstate(all="ignore"):
        for b in range(B):
            if include is not None and not include[b]:
                continue
            qb = apply34(_f64(lidar2box[b]), x)
            a = np.abs(qb)
            owned = free & (a[:, 0] <= inflated[b, 0]) & (a[:, 1] <= inflated[b, 1]) & (a[:, 2] <= inflated[b, 2])     # false on NaN
            inside = owned & (a[:, 0] <= tight[b, 0]) & (a[:, 1] <= tight[b, 1]) & (a[:, 2] <= tight[b, 2])
            slot[owned] = -1
            slot[inside] = 1 + b
            q[inside] = qb[inside]
            free &= ~owned
    groups = [np.nonzero(slot == g)[0] for g in range(B + 1)]
    offsets = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int64)
    out = np.zeros((N, 3))
    out[:offsets[1]] = x[groups[0]]
    if B:
        order = np.concatenate(groups[1:])
        out[offsets[1]:offsets[-1]] = q[order]
    return Split(out, offsets, slot)


def stack_frame(points, boxes, lidar2box, box2lidar, include, lidar2imgs, images, sem_masks, channel_order="bgr", fill_scale=0.25) -> Frame:
    s = split_sweep(points, boxes, lidar2box, include, fill_scale)
    B, kept = len(s.offsets) - 2, int(s.offsets[-1])
    rows = s.points[:kept]
    group = np.repeat(np.arange(B + 1), np.diff(s.offsets))
    paint = rows.copy()
    for b in range(B):                                    # InstanceObject.points_ego: the reference paints the round-tripped point
        sel = group == 1 + b
        if sel.any():
            paint[sel] = apply34(_f64(box2lidar[b]), rows[sel])
    p = lidar_refs.paint_points(paint, lidar2imgs, images, sem_masks, channel_order)
    keep = p.fov
    offsets = np.concatenate([[0], np.cumsum(np.bincount(group[keep], minlength=B + 1))]).astype(np.int64)
    return Frame(rows[keep], p.rgb[keep], p.labels[keep].astype(np.int32), offsets, s.slot)


def accumulate(frames, tokens, includes, lidar2globals, label_cutoff=10) -> Stacked:
    """frames: Frame per frame in frame order; tokens[f][b], includes[f][b] per box; lidar2globals[f] [4, 4] or [3, 4]"""
    xyz, rgb, labels = [np.zeros((0, 3))], [np.zeros((0, 3))], [np.zeros(0, np.int32)]
    tracks: Dict[str, list] = {}
    for fr, toks, inc, g in zip(frames, tokens, includes, lidar2globals):
        n = int(fr.offsets[1])
        keep = fr.labels[:n] < label_cutoff
        xyz.append(apply34(_f64(g), fr.points[:n][keep]))
        rgb.append(fr.rgb[:n][keep])
        labels.append(fr.labels[:n][keep])
        for b, token in enumerate(toks):
            if inc[b]:
                a, e = int(fr.offsets[1 + b]), int(fr.offsets[2 + b])
                tracks.setdefault(token, []).append((fr.points[a:e], fr.rgb[a:e]))
    instances = {}
    for token, parts in tracks.items():
        pts = np.concatenate([p for p, _ in parts])
        if len(pts):
            instances[token] = (pts, np.concatenate([c for _, c in parts]))
    return Stacked((np.concatenate(xyz), np.concatenate(rgb), np.concatenate(labels)), instances)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def boxes_on_the_ring(rng, n_boxes):
    """n_boxes [n, 7] of car size, 5 to 28 m from the sensor; box 1 overlaps box 0 and box 3 stands inside the margin of box 2 (its
    near face 0.1 m from that one's), so points of the later box belong to the earlier one or are dropped"""
    r, a = rng.uniform(5.0, 28.0, n_boxes), rng.uniform(0.0, 2 * np.pi, n_boxes)
    b = np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(0.0, 1.0, n_boxes), rng.uniform(3.0, 5.0, n_boxes), rng.uniform(1.5, 2.2, n_boxes),
                  rng.uniform(1.4, 2.0, n_boxes), rng.uniform(-np.pi, np.pi, n_boxes)], -1)
    if n_boxes >= 2:
        b[1] = b[0]
        b[1, 0] += 1.0
    if n_boxes >= 4:
        b[3] = b[2]
        c, s = np.cos(b[2, 6]), np.sin(b[2, 6])
        b[3, 0] += (b[2, 4] + 0.1) * -s                   # along the box's y axis: one width and 0.1 m
        b[3, 1] += (b[2, 4] + 0.1) * c
    return b


def sweep_with_boxes(rng, n, boxes, per_box=12):
    """n float32 points: a ring (tests/lidar_refs.sweep) with per_box points per box spread over the box, its margin and 0.3 m around
    it, at random places of the sweep"""
    pts = lidar_refs.sweep(rng, n).astype(np.float64)
    k = min(per_box, n)
    for b in boxes if k else ():
        c, s = np.cos(b[6]), np.sin(b[6])
        local = rng.uniform(-1.0, 1.0, (k, 3)) * (b[3:6] / 2 + 0.3)
        where = rng.choice(n, k, replace=False)
        pts[where] = np.stack([c * local[:, 0] - s * local[:, 1] + b[0], s * local[:, 0] + c * local[:, 1] + b[1], local[:, 2] + b[2]], -1)
    return pts.astype(np.float32)


def lidar2global(rng, step):
    """a sensor pose far from the origin (UTM-like coordinates), `step` frames along a gentle curve"""
    yaw = 0.3 + 0.05 * step
    g = np.eye(4)
    g[:3, :3] = [[np.cos(yaw), -np.sin(yaw), 0.0], [np.sin(yaw), np.cos(yaw), 0.0], [0.0, 0.0, 1.0]]
    g[:3, 3] = [664430.0 + 4.0 * step, 3997650.0 + 1.5 * step, 606.0 + rng.uniform(-0.1, 0.1)]
    return g


def ulp_equal(a, b):
    """bit for bit: two float arrays as integers (so that -0.0 != 0.0 and NaN payloads count)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(f"i{a.dtype.itemsize}"), b.view(f"i{b.dtype.itemsize}"))


def golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def golden_frames(g):
    """the three frames of the record as dictionaries: points, boxes, names, tokens, lidar2global, lidar2imgs and the reference's results"""
    return [{k[3:]: v for k, v in g.items() if k.startswith(f"f{f}/")} for f in range(3)]


def check_against_golden(g, frames, stacked):
    """`frames` (Frame per frame) and `stacked` (Stacked) against what the reference's own functions gave: every decision exactly
    (group sizes and order, fov, labels, the background's lidar-frame rows bit for bit), coordinates and colours within the recorded
    largest differences, with no margin added.  Returns the measured maxima."""
    seen = {"box_frame": 0.0, "rgb": 0.0, "global": 0.0}
    worst = lambda key, a, b: seen.__setitem__(key, max(seen[key], float(np.abs(a - b).max()) if len(a) else 0.0))
    cut = []
    for fr, want in zip(frames, golden_frames(g)):
        B = len(want["boxes"])
        assert np.array_equal(np.bincount(fr.slot[fr.slot >= 0], minlength=B + 1), want["raw_sizes"]) and (fr.slot == -1).sum() == want["dropped"]
        assert np.array_equal(np.diff(fr.offsets), np.concatenate([[len(want["bg_points"])], want["sizes"]]))
        nb, end = int(fr.offsets[1]), int(fr.offsets[-1])
        assert ulp_equal(fr.points[:nb], want["bg_points"])
        assert np.array_equal(fr.labels[:end], np.concatenate([want["bg_labels"], want["inst_labels"]])) and fr.labels.dtype == np.int32
        worst("box_frame", fr.points[nb:end], want["inst_points"])
        worst("rgb", fr.rgb[:end], np.concatenate([want["bg_rgb"], want["inst_rgb"]]))
        cut.append(want["bg_labels"] < 10)
    xyz, rgb, labels = stacked.background
    assert np.array_equal(labels, g["stack/labels"]) and xyz.shape == g["stack/xyz"].shape and len(xyz) == sum(int(c.sum()) for c in cut)
    worst("global", xyz, g["stack/xyz"])
    worst("rgb", rgb, np.concatenate([w["bg_rgb"][c] for w, c in zip(golden_frames(g), cut)]))
    assert list(stacked.instances) == list(g["stack/tokens"])
    for token, size in zip(g["stack/tokens"], g["stack/sizes"]):
        parts = [(w["inst_points"], w["inst_rgb"], np.concatenate([[0], np.cumsum(w["sizes"])]), list(w["tokens"])) for w in golden_frames(g)]
        pts = np.concatenate([p[o[t.index(token)]:o[t.index(token) + 1]] for p, _, o, t in parts if token in t])
        col = np.concatenate([c[o[t.index(token)]:o[t.index(token) + 1]] for _, c, o, t in parts if token in t])
        assert stacked.instances[token][0].shape == (size, 3) == pts.shape
        worst("box_frame", stacked.instances[token][0], pts)
        worst("rgb", stacked.instances[token][1], col)
    assert seen["box_frame"] <= float(g["box_frame_max_diff"]) and seen["rgb"] <= float(g["rgb_max_diff"]), seen
    assert seen["global"] <= float(g["global_max_diff"]), seen
    return seen
