"""Stacking lidar sweeps (mtgs_amd/stack.py, csrc/stack.hip, include/mtgs_stack.h) without a GPU: the NumPy restatement of
tests/stack_refs.py against what the reference's own functions gave (tests/golden/stack_ref.npz), `box_matrices` against the
reference's pose and inverse, the header as a group of its own, the host checks of the C entry points, and what the Python layer
refuses before it touches a device."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from mtgs_amd import stack as S
from tests import stack_refs as R

ROOT = Path(__file__).resolve().parents[1]
NAMES = ["mtgs_stack_frame", "mtgs_stack_frame_workspace_bytes", "mtgs_stack_gather", "mtgs_stack_plan", "mtgs_stack_plan_workspace_bytes",
         "mtgs_stack_split", "mtgs_stack_split_workspace_bytes"]


def restated(g):
    frames = []
    for fr in R.golden_frames(g):
        include = np.array([n not in R.SKIP_CLASSES for n in fr["names"]])
        lidar2box, box2lidar, _ = S.box_matrices(fr["boxes"])
        frames.append(R.stack_frame(fr["points"], fr["boxes"], lidar2box, box2lidar, include, fr["lidar2imgs"], g["images"], g["masks"], "bgr"))
    gf = R.golden_frames(g)
    includes = [np.array([n not in R.SKIP_CLASSES for n in fr["names"]]) for fr in gf]
    return frames, R.accumulate(frames, [list(fr["tokens"]) for fr in gf], includes, [fr["lidar2global"] for fr in gf])


# ---- the restatement against the reference's recorded outputs -----------------------------------------------------------------------
def test_the_restatement_stacks_what_the_reference_stacked():
    """Decisions exactly; coordinates and colours within the largest differences the maker recorded (the reference's matrix products
    sum in an order of their own), with no margin added."""
    g = R.golden()
    assert R.GOLDEN.stat().st_size <= (ROOT / "tests" / "golden" / "lidar_ref.npz").stat().st_size
    assert sum(len(fr["points"]) for fr in R.golden_frames(g)) <= 6000 and max(len(fr["boxes"]) for fr in R.golden_frames(g)) <= 24
    assert g["images"].shape == (3, 37, 53, 3) and g["masks"].shape == (3, 37, 53, 1)
    frames, stacked = restated(g)
    seen = R.check_against_golden(g, frames, stacked)
    print(f"restatement against the reference: {seen}; recorded box frame {float(g['box_frame_max_diff']):.3g}, rgb "
          f"{float(g['rgb_max_diff']):.3g}, global {float(g['global_max_diff']):.3g}")
    assert float(g["box_frame_max_diff"]) < 1e-12 and float(g["rgb_max_diff"]) < 1e-10 and float(g["global_max_diff"]) < 1e-8


def test_the_record_exercises_the_rule():
    g = R.golden()
    gf = R.golden_frames(g)
    assert sum(int(fr["dropped"]) for fr in gf) > 0                                                      # dropped in a margin
    assert any(n in R.SKIP_CLASSES for fr in gf for n in fr["names"])                                      # a skipped class
    assert "track04" in gf[0]["tokens"] and "track04" not in gf[1]["tokens"] and "track04" in g["stack/tokens"]   # absent from a frame
    assert "track20" in gf[0]["tokens"] and "track20" not in g["stack/tokens"]                          # a track without a point
    labels = np.concatenate([fr["bg_labels"] for fr in gf])
    assert (labels < 10).any() and (labels >= 10).any()
    owned_earlier = 0
    for fr in gf:
        include = np.array([n not in R.SKIP_CLASSES for n in fr["names"]])
        lidar2box = S.box_matrices(fr["boxes"])[0]
        slot = R.split_sweep(fr["points"], fr["boxes"], lidar2box, include).slot
        for b in np.nonzero(include)[0]:
            inside = (np.abs(R.apply34(lidar2box[b], fr["points"].astype(np.float64))) <= fr["boxes"][b, 3:6] / 2).all(1)
            owned_earlier += int((inside & (slot != 1 + b) & (slot != 0)).sum())
    assert owned_earlier > 0                                                                            # inside a later box, owned by an earlier one


def test_box_matrices_are_the_references_pose_and_inverse():
    g = R.golden()
    for fr in R.golden_frames(g):
        lidar2box, box2lidar, half = S.box_matrices(fr["boxes"])
        include = np.array([n not in R.SKIP_CLASSES for n in fr["names"]])
        assert include.sum() < len(include) and np.isnan(fr["pose"][~include]).all()
        assert R.ulp_equal(box2lidar[include], fr["pose"][include]) and R.ulp_equal(lidar2box[include], fr["inverse"][include])
        assert R.ulp_equal(half, fr["boxes"][:, 3:6] / 2)
    lidar2box, box2lidar, half = S.box_matrices(np.zeros((0, 7)))
    assert lidar2box.shape == box2lidar.shape == (0, 4, 4) and half.shape == (0, 3)
    one = S.box_matrices(torch.tensor([[1.0, 2.0, 3.0, 4.0, 2.0, 1.5, 0.0]]))
    assert np.array_equal(one[1][0], [[1, 0, 0, 1], [0, 1, 0, 2], [0, 0, 1, 3], [0, 0, 0, 1]]) and np.array_equal(one[2], [[2.0, 1.0, 0.75]])


def test_the_restated_rule_on_hand_made_points():
    """the first box whose inflated test holds owns the point; tight -> instance, margin -> dropped and never a later box's"""
    boxes = np.array([[0.0, 0, 0, 4, 2, 2, 0], [2.0, 0, 0, 4, 2, 2, 0], [20.0, 0, 0, 2, 2, 2, 0]])
    m = S.box_matrices(boxes)[0]
    pts = np.array([[1.5, 0, 0],           # in both 0 and 1: box 0
                    [2.1, 0, 0],           # in the margin of 0, inside 1: dropped
                    [3.0, 0, 0],           # outside the margin of 0 (|x| <= 2.125), inside 1
                    [2.0, 0, 0],           # exactly on the tight face of 0
                    [2.125, 0, 0],         # exactly on the inflated face of 0: dropped
                    [np.nan, 0, 0], [0, np.inf, 0], [50.0, 0, 0],
                    [20.5, 0.5, -1.0]])
    s = R.split_sweep(pts, boxes, m)
    assert list(s.slot) == [1, -1, 2, 1, -1, 0, 0, 0, 3] and list(s.offsets) == [0, 3, 5, 6, 7]
    assert np.array_equal(s.points[3:7], [[1.5, 0, 0], [2.0, 0, 0], [1.0, 0, 0], [0.5, 0.5, -1.0]]) and not s.points[7:].any()
    assert np.isnan(s.points[0, 0]) and np.isinf(s.points[1, 1]) and s.points[2, 0] == 50.0
    skip0 = R.split_sweep(pts, boxes, m, include=[False, True, True])
    assert list(skip0.slot) == [2, 2, 2, 2, 2, 0, 0, 0, 3]
    assert list(R.split_sweep(pts, boxes[:0], m[:0]).slot) == [0] * 9 and list(R.split_sweep(pts[:0], boxes, m).offsets) == [0] * 5


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_the_header_is_declared_bound_and_exported():
    from mtgs_amd import _abi, _lib, build
    assert sorted(_lib.GROUPS["mtgs_stack.h"]) == NAMES
    abi = _abi.header_abi("mtgs_stack.h")
    assert S.MAX_BOXES == abi.constants["MTGS_STACK_MAX_BOXES"] == 1024 and S.BOX_CHUNK == abi.constants["MTGS_STACK_BOX_CHUNK"] == 64
    assert abi.structs["mtgs_stack_frame_desc"].itemsize == 152
    assert build.PER_FILE_FLAGS["stack.hip"] == ["-ffp-contract=off"]
    assert _abi.constant("MTGS_RAST_ABI_VERSION") == 29 and _abi.constant("MTGS_RAST_HOT_ABI_VERSION") == 7


def test_the_host_checks_name_the_bad_argument(hip_lib):
    size = C.c_size_t(0)
    buf = (C.c_double * 64)()                # stands for every pointer: each call below fails a check, nothing is launched
    split = dict(N=4, points=buf, f64=1, stride=3, B=1, l2b=buf, tight=buf, infl=buf, include=None, out=buf, offsets=buf, slot=None, ws=buf,
                 ws_bytes=0, stream=None)
    frame = dict(N=4, points=buf, f64=1, stride=3, B=1, l2b=buf, b2l=buf, tight=buf, infl=buf, include=None, C=1, mats=buf, h=4, w=4, images=buf,
                 reverse=1, masks=buf, cutoff=10, out=buf, rgb=buf, labels=buf, offsets=buf, bg_sel=buf, bg_kept=buf, slot=None, ws=buf,
                 ws_bytes=0, stream=None)
    plan = dict(S=2, seg_frame=buf, seg_slot=buf, F=1, frames=buf, prefix=buf, ws=buf, ws_bytes=0, stream=None)
    gather = dict(S=2, seg_frame=buf, seg_slot=buf, F=1, frames=buf, prefix=buf, total=5, xyz=buf, rgb=buf, labels=buf, stream=None)
    s = lambda **kw: hip_lib.mtgs_stack_split(*(split | kw).values())
    f = lambda **kw: hip_lib.mtgs_stack_frame(*(frame | kw).values())
    p = lambda **kw: hip_lib.mtgs_stack_plan(*(plan | kw).values())
    g = lambda **kw: hip_lib.mtgs_stack_gather(*(gather | kw).values())
    sizes = hip_lib.mtgs_stack_split_workspace_bytes
    for refused, message in ((lambda: sizes(-1, 1, C.byref(size)), r"N outside \[0, 2\^31\) \(-1\)"),
                             (lambda: sizes(4, 1025, C.byref(size)), r"B outside \[0, 1024\] \(1025\)"),
                             (lambda: sizes(4, 1, None), r"null pointer: bytes"),
                             (lambda: hip_lib.mtgs_stack_frame_workspace_bytes(4, -1, C.byref(size)), r"B outside \[0, 1024\] \(-1\)"),
                             (lambda: hip_lib.mtgs_stack_plan_workspace_bytes(-2, C.byref(size)), r"S outside"),
                             (lambda: s(N=1 << 31), r"N outside"), (lambda: s(B=2000), r"B outside"),
                             (lambda: s(points=None), r"null pointer: points"), (lambda: s(stride=2), r"row_stride < 3 \(2\)"),
                             (lambda: s(l2b=None), r"null pointer: lidar2box"), (lambda: s(tight=None), r"null pointer: half_tight"),
                             (lambda: s(infl=None), r"null pointer: half_inflated"), (lambda: s(ws=None), r"null pointer: ws"),
                             (lambda: s(offsets=None), r"null pointer: offsets"), (lambda: s(), r"mtgs_stack_split: workspace 0 < \d+ bytes"),
                             (lambda: f(N=-1), r"N outside"), (lambda: f(b2l=None), r"null pointer: box2lidar"),
                             (lambda: f(mats=None), r"null pointer: lidar2imgs"), (lambda: f(images=None), r"null pointer: images"),
                             (lambda: f(masks=None), r"null pointer: masks"), (lambda: f(offsets=None), r"null pointer: out_offsets"),
                             (lambda: f(bg_kept=None), r"null pointer: bg_kept"), (lambda: f(), r"mtgs_stack_frame: workspace 0 < \d+ bytes"),
                             (lambda: p(S=-1), r"S outside"), (lambda: p(F=-1), r"F outside"), (lambda: p(prefix=None), r"null pointer: prefix"),
                             (lambda: p(seg_frame=None), r"null pointer: seg_frame"), (lambda: p(frames=None), r"null pointer: frames"),
                             (lambda: p(), r"mtgs_stack_plan: workspace 0 < \d+ bytes"),
                             (lambda: g(total=-1), r"total outside"), (lambda: g(S=0), r"total > 0 without a segment"),
                             (lambda: g(prefix=None), r"null pointer: prefix"), (lambda: g(xyz=None), r"null pointer: xyz"),
                             (lambda: g(labels=None), r"null pointer: labels")):
        assert refused() != 0 and re.search(message, hip_lib.mtgs_rast_last_error().decode()), (message, hip_lib.mtgs_rast_last_error())
    assert g(total=0, prefix=None) == 0                                          # nothing to gather is no error
    small, large = C.c_size_t(0), C.c_size_t(0)
    assert sizes(0, 0, C.byref(small)) == 0 and sizes(100000, 1024, C.byref(large)) == 0 and 0 < small.value < large.value
    assert hip_lib.mtgs_stack_frame_workspace_bytes(100000, 64, C.byref(size)) == 0 and size.value > large.value


# ---- what the Python layer refuses ---------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_by_name():
    pts = torch.zeros(5, 3)
    boxes = np.array([[0.0, 0, 0, 4, 2, 2, 0]])
    for kw, message in ((dict(points=torch.zeros(5, 4)), r"points must be \[N, 3\], got \(5, 4\)"),
                        (dict(boxes=np.zeros((2, 6))), r"boxes must be \[B, 7\] numbers .* got \(2, 6\)"),
                        (dict(boxes=np.zeros((1025, 7))), r"at most 1024 boxes, got \(1025, 7\)"),
                        (dict(boxes=np.array([[np.nan, 0, 0, 4, 2, 2, 0]])), "boxes must be finite"),
                        (dict(include=[True, False]), r"include must be \[B\] with B = 1, got \(2,\)"),
                        (dict(fill_scale=-1.0), "fill_scale must be a number >= 0, got -1.0")):
        with pytest.raises(ValueError, match=message):
            S.split_sweep(**(dict(points=pts, boxes=boxes) | kw))
    with pytest.raises(TypeError, match="float32 or float64"):
        S.split_sweep(pts.to(torch.float16), boxes)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.split_sweep(pts, boxes)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.upload_boxes(boxes, device="cpu")
    with pytest.raises(ValueError, match="label_cutoff must be an integer, got 9.5"):
        S.SweepStack(label_cutoff=9.5)
    with pytest.raises(ValueError, match="fill_scale must be a number >= 0"):
        S.SweepStack(fill_scale="a")
    stack = S.SweepStack()
    frame = dict(points=pts, boxes=boxes, names=["vehicle"], track_tokens=["a"], lidar2global=np.eye(4), lidar2imgs=torch.eye(4)[None],
                 images=torch.zeros(1, 8, 9, 3, dtype=torch.uint8), sem_masks=torch.zeros(1, 8, 9, 1, dtype=torch.uint8))
    for kw, message in ((dict(names=[]), r"one entry per box \(1\), got 0 and 1"),
                        (dict(boxes=np.zeros((2, 7)), names=["vehicle"] * 2, track_tokens=["a", "a"]), "track_tokens must be unique within a frame"),
                        (dict(lidar2global=np.eye(3)), r"lidar2global must be a float \[4, 4\] or \[3, 4\], got \(3, 3\)"),
                        (dict(points=torch.zeros(3)), r"points must be \[N, 3\]")):
        with pytest.raises(ValueError, match=message):
            stack.add_frame(**(frame | kw))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        stack.add_frame(**frame)
    assert len(stack) == 0
    table = S.BoxTable(*(torch.zeros(1, n, dtype=torch.float64) for n in (12, 12, 3, 3)), torch.ones(1, dtype=torch.uint8))
    cams = dict(points=pts, table=table, lidar2imgs=frame["lidar2imgs"], images=frame["images"], sem_masks=frame["sem_masks"])
    for kw, message in ((dict(lidar2imgs=torch.eye(4)), r"lidar2imgs must be \[C, 4, 4\] or \[C, 3, 4\], got \(4, 4\)"),
                        (dict(images=torch.zeros(2, 8, 9, 3, dtype=torch.uint8)), r"images must be \[C, H, W, 3\] with C = 1, got \(2, 8, 9, 3\)"),
                        (dict(sem_masks=torch.zeros(1, 9, 8, dtype=torch.uint8)), r"sem_masks must be .* the images' size 8 x 9, got \(1, 9, 8\)"),
                        (dict(channel_order="gbr"), "channel_order must be 'bgr' or 'rgb', got 'gbr'"),
                        (dict(label_cutoff=True), "label_cutoff must be an integer, got True")):
        with pytest.raises(ValueError, match=message):
            S.stack_frame(**(cams | kw))
    with pytest.raises(TypeError, match="must be uint8"):
        S.stack_frame(**(cams | dict(images=frame["images"].float())))
    with pytest.raises(TypeError, match="table must be a BoxTable"):
        S.stack_frame(**(cams | dict(table=boxes)))


def test_the_public_surface():
    import mtgs_amd
    assert mtgs_amd.split_sweep is S.split_sweep and mtgs_amd.box_matrices is S.box_matrices and mtgs_amd.SweepStack is S.SweepStack
    assert {"split_sweep", "box_matrices", "SweepStack", "SplitSweep", "StackedClouds"} <= set(mtgs_amd.__all__)
    s = inspect.signature(S.split_sweep).parameters
    assert list(s) == ["points", "boxes", "include", "fill_scale"] and (s["include"].default, s["fill_scale"].default) == (None, 0.25)
    s = inspect.signature(S.SweepStack.__init__).parameters
    assert list(s) == ["self", "fill_scale", "label_cutoff", "skip_classes"]
    assert (s["fill_scale"].default, s["label_cutoff"].default, s["skip_classes"].default) == (0.25, 10, ("traffic_cone", "barrier", "czone_sign"))
    s = inspect.signature(S.SweepStack.add_frame).parameters
    assert list(s) == ["self", "points", "boxes", "names", "track_tokens", "lidar2global", "lidar2imgs", "images", "sem_masks", "channel_order"]
    assert s["channel_order"].default == "bgr"
    assert S.SplitSweep._fields == ("points", "offsets", "slot") and S.StackedClouds._fields == ("background", "instances")
