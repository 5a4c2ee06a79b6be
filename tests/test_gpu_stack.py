"""mtgs_amd.stack on the device against the NumPy restatement of tests/stack_refs.py, BIT FOR BIT (floats compared as integers): the
slot of every point, the group offsets, the background rows, the box-frame rows, the colours, the labels and the stacked clouds; and,
for the recorded traversal, against what the reference's own functions gave under the bounds of tests/test_stack_host.py.  Shapes
are small: N up to a few thousand (one size above the 1024-row tile of the radix sort and the 2048-row tile of the scan), B up to
MAX_BOXES, three cameras of 37 x 53."""
import numpy as np
import pytest
import torch

from mtgs_amd import stack as S
from tests import lidar_refs
from tests import stack_refs as R

pytestmark = pytest.mark.gpu
H, W = 37, 53


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def host(t):
    return t.cpu().numpy()


def check_split(points, boxes, include=None, fill_scale=0.25, make=dev, what="split"):
    """split_sweep on the device against the restatement with the same matrices; `points` and `boxes` are NumPy arrays"""
    got = S.split_sweep(make(points), boxes, include, fill_scale)
    torch.cuda.synchronize()
    want = R.split_sweep(points, boxes, S.box_matrices(boxes)[0], include, fill_scale)
    n, B = len(points), len(boxes)
    pts, offsets, slot = host(got.points), host(got.offsets), host(got.slot)
    assert pts.dtype == np.float64 and pts.shape == (n, 3) and offsets.dtype == np.int64 and offsets.shape == (B + 2,) and slot.dtype == np.int32
    print(f"{what}: N={n} B={B} background {want.offsets[1]} in boxes {want.offsets[-1] - want.offsets[1]} dropped {n - want.offsets[-1]}, "
          f"bitwise equal: {R.ulp_equal(pts, want.points)}")
    assert np.array_equal(slot, want.slot) and np.array_equal(offsets, want.offsets)
    assert R.ulp_equal(pts, want.points)
    return want


def cameras(n=3, seed=6):
    rng = np.random.default_rng(seed)
    mats = np.stack([lidar_refs.camera(50.0 * c + 10.0, 30.0, rng.uniform(-0.5, 0.5, 3), W, H)[0] for c in range(n)])
    return mats, rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8), rng.integers(0, 20, (n, H, W, 1), dtype=np.uint8)


def frame_to_host(fr):
    """a FrameClouds as a tests.stack_refs.Frame, cut at the kept rows"""
    offsets = host(fr.offsets)
    end = int(offsets[-1])
    return R.Frame(host(fr.points)[:end], host(fr.rgb)[:end], host(fr.labels)[:end], offsets, host(fr.slot))


def same_frame(got: R.Frame, want: R.Frame):
    assert np.array_equal(got.slot, want.slot) and np.array_equal(got.offsets, want.offsets)
    assert np.array_equal(got.labels, want.labels) and got.labels.dtype == np.int32
    assert R.ulp_equal(got.points, want.points) and R.ulp_equal(got.rgb, want.rgb)


def same_stack(got, want: R.Stacked):
    for a, b in zip(got.background, want.background):
        assert R.ulp_equal(host(a), b)
    assert list(got.instances) == list(want.instances)
    for token, (xyz, rgb) in got.instances.items():
        assert R.ulp_equal(host(xyz), want.instances[token][0]) and R.ulp_equal(host(rgb), want.instances[token][1])


# ---- split_sweep: point and box counts ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 2500])
def test_point_and_box_counts(n):
    """every N at a wave and workgroup edge with every B at an edge of the LDS chunk (64 boxes) and at MAX_BOXES, float32 and float64"""
    assert (S.BOX_CHUNK, S.MAX_BOXES) == (64, 1024)
    for B in (0, 1, S.BOX_CHUNK - 1, S.BOX_CHUNK, S.BOX_CHUNK + 1, S.MAX_BOXES):
        rng = np.random.default_rng(1000 * n + B)
        boxes = R.boxes_on_the_ring(rng, B)
        pts = R.sweep_with_boxes(rng, n, boxes[-70:], per_box=4)            # the LAST boxes hold points: the whole table is walked
        include = rng.uniform(size=B) > 0.1
        for dtype in (np.float32, np.float64):
            want = check_split(pts.astype(dtype), boxes, include, what=f"counts {np.dtype(dtype).name}")
        if n >= 255 and B >= 63:
            assert want.offsets[-1] < n and want.offsets[-1] > want.offsets[1] > 0


def test_a_strided_view_is_read_in_place():
    rng = np.random.default_rng(2)
    boxes = R.boxes_on_the_ring(rng, 9)
    pts = R.sweep_with_boxes(rng, 700, boxes)
    for dtype in (np.float32, np.float64):
        wide = np.concatenate([pts.astype(dtype), rng.uniform(0, 255, (700, 1)).astype(dtype)], 1)      # x, y, z, intensity
        made = []

        def view(p, wide=wide):
            t = dev(wide)[:, :3]
            made.append(t)
            return t
        check_split(pts.astype(dtype), boxes, make=view, what="strided")
        assert made[0].stride() == (4, 1) and S._sweep(made[0]).data_ptr() == made[0].data_ptr()


def test_nan_and_inf_points_are_background():
    rng = np.random.default_rng(3)
    boxes = R.boxes_on_the_ring(rng, 5)
    pts = R.sweep_with_boxes(rng, 300, boxes).astype(np.float64)
    inside = R.split_sweep(pts, boxes, S.box_matrices(boxes)[0]).slot > 0
    bad = np.nonzero(inside)[0][:6]
    assert len(bad) == 6
    pts[bad[0], 0] = np.nan
    pts[bad[1], 1] = np.nan
    pts[bad[2], 2] = np.nan
    pts[bad[3], 0] = np.inf
    pts[bad[4], 1] = -np.inf
    pts[bad[5]] = np.nan
    want = check_split(pts, boxes, what="nan and inf")
    assert (want.slot[bad] == 0).all()
    check_split(pts.astype(np.float32), boxes, what="nan and inf float32")


def test_points_on_the_faces_are_inside():
    """`<=` holds on a face: exactly on the tight face an instance point, exactly on the inflated face owned (and dropped); powers of
    two throughout, so the box-frame coordinates are exact"""
    boxes = np.array([[8.0, 4.0, 1.0, 4.0, 2.0, 2.0, 0.0]])
    pts = np.array([[10.0, 4.0, 1.0], [6.0, 4.0, 1.0], [8.0, 5.0, 1.0], [8.0, 4.0, 2.0], [8.0, 4.0, 0.0],           # tight faces
                    [10.125, 4.0, 1.0], [8.0, 2.875, 1.0], [8.0, 4.0, 2.125],                                       # inflated faces
                    [np.nextafter(10.125, 11), 4.0, 1.0], [np.nextafter(10.0, 11), 4.0, 1.0]])                      # one ulp beyond each
    want = check_split(pts, boxes, what="faces")
    assert list(want.slot) == [1, 1, 1, 1, 1, -1, -1, -1, 0, -1]


def test_a_zero_size_box_and_a_zero_margin():
    boxes = np.array([[1.0, 2.0, 0.5, 0.0, 0.0, 0.0, 0.0], [16.0, 0.0, 0.0, 2.0, 2.0, 2.0, 0.0]])
    pts = np.array([[1.0, 2.0, 0.5], [1.125, 2.0, 0.5], [1.0, 2.25, 0.5], [16.0, 1.0, 0.0], [16.0, 1.0625, 0.0]])
    want = check_split(pts, boxes, what="zero size")
    assert list(want.slot) == [1, -1, 0, 2, -1]                            # its centre only; the margin is 0.125 wide
    want = check_split(pts, boxes, fill_scale=0.0, what="zero margin")
    assert list(want.slot) == [1, 0, 0, 2, 0]


def test_all_points_in_one_box_and_none_in_any():
    rng = np.random.default_rng(4)
    boxes = R.boxes_on_the_ring(rng, 6)
    boxes[4, :3], boxes[4, 3:6] = 0.0, 100.0                                   # box 4 holds the whole ring
    pts = lidar_refs.sweep(rng, 1500)
    include = np.array([False, False, False, False, True, True])
    want = check_split(pts, boxes, include, what="all in one box")
    assert (want.slot == 5).all() and list(want.offsets) == [0, 0, 0, 0, 0, 0, 1500, 1500]
    far = boxes.copy()
    far[:, 0] += 500.0
    want = check_split(pts, far, what="none in any box")
    assert (want.slot == 0).all() and R.ulp_equal(want.points, pts.astype(np.float64))


def test_identical_and_excluded_boxes():
    rng = np.random.default_rng(5)
    one = R.boxes_on_the_ring(rng, 1)
    boxes = np.concatenate([one, one, one])
    pts = R.sweep_with_boxes(rng, 400, one, per_box=60)
    want = check_split(pts, boxes, what="identical boxes")
    assert (want.slot == 1).sum() > 10 and not (want.slot > 1).any()           # the first owns the points
    want = check_split(pts, boxes, include=[False, True, True], what="an excluded box on top")
    assert (want.slot == 2).sum() > 10 and not (want.slot == 1).any() and not (want.slot == 3).any()


# ---- the traversal ---------------------------------------------------------------------------------------------------------------------
def traversal(seed=7):
    """five frames: tracks that appear and disappear, a skipped class, an empty sweep, a frame without boxes"""
    rng = np.random.default_rng(seed)
    base = R.boxes_on_the_ring(rng, 10)
    names = np.array(["vehicle"] * 10, dtype="<U16")
    names[3] = "czone_sign"
    tokens = np.array([f"t{i}" for i in range(10)])
    present = [np.arange(10) < 7, np.arange(10) >= 2, np.ones(10, bool), np.zeros(10, bool), np.arange(10) % 2 == 0]
    sizes = [900, 1100, 0, 800, 2300]
    frames = []
    for f, (keep, n) in enumerate(zip(present, sizes)):
        boxes = base[keep].copy()
        boxes[:, :2] += [0.3 * f, 0.2 * f]
        mats = cameras(3, seed=20 + f)[0]
        frames.append(dict(points=R.sweep_with_boxes(rng, n, boxes, per_box=25), boxes=boxes, names=list(names[keep]), tokens=list(tokens[keep]),
                           lidar2global=R.lidar2global(rng, f), lidar2imgs=mats))
    return frames


def run_traversal(frames, images, masks, dtype=np.float32):
    stack = S.SweepStack()
    outs = [stack.add_frame(dev(fr["points"].astype(dtype)), fr["boxes"], fr["names"], fr["tokens"], fr["lidar2global"], dev(fr["lidar2imgs"]),
                            dev(images), dev(masks)) for fr in frames]
    clouds = stack.finish()
    torch.cuda.synchronize()
    return outs, clouds


def restate_traversal(frames, images, masks, dtype=np.float32):
    mine, includes = [], []
    for fr in frames:
        include = np.array([n not in R.SKIP_CLASSES for n in fr["names"]], dtype=bool)
        lidar2box, box2lidar, _ = S.box_matrices(fr["boxes"])
        mine.append(R.stack_frame(fr["points"].astype(dtype), fr["boxes"], lidar2box, box2lidar, include, fr["lidar2imgs"], images, masks, "bgr"))
        includes.append(include)
    return mine, R.accumulate(mine, [fr["tokens"] for fr in frames], includes, [fr["lidar2global"] for fr in frames])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_traversal_against_the_restatement(dtype):
    frames = traversal()
    _, images, masks = cameras(3)
    outs, clouds = run_traversal(frames, images, masks, dtype)
    mine, want = restate_traversal(frames, images, masks, dtype)
    for got, w in zip(outs, mine):
        same_frame(frame_to_host(got), w)
    same_stack(clouds, want)
    xyz, rgb, labels = clouds.background
    print(f"traversal {np.dtype(dtype).name}: background {len(xyz)} rows, tracks {[(t, len(v[0])) for t, v in clouds.instances.items()]}")
    assert xyz.dtype == rgb.dtype == torch.float64 and labels.dtype == torch.int32 and len(xyz) > 500 and int(labels.max()) < 10
    assert "t3" not in clouds.instances and 3 <= len(clouds.instances) <= 9                      # the skipped class has no cloud
    assert any((fr.labels >= 10).any() for fr in mine) and sum(int((fr.slot == -1).sum()) for fr in mine) > 0
    # the same calls again give the same bytes
    outs2, clouds2 = run_traversal(frames, images, masks, dtype)
    for a, b in zip(outs, outs2):
        same_frame(frame_to_host(a), frame_to_host(b))
    same_stack(clouds2, R.Stacked(tuple(host(t) for t in clouds.background), {k: (host(a), host(b)) for k, (a, b) in clouds.instances.items()}))


def test_an_empty_traversal_and_empty_frames():
    _, images, masks = cameras(1)
    mats = dev(cameras(1)[0])
    empty = S.SweepStack().finish()
    assert empty.background[0].shape == (0, 3) and empty.background[2].shape == (0,) and empty.instances == {}
    stack = S.SweepStack()
    for _ in range(2):
        fr = stack.add_frame(torch.zeros((0, 3), device="cuda"), np.zeros((0, 7)), [], [], np.eye(4), mats, dev(images), dev(masks))
        assert host(fr.offsets).tolist() == [0, 0] and int(fr.bg_kept) == 0
    fr = stack.add_frame(torch.zeros((0, 3), device="cuda"), R.boxes_on_the_ring(np.random.default_rng(0), 3), ["vehicle"] * 3, ["a", "b", "c"],
                         np.eye(4), mats, dev(images), dev(masks))
    assert host(fr.offsets).tolist() == [0] * 5
    clouds = stack.finish()
    torch.cuda.synchronize()
    assert clouds.background[0].shape == (0, 3) and clouds.instances == {}


def test_the_clouds_seed_the_next_stage():
    """StackedClouds goes into pointcloud.prepare_seed_cloud as it is"""
    import mtgs_amd
    frames = traversal(seed=9)
    _, images, masks = cameras(3)
    _, clouds = run_traversal(frames, images, masks)
    xyz, rgb, _ = clouds.background
    cloud = mtgs_amd.prepare_seed_cloud(xyz, rgb, voxel_size=0.5)
    torch.cuda.synchronize()
    assert cloud["xyz"].dtype == torch.float32 and cloud["rgb"].dtype == torch.uint8 and 0 < cloud["xyz"].shape[0] == cloud["rgb"].shape[0]


# ---- the recorded traversal: the reference's own outputs ---------------------------------------------------------------------------------
def test_golden_traversal():
    g = R.golden()
    frames = [dict(points=fr["points"], boxes=fr["boxes"], names=list(fr["names"]), tokens=list(fr["tokens"]), lidar2global=fr["lidar2global"],
                   lidar2imgs=fr["lidar2imgs"]) for fr in R.golden_frames(g)]
    outs, clouds = run_traversal(frames, g["images"], g["masks"])
    got = [frame_to_host(o) for o in outs]
    stacked = R.Stacked(tuple(host(t) for t in clouds.background), {k: (host(a), host(b)) for k, (a, b) in clouds.instances.items()})
    seen = R.check_against_golden(g, got, stacked)
    print(f"golden traversal on the device: {seen}")
    mine, want = restate_traversal(frames, g["images"], g["masks"])
    for a, b in zip(got, mine):
        same_frame(a, b)
    same_stack(clouds, want)


# ---- HIP graph -------------------------------------------------------------------------------------------------------------------------
def test_a_captured_frame_replays_the_eager_bytes():
    rng = np.random.default_rng(11)
    boxes = R.boxes_on_the_ring(rng, 12)
    pts, other = dev(R.sweep_with_boxes(rng, 3000, boxes, per_box=30)), dev(R.sweep_with_boxes(rng, 3000, boxes, per_box=30))
    mats, images, masks = (dev(a) for a in cameras(3))
    table = S.upload_boxes(boxes)
    run = lambda p: S.stack_frame(p, table, mats, images, masks)
    first, second, want_other = frame_to_host(run(pts)), frame_to_host(run(pts)), frame_to_host(run(other))
    torch.cuda.synchronize()
    same_frame(first, second)
    assert not np.array_equal(first.slot, want_other.slot)
    static = pts.clone()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        run(static)
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = run(static)
    for points, want in ((other, want_other), (pts, first), (pts, first)):
        static.copy_(points)
        for o in out:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        same_frame(frame_to_host(out), want)
