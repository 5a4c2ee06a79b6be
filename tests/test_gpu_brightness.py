"""mtgs_amd.brightness on the device against the NumPy restatement of tests/brightness_refs.py, BIT FOR BIT: bytes as bytes, floats
and doubles as integers (a NaN is a NaN whatever its sign and payload, which IEEE leaves open).  The estimate is also held against
the reference's own record (tests/golden/brightness_ref.npz).  Shapes are small, except the one image of all 2^24 colours."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from mtgs_amd import brightness as M
from mtgs_amd import stack as S
from tests import brightness_refs as B
from tests import lidar_refs, stack_refs

pytestmark = pytest.mark.gpu
SHAPES = ((1, 1), (1, 3), (1, 4), (1, 5), (3, 7), (5, 64), (2, 257))          # the 4-pixel tails and the 256-thread block edges
FACTORS8 = (0.0, 0.37, 0.999999, 1.0, 1.3, 2.5, 255.0, 0.05)


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def host(t):
    return t.cpu().numpy()


def same(got, want, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    if got.dtype.kind == "f":
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), f"{what}: NaNs differ: {got} != {want}"
        u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
        got, want = np.where(nan, 0, got).view(u), np.where(nan, 0, want).view(u)
    wrong = int((got != want).sum())
    assert wrong == 0, f"{what}: {wrong} of {want.size} elements differ"


def fdev(values):
    return torch.tensor(values, dtype=torch.float64, device="cuda")


@lru_cache(maxsize=None)
def picture(C, h, w, seed=0):
    a = np.random.default_rng(seed).integers(0, 256, (C, h, w, 3), dtype=np.uint8)
    a[0, 0, 0] = (7, 7, 7)                       # a gray, a black and a primary are always among the pixels
    a[-1, -1, -1] = (0, 0, 0)
    a[0, h // 2, w // 2] = (0, 255, 0)
    a.setflags(write=False)
    return a


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---- adjust_brightness ---------------------------------------------------------------------------------------------------------------
def test_all_colours_on_both_paths():
    i = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.stack([(i >> 16) & 255, (i >> 8) & 255, i & 255], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)
    want = B.adjust_brightness(rgb, 1.3)
    x = dev(rgb)
    got = M.adjust_brightness(x, 1.3)
    assert got.is_contiguous() and got.dtype == torch.uint8
    same(host(got), want, "dword path")
    same(host(M.adjust_brightness(x, 1.3, _force_strided=True)), want, "strided path")
    same(host(M.adjust_brightness(x, fdev(1.3), "bgr")), B.adjust_brightness(rgb, 1.3, "bgr"), "bgr")


def layouts(a):
    """{name: (address of channel 0 of pixel (0, 0) of image 0, strides in bytes, the tensor that owns the memory)} of the values of
    a [C, h, w, 3]: contiguous, rows padded, the base one byte off a dword, rows from the bottom up, channels from the last"""
    C, h, w, _ = a.shape
    t = dev(a)
    padded = torch.zeros((C, h + 1, w + 3, 3), dtype=torch.uint8, device="cuda")
    padded[:, :h, 2:w + 2] = t
    window = padded[:, :h, 2:w + 2]
    flat = torch.zeros(a.size + 8, dtype=torch.uint8, device="cuda")        # an allocation starts on a dword
    shifted = flat[1:1 + a.size]
    shifted.copy_(t.reshape(-1))
    assert shifted.data_ptr() % 4 == 1
    shifted = shifted.view(C, h, w, 3)
    upside = torch.flip(t, dims=(1,)).contiguous()                  # the allocation a negative row stride reads
    reversed_ = torch.flip(t, dims=(3,)).contiguous()               # and a negative channel stride
    s = t.stride()
    return {"contiguous": (t.data_ptr(), s, t), "padded": (window.data_ptr(), window.stride(), padded),
            "one byte off": (shifted.data_ptr(), shifted.stride(), flat),
            "rows from the bottom": (upside.data_ptr() + (h - 1) * s[1], (s[0], -s[1], s[2], s[3]), upside),
            "channels from the last": (reversed_.data_ptr() + 2, (s[0], s[1], s[2], -1), reversed_)}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("C", [1, 8])
def test_small_shapes_in_every_layout(shape, C):
    a = picture(C, *shape)
    factors = FACTORS8[:C]
    for order in ("rgb", "bgr"):
        want = B.adjust_brightness(a, np.array(factors), order)
        f = fdev(factors)
        for name, (address, strides, _owner) in layouts(a).items():
            for dtype, w in ((torch.uint8, want), (torch.float32, B.unit_float(want))):
                out = torch.empty(a.shape, dtype=dtype, device="cuda")
                M._launch(address, strides, a.shape[:3], f, 1, order == "bgr", out, stream())
                same(host(out), w, f"{name} {order} {dtype}")
    # the public call on what torch can express: a tensor, a padded view and a view off a dword
    lay = layouts(a)
    views = {"contiguous": lay["contiguous"][2], "padded": lay["padded"][2][:, :shape[0], 2:shape[1] + 2],
             "one byte off": lay["one byte off"][2][1:1 + a.size].view(a.shape)}
    want = B.adjust_brightness(a, np.array(factors))
    for name, v in views.items():
        assert torch.equal(v, dev(a))
        same(host(M.adjust_brightness(v, fdev(factors))), want, name)
        same(host(M.adjust_brightness(v, fdev(factors), image_float=True)), B.unit_float(want), name + " float")
        same(host(M.adjust_brightness(v, fdev(factors), _force_strided=True)), want, name + " strided")
    if C == 1:
        same(host(M.adjust_brightness(views["contiguous"][0], 1.3)), B.adjust_brightness(a[0], 1.3), "one image [h, w, 3]")
        same(host(M.adjust_brightness(views["contiguous"], fdev(1.3))), B.adjust_brightness(a, 1.3), "a factor []")


@pytest.mark.parametrize("factor", [0.0, 1.0, 1e-310, 0.999999, 255.0, 1e300, float("inf"), float("nan")])
def test_factors_at_the_edges(factor):
    a = picture(2, 5, 64, seed=1)
    want = B.adjust_brightness(a, factor)
    same(host(M.adjust_brightness(dev(a), factor)), want, "a Python float")
    same(host(M.adjust_brightness(dev(a), fdev([factor, factor]), image_float=True, _force_strided=True)), B.unit_float(want), "a tensor")
    if factor != factor or factor in (0.0, 1e-310):
        assert not want.any()
    if factor >= 255.0:
        assert np.array_equal(want.max(axis=-1), np.where(a.max(axis=-1) > 0, 255, 0))


def test_a_captured_launch_follows_its_factor_and_its_images():
    frames = [picture(8, 5, 64, seed=s) for s in (2, 3)]
    static, f = dev(frames[0]).clone(), fdev(FACTORS8)
    run = lambda: (M.adjust_brightness(static, f, "bgr"), M.adjust_brightness(static[:, :3, :7], f, image_float=True))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        outs = run()
    for which, factors in ((0, FACTORS8), (0, FACTORS8[::-1]), (1, (1.1,) * 8)):
        static.copy_(dev(frames[which]))
        f.copy_(fdev(factors))                                  # written AFTER the capture: the kernel reads it from device memory
        for o in outs:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        same(host(outs[0]), B.adjust_brightness(frames[which], np.array(factors), "bgr"), f"replay {which}")
        same(host(outs[1]), B.unit_float(B.adjust_brightness(frames[which][:, :3, :7], np.array(factors))), f"replay {which}, a window")


def test_out_is_written_and_an_alias_is_refused():
    a = picture(2, 3, 7)
    x = dev(a)
    out = torch.zeros_like(x)
    assert M.adjust_brightness(x, 2.0, out=out) is out
    same(host(out), B.adjust_brightness(a, 2.0))
    with pytest.raises(ValueError, match="out overlaps images"):
        M.adjust_brightness(x, 2.0, out=x)
    assert torch.equal(x, dev(a))
    with pytest.raises(RuntimeError, match="factors must be a DEVICE tensor"):
        M.adjust_brightness(x, torch.ones(2, dtype=torch.float64))


# ---- estimate_brightness_factors -------------------------------------------------------------------------------------------------------
YAWS8 = (0.0, 55.0, -55.0, 110.0, -110.0, 185.0, -185.0, 180.0)


@lru_cache(maxsize=None)
def scene(n, h=37, w=120, seed=0, yaws=YAWS8, f=86.0):
    rng = np.random.default_rng(seed)
    pts = lidar_refs.sweep(rng, n)
    mats = np.stack([lidar_refs.camera(y, f, rng.uniform(-0.3, 0.3, 3), w, h)[0] for y in yaws])
    images = rng.integers(1, 256, (len(yaws), h, w, 3), dtype=np.uint8)
    for a in (pts, mats, images):
        a.setflags(write=False)
    return pts, mats, images


def check_estimate(pts, mats, images, what="", make=dev, **kw):
    want_f, want_s = B.estimate_factors(pts, mats, images, **kw)
    got_f, got_s = M.estimate_brightness_factors(make(pts), dev(mats), dev(images), return_stats=True, **kw)
    torch.cuda.synchronize()
    assert got_f.dtype == torch.float64 and got_f.is_cuda and got_s.dtype == torch.int64 and tuple(got_s.shape) == want_s.shape
    print(f"{what}: overlap counts {want_s[:, 0].tolist()}, factors {host(got_f).tolist()}")
    same(host(got_s), want_s, what + " stats")
    same(host(got_f), want_f, what + " factors")
    return want_f, want_s


def test_the_golden_scene_equals_the_references_record():
    g = B.golden()
    got_f, got_s = M.estimate_brightness_factors(dev(g["points"]), dev(g["lidar2imgs"]), dev(g["images"]), return_stats=True)
    again = M.estimate_brightness_factors(dev(g["points"]), dev(g["lidar2imgs"]), dev(g["images"]), return_stats=True)
    stats = host(got_s)
    same(host(got_f), g["factors"], "factors against the reference's")
    h, w = g["images"].shape[1:3]
    overlap = stats[:, 0] >= 10
    assert overlap.sum() >= 3 and (~overlap).sum() >= 2
    used = np.stack([g["used_count"], g["used_s1"], g["used_s2"]], axis=1)
    same(np.where(overlap[:, None], stats[:, :3], np.concatenate([np.full((8, 1), h * min(100, w)), stats[:, 3:]], axis=1)), used, "sums")
    same(stats, B.pair_stats(g["points"], g["lidar2imgs"], g["images"]), "stats against the restatement")
    assert torch.equal(again[0], got_f) and torch.equal(again[1], got_s)                  # two runs repeat every bit
    assert M.estimate_brightness_factors(dev(g["points"]), dev(g["lidar2imgs"]), dev(g["images"])).shape == (8,)


@pytest.mark.parametrize("n", [0, 255, 256, 257, 1025])
def test_point_counts_at_the_workgroup_edges(n):
    pts, mats, images = scene(n, seed=n)
    _, stats = check_estimate(pts, mats, images, f"N={n}")
    if n == 0:
        assert not stats[:, :3].any()
    if n == 1025:
        assert (stats[:, 0] > 0).sum() >= 4


@pytest.mark.parametrize("w", [40, 100, 101, 199])
def test_strips_clipped_exact_and_overlapping(w):
    pts, mats, images = scene(300, h=19, w=w, seed=w, f=0.7 * w)
    check_estimate(pts, mats, images, f"w={w}", min_overlap=1 << 30)                   # every pair on its strips
    check_estimate(pts, mats, images, f"w={w} strip=7", strip=7)


@pytest.mark.parametrize("common", [9, 10])
def test_exactly_nine_and_ten_common_points(common):
    """two cameras in one pose see the same points: `common` of them in front, the rest behind"""
    rng = np.random.default_rng(common)
    m = lidar_refs.camera(0.0, 40.0, np.zeros(3), 64, 16)[0]
    front = np.stack([rng.uniform(5, 20, common), rng.uniform(-1, 1, common), rng.uniform(-0.5, 0.5, common)], -1)
    behind = front[rng.integers(0, common, 300 - common)] * [-1.0, 1.0, 1.0]
    pts = np.concatenate([behind[:150], front, behind[150:]]).astype(np.float32)
    images = rng.integers(1, 256, (2, 16, 64, 3), dtype=np.uint8)
    want_f, stats = check_estimate(pts, np.stack([m, m]), images, f"{common} common points", pairs=((0, 1, 0),))
    assert stats[0, 0] == common
    strips = B.solve_factors(stats, 2, 16, 64, ((0, 1, 0),), min_overlap=1 << 30)
    assert (common >= 10) == (not np.array_equal(want_f, strips))


def test_the_chain_branches_on_the_device():
    pts, mats, images = scene(1500, seed=11)
    for what, pairs in (("C = 2, one pair", None), ("cam1 has no factor yet", ((1, 3, 0), (0, 1, 0))),
                        ("a camera that is cam2 twice", ((0, 1, 0), (0, 7, 1), (5, 7, 0), (6, 7, 1))),
                        ("a camera in no pair", ((0, 1, 0), (0, 2, 1))), ("side 1 first", ((0, 2, 1),))):
        if pairs is None:
            f, _ = check_estimate(pts, mats[:2], images[:2], what, pairs=((0, 1, 0),))
        else:
            f, _ = check_estimate(pts, mats, images, what, pairs=pairs)
            untouched = sorted(set(range(8)) - {0} - {b for _, b, _ in pairs})
            assert len(set(f[untouched].tolist() + [f[0]])) == 1                # 1.0 each before the normalisation
    black = np.array(images)
    black[1] = 0
    f, _ = check_estimate(pts[:0], mats, black, "an all-black strip")
    assert np.isnan(f).any() or np.isinf(f).any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_point_rows_with_a_stride(dtype):
    pts, mats, images = scene(700, seed=5)
    wide = np.zeros((700, 5), dtype=dtype)
    wide[:, 1:4] = pts
    check_estimate(wide[:, 1:4], mats, images, f"{dtype.__name__} rows of stride 5", make=lambda a: dev(wide)[:, 1:4])


def test_the_estimate_and_the_adjust_in_one_graph():
    scenes = [scene(900, seed=s) for s in (21, 22)]
    pts, mats = dev(scenes[0][0]).clone(), dev(scenes[0][1])
    static = dev(scenes[0][2]).clone()

    def run():
        f, s = M.estimate_brightness_factors(pts, mats, static, return_stats=True)
        return f, s, M.adjust_brightness(static, f, "bgr")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                     # the pair table is uploaded here, before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        outs = run()
    for which in (1, 0, 0):
        static.copy_(dev(scenes[which][2]))
        pts.copy_(dev(scenes[which][0]))
        for o in outs:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        want_f, want_s = B.estimate_factors(scenes[which][0], scenes[0][1], scenes[which][2])
        same(host(outs[1]), want_s, f"replay on scene {which}: stats")
        same(host(outs[0]), want_f, f"replay on scene {which}: factors")
        same(host(outs[2]), B.adjust_brightness(scenes[which][2], want_f, "bgr"), f"replay on scene {which}: images")


# ---- the stack -------------------------------------------------------------------------------------------------------------------------
def test_the_stack_equalises_in_front_of_the_painting():
    rng = np.random.default_rng(31)
    h, w, pairs = 37, 53, ((0, 1, 0), (1, 2, 0))
    mats = np.stack([lidar_refs.camera(40.0 * c + 10.0, 30.0, rng.uniform(-0.5, 0.5, 3), w, h)[0] for c in range(3)])
    images = (rng.integers(0, 256, (3, h, w, 3)) * np.array([0.4, 0.7, 1.0])[:, None, None, None]).astype(np.uint8)
    masks = rng.integers(0, 20, (3, h, w, 1), dtype=np.uint8)
    boxes = stack_refs.boxes_on_the_ring(rng, 4)
    pts = stack_refs.sweep_with_boxes(rng, 1500, boxes, per_box=25)
    args = lambda img: (dev(pts), boxes, ["vehicle"] * 4, list("abcd"), np.eye(4), dev(mats), img, dev(masks))
    factors = M.estimate_brightness_factors(dev(pts), dev(mats), dev(images), pairs)
    adjusted = M.adjust_brightness(dev(images), factors, "bgr")
    assert not torch.equal(adjusted, dev(images)) and len(set(host(factors).tolist())) == 3
    on = S.SweepStack().configure_brightness(equalise_brightness=True, pairs=pairs).add_frame(*args(dev(images)))
    by_hand = S.SweepStack().add_frame(*args(adjusted))
    off = S.SweepStack().add_frame(*args(dev(images)))
    off_too = S.SweepStack().configure_brightness(equalise_brightness=False).add_frame(*args(dev(images)))
    torch.cuda.synchronize()
    end = int(on.offsets[-1])
    assert end > 100 and torch.equal(on.offsets, by_hand.offsets) and torch.equal(on.offsets, off.offsets)
    for name in ("points", "rgb", "labels"):
        assert torch.equal(getattr(on, name)[:end], getattr(by_hand, name)[:end]), name
        assert torch.equal(getattr(off, name)[:end], getattr(off_too, name)[:end]), name
    assert not torch.equal(on.rgb[:end], off.rgb[:end]) and torch.equal(on.labels[:end], off.labels[:end])
    same(host(adjusted), B.adjust_brightness(images, B.estimate_factors(pts, mats, images, pairs)[0], "bgr"), "the equalised images")
