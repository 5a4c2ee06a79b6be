"""Presenting frames on the device (mtgs_amd/present.py, csrc/present.hip) against the two references of tests/present_refs.py.

Oracle 1, the NumPy restatement of include/mtgs_present.h: the float frame and the uint8 frame are byte-identical, for every kind,
option, layout and alignment.
Oracle 2, the torch transcription of nerfstudio's colormaps and of the viewer's / render tool's frame code, run on the device: the
frames are identical except at threshold pixels (where the restatement's t = v * 255 lies within 4 ulp of an integer), where the
table index may differ by one; threshold pixels are at most 0.1 % of every frame compared (asserted, so that an input cannot hide a
failure behind them).
The depth resize: against F.interpolate on the device within a derived bound, and bit for bit against the restatement."""
import numpy as np
import pytest
import torch

from mtgs_amd import present as P
from tests import present_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
# 3 * W mod 4 takes 3, 3, 0, 2, 3, 3, 0, 3, 1; 257 x 259 gives the stats launch several workgroups and a ragged last one
SHAPES = [(1, 1), (1, 5), (3, 4), (5, 6), (7, 9), (30, 53), (17, 64), (17, 65), (257, 259)]
MAX_THRESHOLD_SHARE = 1e-3
TABLES = R.tables()


@pytest.fixture(scope="module", autouse=True)
def golden_tables():
    """the named tables come from tests/golden/colormap_luts.npz: matplotlib is not needed where this runs"""
    for name, table in TABLES.items():
        P.register_colormap(name, table)
    yield


def rand(shape, seed, lo=0.02, hi=0.98):
    return np.random.default_rng(seed).uniform(lo, hi, size=shape).astype(np.float32)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def lut_of(name):
    return None if name == "gray" else TABLES["turbo" if name == "default" else name]


def np_panel(kind, src, o=P.ColormapOptions(), **kw):
    return R.panel(kind, src, lut=lut_of(o.colormap), normalize=o.normalize, cmin=o.colormap_min, cmax=o.colormap_max, invert=o.invert, **kw)


def ns_options(o):
    return R.NSColormapOptions(o.colormap, o.normalize, o.colormap_min, o.colormap_max, o.invert)


def same_bytes(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    a, b = (got.view(np.uint32), want.view(np.uint32)) if got.dtype == np.float32 else (got, want)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        raise AssertionError(f"{len(bad)} of {a.size} values differ; first at {bad[0].tolist()}: {got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}")


# ---- oracle 1: the depth colormap ------------------------------------------------------------------------------------------------------
DEPTH_CASES = {
    "given": dict(near=1.0, far=60.0),
    "from_data": dict(),
    "near_from_data": dict(far=75.0),
    "near_equals_far": dict(near=20.0, far=20.0),
    "normalize_from_data": dict(o=P.ColormapOptions("viridis", normalize=True)),
    "normalize_given_invert_range": dict(near=10.0, far=50.0, o=P.ColormapOptions("magma", True, 0.1, 0.8, True)),
    "far_below_near_normalize": dict(near=50.0, far=10.0, o=P.ColormapOptions("turbo", normalize=True)),
    "accumulation": dict(near=1.0, far=60.0, acc=True),
    "accumulation_gray_from_data": dict(acc=True, o=P.ColormapOptions("gray")),
    "nan_pixel_given": dict(near=1.0, far=60.0, nan=True, acc=True),
    "nan_pixel_from_data": dict(nan=True),
    "nan_pixel_normalize": dict(near=1.0, far=60.0, nan=True, o=P.ColormapOptions("gray", normalize=True)),
    "all_equal_from_data": dict(equal=True),
    "all_equal_normalize": dict(equal=True, near=0.0, far=100.0, o=P.ColormapOptions("default", normalize=True, invert=True)),
}


@pytest.mark.parametrize("case", list(DEPTH_CASES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_depth_colormap_equals_the_restatement(shape, case):
    c = dict(DEPTH_CASES[case])
    o = c.pop("o", P.ColormapOptions())
    H, W = shape
    depth = np.full((H, W, 1), 37.25, dtype=np.float32) if c.pop("equal", False) else rand((H, W, 1), 11, 0.5, 80.0)
    if c.pop("nan", False):
        depth[H // 2, W // 3, 0] = np.nan
    acc = rand((H, W, 1), 12, 0.0, 1.0) if c.pop("acc", False) else None
    near, far = c.get("near"), c.get("far")
    want = R.panel_np(np_panel("depth", depth, o, acc=acc, near=near, far=far))
    got = P.colorize_depth(dev(depth), dev(acc), near, far, o)
    same_bytes(got, want)
    # the same panel as a uint8 frame through the render tool's entry: the rounding conversion
    outputs = {"depth": dev(depth), "accumulation": dev(acc if acc is not None else np.ones((H, W, 1), dtype=np.float32))}
    want8 = R.quantise_np(R.panel_np(np_panel("depth", depth, o, acc=outputs["accumulation"].cpu().numpy(), near=near, far=far)), "round")
    same_bytes(P.render_frame(outputs, ["depth"], near, far, o), want8)


# ---- oracle 1: the float and boolean colormaps, pass-through -------------------------------------------------------------------------------
FLOAT_OPTIONS = [P.ColormapOptions(), P.ColormapOptions("gray"), P.ColormapOptions("plasma", normalize=True),
                 P.ColormapOptions("viridis", True, 0.2, 0.9, True), P.ColormapOptions("inferno", False, -0.5, 1.5, True)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_float_boolean_and_rgb_equal_the_restatement(shape):
    H, W = shape
    v = rand((H, W, 1), 21, -0.3, 1.4)
    for o in FLOAT_OPTIONS:
        same_bytes(P.colorize(dev(v), o), R.panel_np(np_panel("float", v, o)))
    v[H // 2, W // 2, 0] = np.nan
    for o in FLOAT_OPTIONS[:3]:
        same_bytes(P.colorize(dev(v), o), R.panel_np(np_panel("float", v, o)))
    table = rand((256, 3), 22, 0.0, 1.0)                                   # a table of the caller's
    same_bytes(P.colorize(dev(np.abs(v)), P.ColormapOptions(dev(table))), R.panel_np(R.panel("float", np.abs(v), lut=table)))
    mask = np.random.default_rng(23).random((H, W, 1)) < 0.5
    same_bytes(P.colorize(dev(mask)), R.panel_np(R.panel("bool", mask)))
    same_bytes(P.colorize(dev(mask.astype(np.uint8) * 7)), R.panel_np(R.panel("bool", mask)))
    rgb = rand((H, W, 3), 24, -0.2, 1.2)
    t = dev(rgb)
    assert P.colorize(t) is t
    out = torch.full((H, W, 3), 9.0, device=DEV)
    assert P.colorize(t, out=out) is out
    same_bytes(out, rgb)
    # a uint8 base that is not 4-byte aligned: the byte-store path
    if H * W * 3 >= 2:
        store = torch.zeros(H * W * 3 + 4, dtype=torch.uint8, device=DEV)
        for shift in (1, 2, 3):
            store.zero_()
            frame = store[shift:shift + H * W * 3].view(H, W, 3)
            P.viewer_frame({"rgb": t}, "rgb", out=frame)
            same_bytes(frame, R.quantise_np(rgb, "truncate"))
            assert int(store[:shift].sum()) == 0 and int(store[shift + H * W * 3:].sum()) == 0


# ---- oracle 1: the viewer's frame ------------------------------------------------------------------------------------------------------
def viewer_outputs(H, W, seed):
    rgb, depth = rand((H, W, 3), seed, 0.0, 1.0), rand((H, W, 1), seed + 1, 0.0, 1.0)
    mask = np.random.default_rng(seed + 2).random((H, W, 1)) < 0.5
    return {"rgb": rgb, "depth": depth, "mask": mask}


def viewer_frame_np(outputs, a, oa, b=None, ob=None, pct=0.5, aspect=None, shift=0):
    kind = lambda name: {"rgb": "rgb", "depth": "float", "mask": "bool"}[name]
    H, W = outputs[a].shape[:2]
    ph, pw = P.pad_sizes(H, W, aspect)
    if b is None:
        return R.frame_np([np_panel(kind(a), outputs[a], oa)], [(ph, pw, H, W, 0)], H + 2 * ph, W + 2 * pw, -1, "truncate", shift)
    k = P.split_index(pct, W)
    panels = [np_panel(kind(a), outputs[a], oa), np_panel(kind(b), outputs[b], ob)]
    return R.frame_np(panels, [(ph, pw, H, k, 0), (ph, pw + k, H, W - k, k)], H + 2 * ph, W + 2 * pw, pw + k, "truncate", shift)


VIEWER_CASES = [("rgb", P.ColormapOptions(), None, None), ("depth", P.ColormapOptions("default", normalize=True), None, None),
                ("rgb", P.ColormapOptions(), "depth", P.ColormapOptions("viridis", invert=True)),
                ("depth", P.ColormapOptions("gray", normalize=True), "mask", P.ColormapOptions()),
                ("depth", P.ColormapOptions("magma"), "depth", P.ColormapOptions("cividis", True, 0.1, 0.9))]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_viewer_frame_equals_the_restatement(shape):
    """split at index 0, at W - 1 and in the middle; padding on each axis and none; a frame written into `out=`"""
    H, W = shape
    outputs = viewer_outputs(H, W, 31)
    on_dev = {k: dev(v) for k, v in outputs.items()}
    wide, tall = (W + 14) / H, W / (H + 14)                  # 7 columns on each side; 7 rows above and below
    for a, oa, b, ob in VIEWER_CASES:
        for pct, aspect in ((0.5, None), (0.0, wide), (1.0, tall), (0.37, (W + 10) / H)):     # the last: 5 columns, not padded
            want, _ = viewer_frame_np(outputs, a, oa, b, ob, pct, aspect)
            got = P.viewer_frame(on_dev, a, oa, b, ob, pct, aspect)
            assert got.dtype == torch.uint8
            same_bytes(got, want)
    assert P.pad_sizes(H, W, wide) == (0, 7) and P.pad_sizes(H, W, tall) == (7, 0) and P.pad_sizes(H, W, (W + 10) / H) == (0, 0)
    out = torch.full(want.shape, 77, dtype=torch.uint8, device=DEV)
    assert P.viewer_frame(on_dev, a, oa, b, ob, pct, aspect, out=out) is out
    same_bytes(out, want)


# ---- oracle 1: the render tool's frame -----------------------------------------------------------------------------------------------------
def render_outputs(H, widths, seed):
    """outputs of unequal widths (the tool concatenates whatever the model returns): rgb*, depth*, mask*, one accumulation per depth"""
    out = {}
    for j, w in enumerate(widths):
        out[f"rgb{j}"] = rand((H, w, 3), seed + 10 * j, -0.1, 1.1)
        out[f"mask{j}"] = np.random.default_rng(seed + 10 * j + 1).random((H, w, 1)) < 0.5
        out[f"feature{j}"] = rand((H, w, 1), seed + 10 * j + 2, 0.0, 1.0)
    return out


@pytest.mark.parametrize("H, widths", [(1, (1, 1)), (3, (5, 2)), (7, (9, 6, 3)), (17, (65, 64)), (30, (53, 7, 18)), (257, (259, 33))],
                         ids=lambda v: str(v).replace(" ", ""))
def test_render_frame_concatenation_equals_the_restatement(H, widths):
    outputs = render_outputs(H, widths, 41)
    W0 = widths[0]
    outputs["depth"], outputs["accumulation"] = rand((H, W0, 1), 42, 0.5, 80.0), rand((H, W0, 1), 43, 0.0, 1.0)
    on_dev = {k: dev(v) for k, v in outputs.items()}
    o = P.ColormapOptions("turbo", normalize=True)
    names = ["depth"] + [f"{kind}{j}" for j, kind in zip(range(1, len(widths)), ("rgb", "feature", "mask"))] + ["mask0"]
    kind_of = lambda n: "depth" if n == "depth" else {"r": "rgb", "f": "float", "m": "bool"}[n[0]]
    for near, far in ((None, None), (2.0, 70.0)):
        panels = [np_panel(kind_of(n), outputs[n], o, **(dict(acc=outputs["accumulation"], near=near, far=far) if n == "depth" else {})) for n in names]
        ws = [outputs[n].shape[1] for n in names]
        places = [(0, x0, H, w, 0) for x0, w in zip(P.concat_columns(ws), ws)]
        want, _ = R.frame_np(panels, places, H, sum(ws), fmt="round")
        got = P.render_frame(on_dev, names, near, far, o)
        same_bytes(got, want)
        assert got.shape == (H, sum(ws), 3)


def test_eight_panels_the_maximum():
    H = 7
    widths = (9, 6, 3, 1, 5, 4, 11, 2)
    outputs = {f"feature{j}": rand((H, w, 1), 50 + j, 0.0, 1.0) for j, w in enumerate(widths)}
    outputs.update({f"depth{j}": rand((H, w, 1), 60 + j, 0.5, 80.0) for j, w in enumerate(widths)})
    outputs["accumulation"] = rand((H, 9, 1), 70, 0.0, 1.0)
    on_dev = {k: dev(v) for k, v in outputs.items()}
    o = P.ColormapOptions("inferno", normalize=True)
    names = [f"feature{j}" for j in range(8)]
    places = [(0, x0, H, w, 0) for x0, w in zip(P.concat_columns(widths), widths)]
    want, _ = R.frame_np([np_panel("float", outputs[n], o) for n in names], places, H, sum(widths), fmt="round")
    same_bytes(P.render_frame(on_dev, names, options=o), want)       # eight sources, each with extrema of its own
    with pytest.raises(ValueError, match="9 panels"):
        P.render_frame(on_dev, names + ["feature0"], options=o)
    # eight depth panels need eight accumulations of their widths: only the first fits
    with pytest.raises(ValueError, match="accumulation must be contiguous float32"):
        P.render_frame(on_dev, ["depth0", "depth1"], options=o)


# ---- oracle 2: the torch transcription on the device -------------------------------------------------------------------------------------
def agree_up_to_threshold_pixels(got, torch_frame, threshold, minus, plus):
    """got == the restatement (oracle 1 holds): the transcription's frame may differ from it only at threshold pixels, and there
    only as a table index one lower or one higher would"""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    share = threshold.mean()
    differ = (got != torch_frame).any(axis=-1)
    print(f"{threshold.sum()} threshold pixels of {threshold.size} ({share:.3%}); {differ.sum()} pixels differ, "
          f"{(differ & ~threshold).sum()} of them elsewhere")
    assert share <= MAX_THRESHOLD_SHARE
    assert not (differ & ~threshold).any()
    by_one = (torch_frame == minus).all(axis=-1) | (torch_frame == plus).all(axis=-1)
    assert by_one[differ].all()


ORACLE2_VIEWER = [((30, 53), 0), ((17, 65), 1), ((257, 259), 2)]


@pytest.mark.parametrize("shape, seed", ORACLE2_VIEWER, ids=lambda v: str(v).replace(" ", ""))
def test_viewer_frame_against_the_transcription_on_the_device(shape, seed):
    H, W = shape
    outputs = viewer_outputs(H, W, 100 + seed)
    outputs["depth"] = rand((H, W, 1), 103 + seed, 0.02, 0.98)            # no pixel clipped: t = 0 and t = 255 are integers
    on_dev = {k: dev(v) for k, v in outputs.items()}
    cases = [("depth", P.ColormapOptions(), None, None, 0.5, None), ("rgb", P.ColormapOptions(), "depth", P.ColormapOptions("viridis", invert=True), 0.4, (W + 14) / H),
             ("depth", P.ColormapOptions("magma", False, 0.1, 0.9), "mask", P.ColormapOptions(), 1.0, W / (H + 14))]
    if H * W >= 2000:          # the extrema themselves give t = 0 and t = 255: two threshold pixels, affordable in a large frame only
        cases.append(("depth", P.ColormapOptions("plasma", normalize=True), "rgb", P.ColormapOptions(), 0.0, None))
    for a, oa, b, ob, pct, aspect in cases:
        frames = [viewer_frame_np(outputs, a, oa, b, ob, pct, aspect, shift) for shift in (0, -1, 1)]
        theirs = R.viewer_frame_torch(on_dev, a, ns_options(oa), b, None if ob is None else ns_options(ob), pct, aspect)
        got = P.viewer_frame(on_dev, a, oa, b, ob, pct, aspect)
        same_bytes(got, frames[0][0])
        agree_up_to_threshold_pixels(got, theirs, frames[0][1], frames[1][0], frames[2][0])


@pytest.mark.parametrize("shape, seed", [((30, 53), 0), ((48, 50), 1), ((257, 259), 2)], ids=lambda v: str(v).replace(" ", ""))
def test_depth_colormap_and_render_frame_against_the_transcription_on_the_device(shape, seed):
    H, W = shape
    depth, acc, rgb = rand((H, W, 1), 110 + seed, 2.0, 60.0), rand((H, W, 1), 113 + seed, 0.0, 1.0), rand((H, W, 3), 116 + seed, 0.0, 1.0)
    outputs = {"rgb": rgb, "depth": depth, "accumulation": acc}
    on_dev = {k: dev(v) for k, v in outputs.items()}
    cases = [(1.0, 61.0, P.ColormapOptions()), (0.5, 75.0, P.ColormapOptions("viridis", False, 0.05, 0.95, True))]
    if H * W >= 2000:
        cases += [(None, None, P.ColormapOptions("magma")), (None, 70.0, P.ColormapOptions("turbo", normalize=True))]
    for near, far, o in cases:
        # the eval image: float32
        p = np_panel("depth", depth, o, acc=acc, near=near, far=far)
        floats = [R.frame_np([p], [(0, 0, H, W, 0)], H, W, fmt="float", shift=s) for s in (0, -1, 1)]
        theirs = R.ns_apply_depth_colormap(on_dev["depth"], on_dev["accumulation"], near, far, ns_options(o)).cpu().numpy()
        got = P.colorize_depth(on_dev["depth"], on_dev["accumulation"], near, far, o)
        same_bytes(got, floats[0][0])
        agree_up_to_threshold_pixels(got, theirs, floats[0][1], floats[1][0], floats[2][0])
        # the render tool's frame: rgb | depth, uint8 by the rounding rule
        places = [(0, 0, H, W, 0), (0, W, H, W, 0)]
        frames = [R.frame_np([np_panel("rgb", rgb), p], places, H, 2 * W, fmt="round", shift=s) for s in (0, -1, 1)]
        theirs_f, theirs_8 = R.render_frame_torch(on_dev, ["rgb", "depth"], near, far, ns_options(o))
        got = P.render_frame(on_dev, ["rgb", "depth"], near, far, o)
        same_bytes(got, frames[0][0])
        agree_up_to_threshold_pixels(got, theirs_8, frames[0][1], frames[1][0], frames[2][0])


def test_expected_share_of_threshold_pixels_for_random_depths():
    """about 0.01 % for uniformly random fp32 depths: the restatement on a large frame (no device needed for the count itself)"""
    depth = rand((512, 512, 1), 120, 2.0, 60.0)
    _, threshold = R.frame_np([np_panel("depth", depth, near=1.0, far=61.0)], [(0, 0, 512, 512, 0)], 512, 512, fmt="float")
    print(f"{threshold.sum()} of {threshold.size}: {threshold.mean():.4%}")
    assert threshold.mean() <= 3e-4


# ---- the depth resize ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, state", [((1, 1), "high"), ((30, 53), "low_move"), ((257, 259), "low_static"), ((257, 259), "high"),
                                          ((600, 701), "high"), ((600, 701), "low_move")], ids=lambda v: str(v).replace(" ", ""))
def test_viewer_depth_against_interpolate_and_the_restatement(shape, state):
    """|err| <= 2^-22 * max(H, W) * (max tap - min tap) + 8 * 2^-24 * max|tap| per pixel: one rounding of difference in the source
    coordinate (at most max(H, W) in size, so an error of 2^-23 * max(H, W) in a weight, on both axes) and the seven roundings of
    the blend, with one to spare.  Derived, not tuned."""
    H, W = shape
    depth = rand((H, W, 1), 130, 0.5, 80.0)
    d = dev(depth)
    h, w = P.depth_size(H, W, state)
    got = P.viewer_depth(d, state, 1.0)
    assert got.shape == (h, w, 1) and got.dtype == torch.float32
    want, lo, hi = R.depth_resize_np(depth[..., 0], h, w, 1.0)
    same_bytes(got[..., 0].contiguous(), want)
    theirs = R.viewer_depth_torch(d, state)
    assert theirs.shape == got.shape
    bound = 2.0 ** -22 * max(H, W) * (hi - lo).astype(np.float64) + 8 * 2.0 ** -24 * np.maximum(np.abs(hi), np.abs(lo))
    err = np.abs(got[..., 0].cpu().numpy().astype(np.float64) - theirs[..., 0].cpu().numpy())
    print(f"{H}x{W} -> {h}x{w}: max error {err.max():.3e}, smallest bound {bound.min():.3e}, largest error / bound {(err / bound).max():.3f}")
    assert (err <= bound).all()
    # times viser_scale_ratio: one more fp32 multiplication (the reference's, in NumPy on the host)
    scaled = P.viewer_depth(d, state, 2.5, out=torch.empty((h, w, 1), device=DEV))
    same_bytes(scaled, got.cpu().numpy() * np.float32(2.5))


# ---- behaviour ---------------------------------------------------------------------------------------------------------------------------
def test_a_frame_with_out_is_capturable_and_follows_its_sources():
    H, W = 30, 53
    first, second = viewer_outputs(H, W, 140), viewer_outputs(H, W, 150)
    src = {k: dev(v) for k, v in first.items()}
    oa, ob = P.ColormapOptions("turbo", normalize=True), P.ColormapOptions()
    aspect = (W + 14) / H
    frame = torch.zeros((H, W + 14, 3), dtype=torch.uint8, device=DEV)
    depth_out = torch.zeros((H, W, 1), device=DEV)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):                      # warm-up on the capture stream: the table and the workspace exist
        P.viewer_frame(src, "depth", oa, "rgb", ob, 0.4, aspect, out=frame)
        P.viewer_depth(src["depth"], "high", 1.5, out=depth_out)
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    allocations = lambda: torch.cuda.memory_stats()["allocation.all.allocated"]
    with torch.cuda.graph(graph, stream=stream):
        before = allocations()                           # inside: entering a capture allocates state of torch's own
        P.viewer_frame(src, "depth", oa, "rgb", ob, 0.4, aspect, out=frame)
        P.viewer_depth(src["depth"], "high", 1.5, out=depth_out)
        assert allocations() == before                   # nothing was allocated for the frame
    for outputs in (second, first):
        for k in src:
            src[k].copy_(dev(outputs[k]))
        frame.zero_()
        graph.replay()
        torch.cuda.synchronize()
        same_bytes(frame, viewer_frame_np(outputs, "depth", oa, "rgb", ob, 0.4, aspect)[0])
        same_bytes(depth_out[..., 0].contiguous(), R.depth_resize_np(outputs["depth"][..., 0], H, W, 1.5)[0])


def test_no_host_read_with_extrema_taken_from_the_data():
    H, W = 30, 53
    outputs = viewer_outputs(H, W, 160)
    outputs["accumulation"] = rand((H, W, 1), 161, 0.0, 1.0)
    outputs["depth"] = rand((H, W, 1), 162, 0.5, 80.0)
    src = {k: dev(v) for k, v in outputs.items()}
    o = P.ColormapOptions("turbo", normalize=True)
    P.viewer_frame(src, "depth", o)                      # the one upload of the table
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        frame = P.viewer_frame(src, "depth", o, "rgb", None, 0.5, 3.0)
        image = P.colorize_depth(src["depth"], src["accumulation"], None, None, o)
        tool = P.render_frame(src, ["rgb", "depth"], None, None, o)
        small = P.viewer_depth(src["depth"], "low_move", 2.0)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    same_bytes(frame, viewer_frame_np(outputs, "depth", o, "rgb", P.ColormapOptions(), 0.5, 3.0)[0])
    same_bytes(image, R.panel_np(np_panel("depth", outputs["depth"], o, acc=outputs["accumulation"])))
    assert tool.shape == (H, 2 * W, 3) and small.shape == (H, W, 1)


def test_a_named_table_is_uploaded_once():
    v = dev(rand((7, 9, 1), 170))
    device = v.device
    P.register_colormap("cividis", TABLES["cividis"])    # drops any device copy: the next call uploads
    assert ("cividis", device) not in P._DEVICE_TABLES
    o = P.ColormapOptions("cividis")
    out = torch.empty((7, 9, 3), device=DEV)
    P.colorize(v, o, out=out)
    table = P._DEVICE_TABLES[("cividis", device)]
    pointer, count = table.data_ptr(), len(P._DEVICE_TABLES)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    P.colorize(v, o, out=out)
    P.viewer_frame({"depth": v}, "depth", o)
    assert P._DEVICE_TABLES[("cividis", device)] is table and table.data_ptr() == pointer and len(P._DEVICE_TABLES) == count
    assert torch.cuda.memory_allocated() == before       # the frame of the second call above is freed again; no new table stays
    assert torch.equal(table.cpu(), torch.from_numpy(TABLES["cividis"]))
