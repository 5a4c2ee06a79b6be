"""mtgs_amd.undistort on the device: bit for bit the NumPy restatement (tests/undistort_refs.py).  No tolerance anywhere: the map is
fp64 with one rounding per operation (add, multiply and divide are correctly rounded on both sides), everything after it is integer
arithmetic.  uint8 and int32 results are compared for equality, floats and the map as uint32 patterns.  No input has more than
20 000 pixels; every reference is computed once per case."""
from functools import lru_cache
from itertools import permutations
from pathlib import Path

import numpy as np
import pytest
import torch

from mtgs_amd import frame as F
from mtgs_amd import jpegdec as J
from mtgs_amd import undistort as U
from tests import frame_refs as FR
from tests import jpegdec_refs as JD
from tests import undistort_refs as R

pytestmark = pytest.mark.gpu
TW, TH = U.TILE_W, U.TILE_H
JPEG = Path(__file__).resolve().parent / "golden" / "undistort_frame_64x48.jpg"

# The lenses.  "wide" looks through a new camera of 0.7 times the focal length at a pincushion lens with tangential terms: the map
# runs off the source on all four sides, the destination corners lie fully outside.  "barrel" is a nuPlan-like lens in
# keep_focal_length: every pixel stays inside.  Four and five coefficients.
WIDE = (0.3, 0.1, 0.02, -0.015, 0.02)
BARREL = (-0.356, 0.173, 0.001, -0.0005)
EXACT = (16.0, 8.0, 7.0, 5.0)             # powers of two: the shifted maps below are exact


def lens(h, w):
    """(K, new_K) in the dataset's convention for a source of h x w: the principal point off the centre, K' = 0.7 K"""
    f = 0.9 * max(h, w, 8)
    K = (f, 1.05 * f, 0.5 * w + 0.3, 0.5 * h - 0.2)
    return K, (0.7 * K[0], 0.7 * K[1], K[2] + 0.4, K[3] - 0.3)


def shifted(dx, dy=0.0):
    return dict(K=EXACT, D=(0.0,) * 4, new_K=(EXACT[0], EXACT[1], EXACT[2] - dx, EXACT[3] - dy))


# name -> (source size, destination size or None, undistort_camera's arguments)
CASES = {}
for _h, _w in ((1, 1), (2, 2), (37, 53), (TH - 1, TW - 1), (TH, TW), (TH + 1, TW + 1), (2 * TH + 1, 2 * TW + 2)):
    _K, _newK = lens(_h, _w)
    CASES[f"wide-{_h}x{_w}"] = ((_h, _w), None, dict(K=_K, D=WIDE, new_K=_newK))
    # half a pixel up and left into a destination one larger: a 2 x 2 footprint crosses every border and every corner at any size
    CASES[f"half-{_h}x{_w}"] = ((_h, _w), (_h + 1, _w + 1), dict(K=_K, D=(0.0,) * 4, new_K=(_K[0], _K[1], _K[2] + 0.5, _K[3] + 0.5)))
CASES["barrel-37x53"] = ((37, 53), None, dict(K=lens(37, 53)[0], D=BARREL, mode="keep_focal_length"))
CASES["optimal-37x53"] = ((37, 53), None, dict(K=lens(37, 53)[0], D=BARREL + (-0.052,), mode="optimal"))
CASES["other-size"] = ((37, 53), (TH + 2, 2 * TW + 1), dict(K=lens(37, 53)[0], D=WIDE, new_K=lens(TH + 2, 2 * TW + 1)[1]))
CASES["tie-1/64"] = ((13, 17), None, shifted(1.0 / 64))
CASES["tie-3/64"] = ((13, 17), None, shifted(3.0 / 64, 3.0 / 64))
CASES["half"] = ((13, 17), None, shifted(0.5))
CASES["negative"] = ((13, 17), None, shifted(-1.0 / 32, -1.0 / 32))
CASES["nan"] = ((13, 17), None, dict(K=EXACT, D=(float("nan"), 0.0, 0.0, 0.0), mode="keep_focal_length"))
CASES["huge"] = ((13, 17), None, dict(K=EXACT, D=(1e300, 1e300, 0.0, 0.0, 1e300), mode="keep_focal_length"))


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()             # a copy: the cached sources are read-only


def host(t):
    return t.cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint8) if a.dtype == np.bool_ else a


def same(got, want, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    wrong = int((bits(got) != bits(want)).sum())
    assert wrong == 0, f"{what}: {wrong} of {want.size} elements differ"


@lru_cache(maxsize=None)
def sources(shape, seed=0):
    """the planes of a frame as the dataset holds them, and two more dtypes for the nearest rule"""
    h, w = shape
    rng = np.random.default_rng([seed, h, w])
    p = {"image": rng.integers(1, 256, (h, w, 3), dtype=np.uint8), "ego": (rng.random((h, w)) < 0.3).astype(np.uint8) * 255,
         "panoptic": rng.integers(1, 256, (h, w, 3), dtype=np.uint8), "semantic": rng.integers(1, 20, (h, w, 1), dtype=np.uint8),
         "ids": rng.integers(-2 ** 31, 2 ** 31, (h, w, 2), dtype=np.int64).astype(np.int32), "flag": rng.random((h, w)) < 0.5}
    for a in p.values():
        a.setflags(write=False)
    return p


@lru_cache(maxsize=None)
def camera(name):
    shape, size, kw = CASES[name]
    return U.undistort_camera(size=shape, out_size=size, **kw)


def map_arguments(cam):
    """(K, D, new_K) of the restatement: the scalars the camera uploaded, the half pixel already taken off"""
    p = cam.params.cpu().numpy()
    return tuple(p[:4]), tuple(p[8:13]), tuple(p[4:8])


@lru_cache(maxsize=None)
def reference(name):
    """every plane of the restatement for one case, computed once"""
    cam = camera(name)
    K, D, new_K = map_arguments(cam)
    s = sources(cam.source_size)
    h, w = cam.source_size
    m = R.undistort_map(K, D, new_K, *cam.size)
    image = R.remap_linear(s["image"], m)
    return {"map": m, "image": image, "image_float": R.to_float(image), "gray": R.remap_linear(s["image"][:, :, 1], m),
            "valid": R.valid_mask(m, h, w), "valid_ego": R.valid_mask(m, h, w, s["ego"]), "panoptic": R.remap_nearest(s["panoptic"], m),
            "semantic": R.remap_nearest(s["semantic"], m), "ids": R.remap_nearest(s["ids"], m), "flag": R.remap_nearest(s["flag"], m)}


def footprints(name):
    """how many destination pixels have a 2 x 2 footprint that crosses the source's (left, right, top, bottom) border with its other
    axis inside, and its (top-left, top-right, bottom-left, bottom-right) corner; and the share of pixels fully outside"""
    cam = camera(name)
    m, (h, w) = reference(name)["map"], cam.source_size
    ix, iy = R.fixed(m[..., 0]) >> R.SHIFT, R.fixed(m[..., 1]) >> R.SHIFT
    xin, yin = (ix >= 0) & (ix + 1 < w), (iy >= 0) & (iy + 1 < h)
    left, right, top, bottom = ix == -1, ix == w - 1, iy == -1, iy == h - 1
    borders = [int((left & yin).sum()), int((right & yin).sum()), int((top & xin).sum()), int((bottom & xin).sum())]
    corners = [int((top & left).sum()), int((top & right).sum()), int((bottom & left).sum()), int((bottom & right).sum())]
    outside = (ix < -1) | (ix >= w) | (iy < -1) | (iy >= h)
    return borders, corners, float(outside.mean())


# ---- the cases are what they claim to be (host arithmetic, stated here so that a changed lens cannot empty a test quietly) --------
def test_the_lenses_cross_every_border_and_corner():
    for name in CASES:
        if name.startswith("half-"):
            borders, corners, _ = footprints(name)
            (h, w) = CASES[name][0]
            assert corners == [1, 1, 1, 1] and borders == [max(h - 1, 0), max(h - 1, 0), max(w - 1, 0), max(w - 1, 0)], name
    # the wide lens on 37 x 53: a 2 x 2 footprint crosses each of the four borders, the four destination corners are fully outside
    borders, _, outside = footprints("wide-37x53")
    assert all(n > 0 for n in borders), borders
    for name in ("wide-37x53", f"wide-{TH + 1}x{TW + 1}", f"wide-{2 * TH + 1}x{2 * TW + 2}", "other-size"):
        v = reference(name)["valid"]
        assert not v[0, 0] and not v[0, -1] and not v[-1, 0] and not v[-1, -1], name
    # the outside share of the chosen coefficients, by the restatement: K' = 0.7 K shows about 1 / 0.49 of the field and the
    # pincushion terms push it further out -- 55.8 % of the 37 x 53 footprints lie fully outside, 58.4 % of the pixels are not valid
    assert round(outside, 3) == 0.558 and round(1.0 - float(reference("wide-37x53")["valid"].mean()), 3) == 0.584
    assert reference("barrel-37x53")["valid"].all() and 0.0 < 1.0 - reference("optimal-37x53")["valid"].mean() < 0.35
    assert not reference("nan")["valid"].any() and not np.isfinite(reference("nan")["map"]).any()
    assert not reference("huge")["valid"][0, 0] and not reference("huge")["image"][0, 0].any()


# ---- one plane, a frame, eight planes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_every_plane_is_the_restatement_bit_for_bit(name, monkeypatch):
    cam, want = camera(name), reference(name)
    s = {k: dev(v) for k, v in sources(cam.source_size).items()}
    got_map = host(U.undistort_map(cam))
    if name in ("nan", "huge"):                  # NaN payloads are nobody's contract: the non-finite entries are in the same places
        assert np.array_equal(np.isfinite(got_map), np.isfinite(want["map"])) and np.array_equal(np.isnan(got_map), np.isnan(want["map"]))
        assert np.array_equal(got_map[np.isfinite(got_map)], want["map"][np.isfinite(want["map"])])
    else:
        same(got_map, want["map"], "map")
    # the frame: exactly one launch
    calls = []
    monkeypatch.setattr(U, "call", lambda fn, *a, _call=U.call: (calls.append(fn), _call(fn, *a))[1])
    out = U.undistort_frame(cam, image=s["image"], ego_mask=s["ego"], panoptic=s["panoptic"], semantic=s["semantic"])
    assert calls == ["mtgs_undistort_frame"]
    as_float = U.undistort_frame(cam, image=s["image"], image_float=True)
    torch.cuda.synchronize()
    assert set(out) == {"image", "valid_mask", "panoptic", "semantic"} and set(as_float) == {"image", "valid_mask"}
    assert out["valid_mask"].dtype == torch.bool and out["valid_mask"].shape == cam.size + (1,)
    same(host(out["image"]), want["image"], "image")
    same(host(out["valid_mask"]), want["valid_ego"], "valid mask with the ego rule")
    same(host(out["panoptic"]), want["panoptic"], "panoptic")
    same(host(out["semantic"]), want["semantic"], "semantic")
    same(host(as_float["image"]), want["image_float"], "image_float")
    same(host(as_float["valid_mask"]), want["valid"], "valid mask")
    same(host(as_float["image"]), (out["image"].cpu().float() / 255).numpy(), "image_float against torch on the host")
    # one plane at a time: 1 and 3 channels, uint8 and float, [h, w] and [h, w, 1], uint8, int32 and bool through the nearest rule
    same(host(U.undistort_plane(s["image"], cam)), want["image"], "image alone")
    same(host(U.undistort_plane(s["image"], cam, out_dtype=torch.float32)), want["image_float"], "out_dtype")
    same(host(U.undistort_plane(s["image"][:, :, 1], cam)), want["gray"], "one channel [h, w]")
    same(host(U.undistort_plane(s["image"][:, :, 1:2], cam, out_dtype=torch.float32)), R.to_float(want["gray"])[..., None], "one channel, float")
    same(host(U.undistort_plane(s["panoptic"], cam, "nearest")), want["panoptic"], "nearest uint8 x 3")
    same(host(U.undistort_plane(s["ids"], cam, "nearest")), want["ids"], "nearest int32 x 2")
    same(host(U.undistort_plane(s["flag"], cam, "nearest")), want["flag"], "nearest bool")


EIGHT = ("image", "image_float", "gray", "ids", "panoptic", "flag", "valid", "valid_ego")


def eight_planes(cam, s, order):
    """all MAX_PLANES planes in one launch, in `order`: every operation, every dtype"""
    spec = {"image": (s["image"], torch.uint8, U._LINEAR), "image_float": (s["image"], torch.float32, U._LINEAR),
            "gray": (s["image"][:, :, 1:2], torch.uint8, U._LINEAR), "ids": (s["ids"], torch.int32, U._NEAREST),
            "panoptic": (s["panoptic"], torch.uint8, U._NEAREST), "flag": (s["flag"].view(torch.uint8)[:, :, None], torch.uint8, U._NEAREST),
            "valid": (None, torch.uint8, U._VALID), "valid_ego": (s["ego"][:, :, None], torch.uint8, U._VALID)}
    outs, records = {}, []
    for key in order:
        src, dtype, op = spec[key]
        c = 1 if op == U._VALID else src.shape[2]
        outs[key] = torch.full(cam.size + (c,), 77, dtype=dtype, device="cuda")
        records.append(U._record(src, outs[key], op, c, dtype == torch.float32))
    U._launch(cam, records, torch.cuda.current_stream().cuda_stream)
    return outs


@pytest.mark.parametrize("name", ["wide-37x53", f"half-{TH + 1}x{TW + 1}", "other-size", "negative"])
def test_eight_planes_in_one_launch_in_any_order(name):
    assert len(EIGHT) == U.MAX_PLANES
    cam, want = camera(name), reference(name)
    s = {k: dev(v) for k, v in sources(cam.source_size).items()}
    orders = [EIGHT, EIGHT[::-1], *list(permutations(EIGHT))[1234::9000]]
    assert len(orders) >= 5
    for order in orders:
        outs = eight_planes(cam, s, order)
        torch.cuda.synchronize()
        for key in EIGHT:
            w = want[key]
            w = w.astype(np.uint8) if w.dtype == np.bool_ else w
            same(host(outs[key]), w if w.ndim == 3 else w[..., None], f"{key} in order {order}")
    with pytest.raises(ValueError, match="at most 8 planes, got 9"):
        U._launch(cam, [U._record(None, torch.empty(1), U._VALID)] * 9, None)


# ---- layouts -------------------------------------------------------------------------------------------------------------------------
def views(a):
    """the same values behind other strides: a window of a larger allocation, a transposed allocation, flipped channels"""
    t = dev(a)
    t3 = t if t.dim() == 3 else t[:, :, None]
    big = torch.zeros((t3.shape[0] + 3, t3.shape[1] + 5, t3.shape[2] + 1), dtype=t.dtype, device="cuda")
    big[2:-1, 4:-1, 1:] = t3
    out = {"window": big[2:-1, 4:-1, 1:], "transposed": t3.permute(1, 0, 2).contiguous().permute(1, 0, 2),
           "channel-flipped": torch.flip(t3, dims=(2,)).contiguous()}        # the allocation a negative channel stride reads
    return {k: (v if t.dim() == 3 else v[:, :, 0]) for k, v in out.items()}


@pytest.mark.parametrize("name", ["wide-37x53", f"half-{TH}x{TW}"])
def test_sliced_transposed_and_channel_flipped_sources_give_the_same_bytes(name):
    cam, want = camera(name), reference(name)
    src = sources(cam.source_size)
    for key, how in (("image", "linear"), ("panoptic", "nearest"), ("ids", "nearest")):
        v = views(src[key])
        for layout in ("window", "transposed"):
            assert not v[layout].is_contiguous() and torch.equal(v[layout], dev(src[key]))
            same(host(U.undistort_plane(v[layout], cam, how)), want[key], f"{key} as {layout}")
    # BGR as cv2 holds it: the RGB bytes read through a NEGATIVE channel stride.  torch refuses negative strides, so the record is
    # written by hand: the base points at the last channel of the flipped allocation, the channel stride is -1
    bgr = views(src["image"])["channel-flipped"]
    assert torch.equal(bgr.flip(2), dev(src["image"]))
    out = torch.empty(cam.size + (3,), dtype=torch.uint8, device="cuda")
    record = (bgr.data_ptr() + 2, out.data_ptr(), (bgr.stride(0), bgr.stride(1), -1), U._LINEAR, 1, 3, 0)
    U._launch(cam, [record], torch.cuda.current_stream().cuda_stream)
    same(host(out), want["image"], "image through a negative channel stride")
    # and rows from the bottom up: a negative row stride over a vertically flipped allocation
    rows = torch.flip(dev(src["panoptic"]), dims=(0,)).contiguous()
    out = torch.empty(cam.size + (3,), dtype=torch.uint8, device="cuda")
    h = cam.source_size[0]
    record = (rows.data_ptr() + (h - 1) * rows.stride(0), out.data_ptr(), (-rows.stride(0), rows.stride(1), 1), U._NEAREST, 1, 3, 0)
    U._launch(cam, [record], torch.cuda.current_stream().cuda_stream)
    same(host(out), want["panoptic"], "panoptic through a negative row stride")
    # a frame of windows, the ego mask as bool
    w = {k: views(src[k])["window"] for k in ("image", "panoptic", "semantic")}
    out = U.undistort_frame(cam, image=w["image"], ego_mask=dev(src["ego"] != 0), panoptic=w["panoptic"], semantic=w["semantic"][:, :, 0])
    same(host(out["image"]), want["image"], "image in a frame of windows")
    same(host(out["valid_mask"]), want["valid_ego"], "bool ego mask")
    same(host(out["panoptic"]), want["panoptic"], "panoptic in a frame of windows")
    same(host(out["semantic"]), want["semantic"][..., 0], "semantic [h, w] in a frame of windows")


def test_a_map_of_the_callers_replaces_the_closed_form():
    """the kernel's `map` argument: the camera is not read, the planes follow the given map (here another case's)"""
    cam, other = camera("wide-37x53"), "barrel-37x53"
    s = {k: dev(v) for k, v in sources(cam.source_size).items()}
    m = U.undistort_map(camera(other))
    out = torch.empty(cam.size + (3,), dtype=torch.uint8, device="cuda")
    valid = torch.empty(cam.size + (1,), dtype=torch.uint8, device="cuda")
    U._launch(cam, [U._record(s["image"], out, U._LINEAR, 3), U._record(None, valid, U._VALID)], torch.cuda.current_stream().cuda_stream, map=m)
    same(host(out), reference(other)["image"], "image through a given map")
    same(host(valid), reference(other)["valid"].astype(np.uint8), "valid through a given map")


# ---- one graph -----------------------------------------------------------------------------------------------------------------------
def test_a_captured_frame_replays_to_the_same_bytes_and_follows_its_camera():
    names = ("wide-37x53", "barrel-37x53")
    cams = [camera(n) for n in names]
    frames = [{k: dev(v) for k, v in sources((37, 53), seed).items()} for seed in (0, 5)]
    keys = ("image", "ego", "panoptic", "semantic")
    static = {k: frames[0][k].clone() for k in keys}
    cam = U.undistort_camera(size=(37, 53), **CASES[names[0]][2])            # its scalars are uploaded here, before the capture
    run = lambda: U.undistort_frame(cam, image=static["image"], ego_mask=static["ego"], panoptic=static["panoptic"],
                                    semantic=static["semantic"], image_float=True)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        run()
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        outs = run()
    for which, lens_at in ((1, 0), (0, 1), (0, 0)):
        for k in keys:
            static[k].copy_(frames[which][k])
        cam.params.copy_(cams[lens_at].params)                                 # the camera lives on the device: a replay follows it
        for o in outs.values():
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        K, D, new_K = map_arguments(cams[lens_at])
        src = sources((37, 53), (0, 5)[which])
        want = R.undistort_frame(K, D, new_K, (37, 53), image=src["image"], ego_mask=src["ego"], panoptic=src["panoptic"],
                                 semantic=src["semantic"], image_float=True)
        for key, w in want.items():
            same(host(outs[key]), w, f"replay of frame {which} through lens {names[lens_at]}: {key}")


# ---- the chain of a training frame ---------------------------------------------------------------------------------------------------
def test_decode_undistort_resize_and_masks_equal_the_chain_of_the_restatements():
    """a JPEG file -> decode_jpeg -> undistort_frame -> resize_frame / frame_masks, nothing on the host in between"""
    data = JPEG.read_bytes()
    pixels = JD.decode(data)
    assert pixels.shape == (48, 64, 3)
    src = sources((48, 64))
    size, labels = (18, 26), F.masked_labels(["vehicle"])
    cam = U.undistort_camera((58.0, 60.0, 32.3, 23.8), BARREL + (-0.052,), (48, 64), mode="optimal")
    K, D, new_K = map_arguments(cam)
    # the restatements
    u = R.undistort_frame(K, D, new_K, (48, 64), image=pixels, ego_mask=src["ego"], panoptic=src["panoptic"])
    assert 0.02 < 1.0 - u["valid_mask"].mean() < 0.9
    want = FR.resize_frame({"image": u["image"]}, *size, image_float=True)
    masks = FR.frame_masks(panoptic=u["panoptic"], valid=u["valid_mask"], labels=labels)
    want.update({k: FR.nearest(m, *size) for k, m in zip(("instance_map", "semantic_map", "mask"), masks)})
    # the device
    image = J.decode_jpeg(data)
    out = U.undistort_frame(cam, image=image, ego_mask=dev(src["ego"]), panoptic=dev(src["panoptic"]))
    got = F.resize_frame({"image": out["image"]}, size, image_float=True)
    inst, sem, mask = F.frame_masks(panoptic=out["panoptic"], valid=out["valid_mask"], labels=labels, size=size)
    got.update({"instance_map": inst, "semantic_map": sem, "mask": mask})
    torch.cuda.synchronize()
    same(host(image), pixels, "decoded pixels")
    same(host(out["image"]), u["image"], "undistorted image")
    for key, w in want.items():
        same(host(got[key]), w, key)
