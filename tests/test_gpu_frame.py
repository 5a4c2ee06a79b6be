"""mtgs_amd.frame on the device: byte for byte the NumPy restatement (tests/frame_refs.py) and Pillow's recorded outputs
(tests/golden/frame_ref.npz).  No tolerance anywhere: the 8-bit path is integer arithmetic, the float32 path rounds once per
operation, NEAREST is a gather.  Floats are compared as uint32 patterns; only in the non-finite case the payloads may differ and the
POSITIONS of the non-finite outputs are compared.  No input has more than 20 000 pixels; every reference is computed once per shape."""
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest
import torch

from mtgs_amd import frame as F
from tests import frame_refs as R

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden" / "frame_ref.npz"
TW, TH = F.TILE_W, F.TILE_H
# one below, at and one above the tile extents; more source rows than one chunk (130 -> 17: 4 chunks) with staged rows (150 -> 65:
# 3 * 150 bytes < MTGS_FRAME_RAW_ROW_BYTES) and with rows too long to stage (400 -> 65); a one-pixel input; no resize at all
EDGE_SHAPES = (((40, 150), (TH - 1, TW - 1)), ((40, 150), (TH, TW)), ((40, 150), (TH + 1, TW + 1)), ((130, 150), (TH + 1, TW + 1)),
               ((20, 400), (TH + 1, TW + 1)), ((1, 1), (3, 2)), ((1, 1), (1, 1)), ((37, 53), (37, 53)))
SHAPES = R.GOLDEN_SHAPES + EDGE_SHAPES
ids = lambda v: "x".join(map(str, v))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


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
def planes(shape, seed=0):
    """the five planes of a frame as the dataset holds them: image [H, W, 3], the others [H, W, 1]"""
    p = R.frame_inputs(seed, *shape)
    return {k: (v if k == "image" else v[:, :, None]) for k, v in p.items()}


@lru_cache(maxsize=None)
def reference(shape, size, seed=0):
    return R.resize_frame(planes(shape, seed), *size)


# ---- the resamplers against the restatement and against Pillow ------------------------------------------------------------------------
@pytest.mark.parametrize("shape, size", SHAPES, ids=ids)
def test_a_frame_is_the_restatement_byte_for_byte(shape, size, monkeypatch):
    """resize_frame on the full five-key dict: every plane equals the restatement, equals the per-plane call, non-tensor entries
    pass through, and the whole frame takes three launches"""
    data = {k: dev(v) for k, v in planes(shape).items()}
    data["image_idx"] = 7
    calls = []
    monkeypatch.setattr(F, "call", lambda name, *a, _call=F.call: (calls.append(name), _call(name, *a))[1])
    out = F.resize_frame(data, size)
    assert sorted(calls) == ["mtgs_frame_nearest", "mtgs_frame_resize_f32", "mtgs_frame_resize_u8"]
    as_float = F.resize_frame({"image": data["image"]}, size, image_float=True)["image"]
    torch.cuda.synchronize()
    want = reference(shape, size)
    assert out["image_idx"] == 7 and set(out) == set(data)
    for key, w in want.items():
        same(host(out[key]), w, key)
        resample = F.RESAMPLE_MAP[key]
        same(host(F.resize_plane(data[key], size, resample)), w, key + " alone")
        same(host(F.resize_plane(data[key][..., 0], size, resample)) if key != "image" else w, w[..., 0] if key != "image" else w, key + " [H, W]")
    # get_gt_img folded in: one correctly rounded division per byte
    same(host(as_float), R.to_float(want["image"]), "image_float")
    same(host(as_float), (out["image"].cpu().float() / 255).numpy(), "image_float against torch on the host")
    same(host(F.resize_plane(data["image"], size, out_dtype=torch.float32)), R.to_float(want["image"]), "out_dtype")
    gray = np.ascontiguousarray(planes(shape)["image"][:, :, 1])
    same(host(F.resize_plane(dev(gray), size)), R.bilinear_u8(gray, *size), "one channel")
    same(host(F._bilinear(data["image"], *size, two_pass=True)), want["image"], "two launches")
    same(host(F._bilinear(data["depth"], *size, two_pass=True)), want["depth"], "two launches, float32")


def test_the_recorded_pillow_outputs():
    g = np.load(GOLDEN)
    seed = int(g["seed"])
    for (h, w), size in R.GOLDEN_SHAPES:
        p, name = R.frame_inputs(seed, h, w), f"{h}x{w}_{size[0]}x{size[1]}"
        assert R.checksum(p) == int(g[f"{name}/crc"])
        out = F.resize_frame({k: dev(v) for k, v in p.items()}, size)
        torch.cuda.synchronize()
        for key in p:
            same(host(out[key]), g[f"{name}/{key}"], f"{name}/{key}")


def test_three_channel_nearest_and_int32_channels():
    p = planes((37, 53))
    rgb, inst = p["image"], np.concatenate([p["instance_map"], p["instance_map"][::-1] + 1], axis=2)
    same(host(F.resize_plane(dev(rgb), (18, 26), "nearest")), R.nearest(rgb, 18, 26), "uint8 x 3")
    same(host(F.resize_plane(dev(inst), (46, 70), "nearest")), R.nearest(inst, 46, 70), "int32 x 2")


def test_non_finite_depths_stay_where_pillow_puts_them():
    depth = R.frame_inputs(3, 37, 53)["depth"].copy()
    depth[5, 7], depth[20, 30], depth[36, 52] = np.nan, np.inf, -np.inf
    for size in ((18, 26), (46, 70), (37, 26)):
        got, want = host(F.resize_plane(dev(depth), size)), R.bilinear_f32(depth, *size)
        finite = np.isfinite(want)
        assert (~finite).any() and np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isposinf(got), np.isposinf(want))
        assert np.array_equal(np.isneginf(got), np.isneginf(want))
        same(np.where(finite, got, np.float32(0)), np.where(finite, want, np.float32(0)), f"finite part at {size}")


# ---- layouts --------------------------------------------------------------------------------------------------------------------------
def views(a):
    """the same values as device views that are not contiguous: an offset window of a larger buffer (rows that start at every
    byte alignment), every second column of a wider buffer, and (three channels) a planar [C, H, W] buffer"""
    h, w = a.shape[:2]
    big = np.zeros((h + 3, w + 5) + a.shape[2:], a.dtype)
    big[2:2 + h, 3:3 + w] = a
    wide = np.zeros((h, 2 * w) + a.shape[2:], a.dtype)
    wide[:, ::2] = a
    out = {"window": dev(big)[2:2 + h, 3:3 + w], "columns": dev(wide)[:, ::2]}
    if a.ndim == 3 and a.shape[2] == 3:
        out["planar"] = dev(a.transpose(2, 0, 1)).permute(1, 2, 0)
    return out


@pytest.mark.parametrize("shape, size", [((37, 53), (18, 26)), ((37, 53), (37, 39)), ((40, 150), (TH + 1, TW + 1))], ids=ids)
def test_strided_and_offset_views_give_the_same_bytes(shape, size):
    want = reference(shape, size)
    for key, a in planes(shape).items():
        for name, v in views(a).items():
            assert not v.is_contiguous() and torch.equal(v, dev(a))
            same(host(F.resize_plane(v, size, F.RESAMPLE_MAP[key])), want[key], f"{key} as {name}")
    data = {k: views(a)["window"] for k, a in planes(shape).items()}
    out = F.resize_frame(data, size, image_float=True)
    for key in data:
        same(host(out[key]), R.to_float(want[key]) if key == "image" else want[key], f"{key} in a frame of windows")


# ---- the masks ------------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def panoptic_inputs(shape=(37, 53)):
    rng = np.random.default_rng(11)
    pan = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    pan[:, :, 2] = R.frame_inputs(0, *shape)["semantic_map"]
    return pan, rng.random(shape + (1,)) < 0.8


@pytest.mark.parametrize("labels", [F.masked_labels(["vehicle"]), F.masked_labels((), True), (), tuple(range(256))], ids=["vehicle", "foreground", "none", "all"])
@pytest.mark.parametrize("size", [None, (18, 26), (46, 70)], ids=["full", "down", "up"])
def test_frame_masks_equal_prepare_then_resize(labels, size):
    pan, ok = panoptic_inputs()
    oh, ow = size or pan.shape[:2]
    for use_panoptic in (True, False):
        for valid in (None, ok):
            src = {"panoptic": pan} if use_panoptic else {"semantic": pan[:, :, 2:3]}
            want = [None if m is None else R.nearest(m, oh, ow) for m in R.frame_masks(valid=valid, labels=labels, **src)]
            got = F.frame_masks(valid=None if valid is None else dev(valid), labels=labels, size=size, **{k: dev(v) for k, v in src.items()})
            assert (got[0] is None) == (not use_panoptic)
            for g, w, what in zip(got, want, ("instance_map", "semantic_map", "mask")):
                if w is not None:
                    same(host(g), w, f"{what} panoptic={use_panoptic} valid={valid is not None}")
            mask = host(got[2])
            if len(labels) == 256:
                assert not mask.any()
            if len(labels) == 0:
                assert np.array_equal(mask, np.ones_like(mask) if valid is None else R.nearest(ok, oh, ow))
    # views: the semantic channel of a panoptic map as a [H, W] map, a uint8 valid mask [H, W]
    inst, sem, mask = F.frame_masks(semantic=dev(pan)[:, :, 2], valid=dev(ok[..., 0].astype(np.uint8)), labels=labels, size=size)
    want = R.frame_masks(semantic=pan[:, :, 2], valid=ok, labels=labels)
    assert inst is None
    same(host(sem), R.nearest(want[1], oh, ow), "semantic view")
    same(host(mask), R.nearest(want[2], oh, ow), "mask view")


def test_the_prepared_masks_are_the_planes_of_a_frame():
    """frame_masks at full size, then resize_frame: the reference's own order gives the bytes of the fused call"""
    pan, ok = panoptic_inputs()
    labels = F.masked_labels(["vehicle", "pedestrian"])
    inst, sem, mask = F.frame_masks(panoptic=dev(pan), valid=dev(ok), labels=labels)
    two_steps = F.resize_frame({"instance_map": inst, "semantic_map": sem, "mask": mask}, (27, 39))
    fused = F.frame_masks(panoptic=dev(pan), valid=dev(ok), labels=labels, size=(27, 39))
    for key, g in zip(("instance_map", "semantic_map", "mask"), fused):
        assert torch.equal(two_steps[key], g) and g.shape == (27, 39, 1)
    assert mask.dtype == torch.bool and inst.dtype == torch.int32 and sem.dtype == torch.uint8


# ---- one graph --------------------------------------------------------------------------------------------------------------------------
def test_a_captured_frame_replays_to_the_same_bytes():
    shape, size = (37, 53), (27, 39)
    frames = [{k: dev(v) for k, v in planes(shape, seed).items()} for seed in (0, 5)]
    wants = [R.resize_frame(planes(shape, seed), *size, image_float=True) for seed in (0, 5)]
    static = {k: v.clone() for k, v in frames[0].items()}
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        F.resize_frame(static, size, image_float=True)          # the tables are uploaded here, before the capture
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        outs = F.resize_frame(static, size, image_float=True)
    for which in (1, 0, 0):
        for k, v in frames[which].items():
            static[k].copy_(v)
        for o in outs.values():
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for key, w in wants[which].items():
            same(host(outs[key]), w, f"replay of frame {which}: {key}")
