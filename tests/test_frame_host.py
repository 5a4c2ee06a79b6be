"""mtgs_amd.frame without a GPU: the NumPy restatement (tests/frame_refs.py) against Pillow itself and against Pillow's recorded
outputs (tests/golden/frame_ref.npz), byte for byte -- floats as uint32 views --, the host tables against weights recomputed
independently, the label list, the size rule and the refusals."""
from pathlib import Path

import numpy as np
import pytest
import torch

from mtgs_amd import dino, frame as F
from tests import frame_refs as R

GOLDEN = Path(__file__).resolve().parent / "golden" / "frame_ref.npz"
PILLOW_SHAPES = (((37, 53), (18, 26)), ((37, 53), (27, 39)), ((64, 100), (64, 50)), ((31, 47), (46, 70)), ((540, 960), (405, 720)),
                 ((5, 7), (1, 1)), ((9, 9), (9, 4)), ((9, 9), (4, 9)), ((1, 1), (3, 2)))


def bits(a):
    """what is compared: the bytes of an array (a float32 as its uint32 pattern)"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint8) if a.dtype == np.bool_ else a


@pytest.mark.parametrize("shape, size", PILLOW_SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_the_restatement_is_pillow_byte_for_byte(shape, size):
    Image = pytest.importorskip("PIL.Image")
    planes, (oh, ow) = R.frame_inputs(1, *shape), size
    mine = R.resize_frame(planes, oh, ow)
    planes["gray"] = planes["image"][:, :, 1].copy()
    mine["gray"] = R.bilinear_u8(planes["gray"], oh, ow)
    for key, x in planes.items():
        resample = Image.Resampling.BILINEAR if key in ("image", "depth", "gray") else Image.Resampling.NEAREST
        got = np.array(Image.fromarray(x).resize((ow, oh), resample=resample), dtype=x.dtype)
        got = got.view(np.uint8) != 0 if x.dtype == np.bool_ else got
        assert got.dtype == mine[key].dtype and got.shape == mine[key].shape, key
        assert np.array_equal(bits(got), bits(mine[key])), key


def test_the_restatement_is_the_recorded_pillow():
    """no skip: the recorded outputs of Pillow 12.2.0 travel with the repository"""
    g = np.load(GOLDEN)
    assert str(g["pillow"]) == "12.2.0" and GOLDEN.stat().st_size < 100_000
    seed = int(g["seed"])
    for (h, w), (oh, ow) in R.GOLDEN_SHAPES:
        assert h * w <= 64 * 100
        planes, name = R.frame_inputs(seed, h, w), f"{h}x{w}_{oh}x{ow}"
        assert R.checksum(planes) == int(g[f"{name}/crc"]), "the random stream changed: the inputs are not the recorded ones"
        mine = R.resize_frame(planes, oh, ow)
        for key in planes:
            want = g[f"{name}/{key}"]
            assert want.dtype == mine[key].dtype and want.shape == mine[key].shape == ((oh, ow, 3) if key == "image" else (oh, ow))
            assert np.array_equal(bits(want), bits(mine[key])), (name, key)


def test_the_inputs_have_the_edges_the_kernels_can_get_wrong():
    p = R.frame_inputs(0, 37, 53)
    img = p["image"]
    assert (img[:12, :17] == 0).all() and (img[25:, 36:] == 255).all()
    band = img[12:25, :26, 0].astype(int)
    assert set(np.unique(band)) == {0, 255} and (np.abs(np.diff(band, axis=1)) == 255).all() and (np.abs(np.diff(band, axis=0)) == 255).all()
    assert (p["depth"] == 0).mean() > 0.1 and p["depth"].max() > 5e4 and p["depth"].min() >= 0
    assert (p["semantic_map"] == 255).any() and p["instance_map"].max() > 1 << 16 and p["mask"].dtype == np.bool_


@pytest.mark.parametrize("n_in, n_out", [(53, 26), (37, 27), (47, 70), (7, 1), (400, 3), (1, 3), (960, 720), (9, 9)])
def test_the_host_tables_are_the_weights_recomputed(n_in, n_out):
    """dino.bilinear_weights (the float32 path's doubles, not quantised), dino.bilinear_coefficients (22 bits) and
    dino.nearest_sources against the restatement's own loops"""
    bounds, w = dino.bilinear_weights(n_in, n_out, 0, n_out)
    bounds_q, q = dino.bilinear_coefficients(n_in, n_out, 0, n_out)
    ref, ref_q = R.weights(n_in, n_out), R.coefficients(n_in, n_out)
    assert w.dtype == np.float64 and q.dtype == np.int32 and bounds.dtype == np.int32 and np.array_equal(bounds, bounds_q)
    assert w.shape == q.shape == (n_out, max(len(k) for _, k in ref))
    for j, ((xmin, k), (_, kq)) in enumerate(zip(ref, ref_q)):
        assert tuple(bounds[j]) == (xmin, len(k))
        assert np.array_equal(w[j, :len(k)].view(np.uint64), np.array(k, np.float64).view(np.uint64)) and not w[j, len(k):].any()
        assert q[j, :len(k)].tolist() == kq and not q[j, len(k):].any()
        assert abs(sum(k) - 1.0) < 1e-12 and abs(sum(kq) - (1 << 22)) <= len(kq)
    assert np.array_equal(dino.nearest_sources(n_in, n_out, 0, n_out), R.nearest_index(n_in, n_out))
    if (n_in, n_out) == (400, 3):
        assert max(len(k) for _, k in ref) == 266                       # of Pillow's ksize = 269: the tap count has no bound


def test_masked_labels():
    assert F.masked_labels() == (255,) and F.masked_labels((), False) == (255,)
    assert F.masked_labels(["pedestrian"]) == (255, 11)
    assert F.masked_labels(["bicycle"]) == (255, 18, 17, 12)
    assert F.masked_labels(["vehicle"]) == (255, 13, 14, 15)
    assert F.masked_labels(("vehicle", "pedestrian")) == (255, 11, 13, 14, 15)
    assert F.masked_labels((), True) == F.masked_labels(["pedestrian", "bicycle", "vehicle"]) == (255, 11, 18, 17, 12, 13, 14, 15)
    assert F.masked_labels(["sky"]) == (255,)
    table = F.label_bits(F.masked_labels((), True))
    assert table.dtype == np.uint8 and table.shape == (32,)
    assert [l for l in range(256) if table[l >> 3] >> (l & 7) & 1] == [11, 12, 13, 14, 15, 17, 18, 255]
    assert not F.label_bits(()).any() and (F.label_bits(range(256)) == 255).all()
    for bad in (256, -1, 1.5, True):
        with pytest.raises(ValueError, match="labels must be integers"):
            F.label_bits([bad])


def test_scaled_size_floors():
    assert F.scaled_size(1080, 1920, 0.5) == (540, 960) and F.scaled_size(1080, 1920, 0.75) == (810, 1440)
    assert F.scaled_size(37, 53, 0.5) == (18, 26) and F.scaled_size(37, 53, 0.75) == (27, 39) and F.scaled_size(37, 53, 1.0) == (37, 53)
    assert F.scaled_size(5, 7, 0.99) == (4, 6) and F.scaled_size(3, 3, 1.5) == (4, 4)
    for bad in ((0, 5, 1.0), (5, 5, 0.0), (5, 5, -1.0), (5, 5, float("nan")), (1, 9, 0.5)):
        with pytest.raises(ValueError):
            F.scaled_size(*bad)
    assert "RECALLED" in F.scaled_size.__doc__


def test_the_refusals_come_before_the_device():
    img, depth = torch.zeros(5, 7, 3, dtype=torch.uint8), torch.zeros(5, 7, 1)
    with pytest.raises(NotImplementedError, match="4 channels.*RGBA"):
        F.resize_plane(torch.zeros(5, 7, 4, dtype=torch.uint8), (2, 2))
    with pytest.raises(NotImplementedError, match="2 channels"):
        F.resize_plane(torch.zeros(5, 7, 2, dtype=torch.uint8), (2, 2))
    with pytest.raises(NotImplementedError, match="float32 with 3 channels"):
        F.resize_plane(torch.zeros(5, 7, 3), (2, 2))
    with pytest.raises(NotImplementedError, match="4 channels"):
        F.resize_plane(torch.zeros(5, 7, 4, dtype=torch.int32), (2, 2), "nearest")
    for size in ((0, 3), (3, 0), (-1, 2), (2,), (2.0, 2), None, 4):
        with pytest.raises(ValueError, match="size must be"):
            F.resize_plane(img, size)
        with pytest.raises(ValueError, match="size must be"):
            F.resize_frame({"image": img}, size)
    with pytest.raises(ValueError, match=r"size must be at most"):
        F.resize_plane(img, (F.MAX_SIZE + 1, 2))
    with pytest.raises(ValueError, match="resample must be"):
        F.resize_plane(img, (2, 2), "bicubic")
    with pytest.raises(TypeError, match="x must be uint8 or float32, got torch.int32"):
        F.resize_plane(torch.zeros(5, 7, dtype=torch.int32), (2, 2))
    with pytest.raises(TypeError, match="x must be uint8 or int32 or bool, got torch.float32"):
        F.resize_plane(depth, (2, 2), "nearest")
    with pytest.raises(ValueError, match=r"x must be \[H, W\] or \[H, W, C\], got \(5,\)"):
        F.resize_plane(torch.zeros(5), (2, 2))
    with pytest.raises(ValueError, match="at least one pixel"):
        F.resize_plane(torch.zeros(0, 7, dtype=torch.uint8), (2, 2))
    with pytest.raises(ValueError, match="out_dtype"):
        F.resize_plane(depth, (2, 2), out_dtype=torch.uint8)
    with pytest.raises(ValueError, match="out_dtype"):
        F.resize_plane(img, (2, 2), "nearest", out_dtype=torch.float32)
    with pytest.raises(KeyError, match="normals"):
        F.resize_frame({"image": img, "normals": depth}, (2, 2))
    with pytest.raises(ValueError, match="one of the two"):
        F.frame_masks()
    with pytest.raises(ValueError, match="one of the two"):
        F.frame_masks(panoptic=img, semantic=img[..., 0])
    with pytest.raises(NotImplementedError, match="panoptic has 1 channels"):
        F.frame_masks(panoptic=img[..., :1])
    with pytest.raises(ValueError, match=r"valid must be \[5, 7\]"):
        F.frame_masks(panoptic=img, valid=torch.ones(5, 6, dtype=torch.bool))
    with pytest.raises(ValueError, match="labels must be integers"):
        F.frame_masks(panoptic=img, labels=[300])
    # a CPU tensor is refused as everywhere in the package, after the argument checks
    for run in (lambda: F.resize_plane(img, (2, 2)), lambda: F.resize_plane(depth, (2, 2)), lambda: F.resize_plane(img, (2, 2), "nearest"),
                lambda: F.resize_frame({"image": img, "depth": depth, "image_idx": 3}, (2, 2)), lambda: F.frame_masks(panoptic=img),
                lambda: F.frame_masks(semantic=img[..., 0], valid=torch.ones(5, 7, dtype=torch.bool), size=(2, 2))):
        with pytest.raises(RuntimeError, match="must live on the HIP device"):
            run()


def test_the_module_is_exported_and_reads_its_constants_from_the_header():
    import mtgs_amd
    from mtgs_amd import _abi
    for name in ("resize_plane", "resize_frame", "frame_masks", "masked_labels", "scaled_size"):
        assert getattr(mtgs_amd, name) is getattr(F, name) and name in mtgs_amd.__all__
    c = _abi.header_abi("mtgs_frame.h").constants
    assert (F.TILE_W, F.TILE_H, F.CHUNK_ROWS, F.MAX_PLANES) == (c["MTGS_FRAME_TILE_W"], c["MTGS_FRAME_TILE_H"], c["MTGS_FRAME_CHUNK_ROWS"],
                                                               c["MTGS_FRAME_MAX_PLANES"])
    assert F.RESAMPLE_MAP == {"image": "bilinear", "depth": "bilinear", "mask": "nearest", "semantic_map": "nearest", "instance_map": "nearest"}
    assert dino.bilinear_coefficients is F.bilinear_coefficients and dino.nearest_sources is F.nearest_sources
    assert "(width, height)" in F.resize_plane.__doc__


def test_the_launchers_name_the_bad_argument(hip_lib):
    import ctypes as C
    err = lambda: hip_lib.mtgs_rast_last_error().decode()
    one = C.c_void_p(16)
    assert hip_lib.mtgs_frame_resize_u8(0, 4, 3, one, 12, 3, 1, 2, 2, one, one, 3, one, one, 3, 0, one, None) == 1 and "h outside" in err()
    assert hip_lib.mtgs_frame_resize_u8(4, 4, 4, one, 16, 4, 1, 2, 2, one, one, 3, one, one, 3, 0, one, None) == 4 and "c outside [1, 3] (4)" in err()
    assert hip_lib.mtgs_frame_resize_u8(4, 4, 3, None, 12, 3, 1, 2, 2, one, one, 3, one, one, 3, 0, one, None) == 1 and "null pointer: src" in err()
    assert hip_lib.mtgs_frame_resize_u8(4, 4, 3, one, 12, 3, 1, 2, 2, None, one, 3, one, one, 3, 0, one, None) == 1 and "null pointer: hb" in err()
    assert hip_lib.mtgs_frame_resize_u8(4, 4, 3, one, 12, 3, 1, 2, 4, None, None, 0, one, one, 0, 0, one, None) == 1 and "vk < 1" in err()
    assert hip_lib.mtgs_frame_resize_f32(4, 4, 1, C.c_void_p(18), 4, 1, 1, 2, 2, one, one, 3, one, one, 3, one, None) == 1 and "src must be 4-byte aligned" in err()
    assert hip_lib.mtgs_frame_resize_f32(4, 4, 1, one, 4, 1, 1, 2, 1 << 21, one, one, 3, one, one, 3, one, None) == 1 and "ow outside" in err()
    plane = np.zeros(1, dtype=F._PLANE)
    args = lambda n=1: (4, 4, 2, 2, one, one, n, plane.ctypes.data, None, None)
    assert hip_lib.mtgs_frame_nearest(*args(0)) == 1 and "n_planes outside [1, 8] (0)" in err()
    assert hip_lib.mtgs_frame_nearest(*args()) == 1 and "null pointer: planes[0].src" in err()
    plane["src"], plane["dst"], plane["op"] = 16, 16, 7
    assert hip_lib.mtgs_frame_nearest(*args()) == 1 and "planes[0].op unknown (7)" in err()
    plane["op"], plane["elem_bytes"], plane["channels"] = 0, 2, 1
    assert hip_lib.mtgs_frame_nearest(*args()) == 4 and "elem_bytes must be 1 or 4 (2)" in err()
    plane["elem_bytes"], plane["channels"] = 4, 4
    assert hip_lib.mtgs_frame_nearest(*args()) == 4 and "channels outside [1, 3] (4)" in err()
    plane["channels"], plane["dst"] = 1, 18
    assert hip_lib.mtgs_frame_nearest(*args()) == 1 and "planes[0].dst must be 4-byte aligned" in err()
    assert hip_lib.mtgs_frame_nearest(4, 4, 2, 2, None, one, 1, plane.ctypes.data, None, None) == 1 and "null pointer: sy" in err()
