"""mtgs_amd.brightness without a GPU: the NumPy restatement (tests/brightness_refs.py) against known answers that hold whatever
OpenCV does, the estimate's restatement against the reference's own record (tests/golden/brightness_ref.npz), NumPy's summation
order, the argument checks, the pair-table builder and the ABI record."""
import colorsys
import ctypes as C

import numpy as np
import pytest
import torch

from tests import brightness_refs as B


@pytest.fixture(scope="module")
def all_colours():
    """every 8-bit colour once, [2^24, 3] (r, g, b), with its HSV and its adjusted colour at factor 1.3"""
    i = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.stack([(i >> 16) & 255, (i >> 8) & 255, i & 255], axis=-1).astype(np.uint8)
    return rgb, B.adjust_brightness(rgb.reshape(4096, 4096, 3), 1.3).reshape(-1, 3)


def test_tables_are_the_rounded_quotients():
    sdiv, hdiv = B.tables()
    assert sdiv[0] == hdiv[0] == 0 and sdiv[255] == 4096 and sdiv[1] == 255 << 12 and hdiv[1] == 122880
    assert hdiv[255] == 482 and sdiv[2] == 522240 and hdiv[4] == 30720
    # a tie of the double quotient goes to the even neighbour: 1044480 / 256 has none, 737280 / (6 * 5) = 24576 exactly
    assert hdiv[5] == 24576


def test_every_colour_h_below_180_s_at_most_255_and_the_largest_channel_is_v(all_colours):
    rgb, out = all_colours
    for at in range(0, rgb.shape[0], 1 << 22):
        h, s, v = B.rgb_to_hsv(rgb[at:at + (1 << 22)])
        assert h.min() >= 0 and h.max() < 180 and s.min() >= 0 and s.max() <= 255
        assert np.array_equal(v, rgb[at:at + (1 << 22)].max(axis=-1))
        assert np.array_equal(out[at:at + (1 << 22)].max(axis=-1), B.scale_v(v, 1.3))


def test_factor_one_is_not_the_identity_but_stays_close():
    rng = np.random.default_rng(0)
    rgb = rng.integers(0, 256, (200000, 3), dtype=np.uint8)
    out = B.adjust_brightness(rgb[None], 1.0)[0]
    diff = np.abs(out.astype(int) - rgb.astype(int))
    same = float((diff.max(axis=-1) == 0).mean())
    assert 0.2 < same < 0.45 and diff.max() <= 5, (same, diff.max())
    assert np.array_equal(out.max(axis=-1), rgb.max(axis=-1))


def test_grays_primaries_black_and_saturation():
    gray = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)[None]
    for factor in (0.0, 0.4, 1.0, 1.7, 300.0):
        out = B.adjust_brightness(gray, factor)[0]
        want = np.trunc(np.clip(np.arange(256) * factor, 0, 255)).astype(np.uint8)
        assert np.array_equal(out, np.repeat(want[:, None], 3, axis=1)), factor
    primaries = np.array([[255, 0, 0], [255, 255, 0], [0, 255, 0], [0, 255, 255], [0, 0, 255], [255, 0, 255]], dtype=np.uint8)
    h, s, v = B.rgb_to_hsv(primaries)
    assert h.tolist() == [0, 30, 60, 90, 120, 150] and s.tolist() == [255] * 6 and v.tolist() == [255] * 6
    assert np.array_equal(B.adjust_brightness(primaries[None], 1.0)[0], primaries)
    rng = np.random.default_rng(1)
    rgb = rng.integers(0, 256, (1, 5000, 3), dtype=np.uint8)
    assert not B.adjust_brightness(rgb, 0.0).any()
    for factor in (255.0, 1e300, np.inf):
        out = B.adjust_brightness(rgb, factor)[0]
        assert np.array_equal(out.max(axis=-1), np.where(rgb[0].max(axis=-1) > 0, 255, 0)), factor
    assert not B.adjust_brightness(rgb, np.nan).any()                    # the defined deviation
    assert not B.adjust_brightness(rgb, 1e-310).any()
    assert not B.adjust_brightness(np.zeros((1, 4, 3), np.uint8), np.inf).any()         # 0 * inf is NaN: 0


def test_bgr_is_rgb_on_the_reversed_image_and_factors_go_per_image():
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (3, 5, 7, 3), dtype=np.uint8)
    fac = np.array([0.5, 1.0, 2.5])
    assert np.array_equal(B.adjust_brightness(img, fac, "bgr"), B.adjust_brightness(img[..., ::-1], fac, "rgb")[..., ::-1])
    for c in range(3):
        assert np.array_equal(B.adjust_brightness(img, fac)[c], B.adjust_brightness(img[c], fac[c]))


def test_hue_agrees_with_colorsys_within_one_unit():
    rng = np.random.default_rng(3)
    rgb = rng.integers(0, 256, (4000, 3), dtype=np.uint8)
    rgb = rgb[rgb.max(axis=1) - rgb.min(axis=1) >= 16]                   # a hue needs some chroma to be defined to a unit
    h = B.rgb_to_hsv(rgb)[0]
    want = np.array([colorsys.rgb_to_hsv(*(c / 255.0))[0] * 180.0 for c in rgb])
    err = np.abs(h - want)
    err = np.minimum(err, 180.0 - err)
    assert err.max() <= 1.0, err.max()


def test_numpy_sum_is_numpys_order():
    rng = np.random.default_rng(4)
    for n in list(range(1, 41)) + [127, 128]:
        for _ in range(20):
            a = rng.uniform(0.0, 1.0, n) * 10.0 ** rng.integers(-8, 8, n)
            assert B.numpy_sum(a) == np.add.reduce(a) and B.numpy_sum(a) / np.float64(n) == np.mean(list(a)), n
    a = np.arange(8, dtype=np.float64)
    assert B.numpy_sum(a) == ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]))


def test_the_estimate_reproduces_the_references_record():
    g = B.golden()
    assert [tuple(r) for r in g["pairs"].tolist()] == list(B.NUPLAN_PAIRS)
    assert g["cameras"].tolist() == ["CAM_F0", "CAM_L0", "CAM_R0", "CAM_L1", "CAM_R1", "CAM_L2", "CAM_R2", "CAM_B0"]
    factors, stats = B.estimate_factors(g["points"], g["lidar2imgs"], g["images"])
    h, w = g["images"].shape[1:3]
    overlap = stats[:, 0] >= 10
    assert overlap.sum() >= 3 and (~overlap).sum() >= 2
    used = np.stack([g["used_count"], g["used_s1"], g["used_s2"]], axis=1)
    want = np.where(overlap[:, None], stats[:, :3], np.concatenate([np.full((8, 1), h * min(100, w)), stats[:, 3:]], axis=1))
    assert np.array_equal(want, used)
    assert np.array_equal(factors.view(np.int64), g["factors"].view(np.int64))
    assert abs(np.mean(factors) - 1.0) < 1e-15


def test_the_chain_branches():
    """base 1.0 for a cam1 without a factor, the average for a second visit, 1.0 for a camera no pair reaches, inf and NaN"""
    stats = np.array([[20, 300, 100, 0, 0], [20, 100, 400, 0, 0], [0, 0, 0, 50, 25]], dtype=np.int64)
    raw = lambda pairs, **kw: B.solve_factors(stats[:len(pairs)], 4, 2, 5, pairs, **kw)
    f = raw(((1, 2, 0),))                                   # camera 1 has no factor: base 1.0; cameras 0 and 3 keep 1.0
    assert np.allclose(f / f[0], [1, 1, 3, 1], rtol=1e-15) and f[0] == 1.0 / 1.5
    f = raw(((0, 2, 0), (1, 2, 1)))                         # camera 2 twice: (3 + 0.25) / 2
    assert np.allclose(f / f[0], [1, 1, 1.625, 1], rtol=1e-15)
    f = raw(((0, 1, 0), (0, 2, 0), (0, 3, 0)), min_overlap=10)      # the third pair falls back to the strips: 50 / 25
    assert np.allclose(f / f[0], [1, 3, 0.25, 2], rtol=1e-15)
    black = np.array([[0, 0, 0, 7, 0], [0, 0, 0, 0, 0]], dtype=np.int64)
    f = B.solve_factors(black, 3, 2, 5, ((0, 1, 0), (0, 2, 0)))
    assert np.isnan(f).all()                                # inf and NaN among the factors: the mean is NaN, as the reference's is
    f = B.solve_factors(black[:1], 2, 2, 5, ((0, 1, 0),))
    assert f[0] == 0.0 and np.isnan(f[1])                   # 1 / inf and inf / inf


def test_strip_columns_are_pythons_slices():
    for w in (40, 100, 101, 199, 250):
        for strip in (1, 100):
            assert list(B.strip_columns(w, strip, True)) == list(range(w))[:strip]
            assert list(B.strip_columns(w, strip, False)) == list(range(w))[-strip:]


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------
def test_pair_table_builder():
    from mtgs_amd import brightness as M
    t = M.pair_table(M.NUPLAN_PAIRS, 8)
    assert t.dtype == np.int32 and t.shape == (8, 3) and t.flags.c_contiguous and [tuple(r) for r in t.tolist()] == list(B.NUPLAN_PAIRS)
    assert M.NUPLAN_PAIRS == B.NUPLAN_PAIRS and len(M.NUPLAN_CAMERAS) == 8
    names = {n: i for i, n in enumerate(M.NUPLAN_CAMERAS)}
    assert [(names[a], names[b]) for a, b in (("CAM_F0", "CAM_L0"), ("CAM_F0", "CAM_R0"), ("CAM_L0", "CAM_L1"), ("CAM_R0", "CAM_R1"),
                                              ("CAM_L1", "CAM_L2"), ("CAM_R1", "CAM_R2"), ("CAM_L2", "CAM_B0"), ("CAM_R2", "CAM_B0"))] \
        == [(a, b) for a, b, _ in M.NUPLAN_PAIRS]
    assert [s for _, _, s in M.NUPLAN_PAIRS] == [0, 1, 0, 1, 0, 1, 0, 1]
    assert M.pair_table(torch.tensor([[1, 0, 1]]), 2).tolist() == [[1, 0, 1]]
    for bad, match in (([(0, 8, 0)], r"pairs\[0\].*outside \[0, 8\)"), ([(0, 1, 0), (2, 2, 0)], r"pairs\[1\].*twice"),
                       ([(0, 1, 2)], r"pairs\[0\].*side 2"), ([(0, 1)], "pairs must be"), ([], "pairs must be"),
                       ([(0.5, 1, 0)], "pairs must be"), ([(-1, 1, 0)], r"pairs\[0\].*outside"),
                       ([(0, 1, 0)] * (M.MAX_PAIRS + 1), "1 to 64 rows")):
        with pytest.raises(ValueError, match=match):
            M.pair_table(bad, 8)


def test_adjust_brightness_refusals_name_the_argument():
    from mtgs_amd import brightness as M
    img = torch.zeros((2, 4, 5, 3), dtype=torch.uint8)
    f = torch.ones(2, dtype=torch.float64)
    for args, kw, exc, match in (
            ((img.float(), 1.0), {}, TypeError, "images must be uint8"),
            ((img[..., 0], 1.0), {}, ValueError, r"images must be \[h, w, 3\]"),
            ((torch.zeros((4, 5, 4), dtype=torch.uint8), 1.0), {}, NotImplementedError, "RGBA"),
            ((img[:0], 1.0), {}, ValueError, "at least one image"),
            ((img, 1.0), {"channel_order": "hsv"}, ValueError, "channel_order"),
            ((img, "1.0"), {}, TypeError, "factors must be a Python float or a device float64 tensor"),
            ((img, True), {}, TypeError, "factors"),
            ((img, f.float()), {}, TypeError, "factors must be float64"),
            ((img, torch.ones(3, dtype=torch.float64)), {}, ValueError, r"factors must be \[C\] with C = 2"),
            ((img, torch.ones((2, 1), dtype=torch.float64)), {}, ValueError, "factors must be"),
            ((img, 1.0), {"out": torch.zeros((2, 4, 5, 3))}, ValueError, "out must be a contiguous torch.uint8"),
            ((img, 1.0), {"out": torch.zeros((2, 4, 5, 3), dtype=torch.uint8), "image_float": True}, ValueError, "out must be a contiguous torch.float32"),
            ((img, 1.0), {"out": torch.zeros((2, 4, 6, 3), dtype=torch.uint8)[:, :, :5]}, ValueError, "out must be a contiguous"),
            ((img, 1.0), {"out": img}, ValueError, "out overlaps images"),
            ((img[None][0], 1.0), {"out": img.view(2, 4, 5, 3)}, ValueError, "out overlaps images")):
        with pytest.raises(exc, match=match):
            M.adjust_brightness(*args, **kw)
    with pytest.raises(RuntimeError, match="HIP device"):          # everything is in order but the device: no CPU fallback
        M.adjust_brightness(img, 1.0)
    big = torch.zeros((4, 6, 8, 3), dtype=torch.uint8)
    window = big[1:3, 1:5, 2:7]                               # an out behind a window of the images' allocation overlaps too
    assert M._extent(window) == (window.data_ptr(), window[-1, -1, -1, -1].data_ptr() + 1)
    flat = torch.zeros(2 * 4 * 9 * 3, dtype=torch.uint8)
    padded = flat.view(2, 4, 9, 3)[:, :, :5]                   # row-padded images; an out in the same allocation overlaps their span
    with pytest.raises(ValueError, match="out overlaps images"):
        M.adjust_brightness(padded, 1.0, out=flat[60:180].view(2, 4, 5, 3))


def test_estimate_refusals_name_the_argument():
    from mtgs_amd import brightness as M
    pts, mats = torch.zeros((5, 3)), torch.zeros((8, 4, 4), dtype=torch.float64)
    img = torch.zeros((8, 4, 5, 3), dtype=torch.uint8)
    for args, kw, exc, match in (
            ((pts[:, :2], mats, img), {}, ValueError, "points must be"),
            ((pts.half(), mats, img), {}, TypeError, "points must be"),
            ((pts, mats[0], img), {}, ValueError, "lidar2imgs must be"),
            ((pts, torch.zeros((17, 4, 4)), torch.zeros((17, 4, 5, 3), dtype=torch.uint8)), {}, ValueError, "1 to 16 cameras"),
            ((pts, mats, img[:7]), {}, ValueError, r"images must be \[C, H, W, 3\] with C = 8"),
            ((pts, mats, img.float()), {}, TypeError, "images must be uint8"),
            ((pts, mats, img), {"strip": 0}, ValueError, "strip must be an integer >= 1"),
            ((pts, mats, img), {"strip": 2.0}, ValueError, "strip must be"),
            ((pts, mats, img), {"min_overlap": -1}, ValueError, "min_overlap must be an integer >= 0"),
            ((pts, mats[:2], img[:2]), {}, ValueError, r"pairs\[1\].*outside \[0, 2\)"),
            ((pts, mats, img), {"pairs": [(0, 1, 3)]}, ValueError, "side 3")):
        with pytest.raises(exc, match=match):
            M.estimate_brightness_factors(*args, **kw)
    with pytest.raises(RuntimeError, match="HIP device"):
        M.estimate_brightness_factors(pts, mats, img)


def test_stack_option_is_checked_and_off_by_default():
    import inspect
    from mtgs_amd import stack
    assert stack.SweepStack().equalise_brightness is False and stack.SweepStack.equalise_brightness is False
    on = stack.SweepStack().configure_brightness(equalise_brightness=True)
    assert isinstance(on, stack.SweepStack) and on.equalise_brightness is True and on.brightness_pairs == B.NUPLAN_PAIRS
    assert stack.SweepStack().configure_brightness(True, [[1, 0, 1]]).brightness_pairs == ((1, 0, 1),)
    assert stack.SweepStack().equalise_brightness is False                        # an instance's choice, not the class's
    with pytest.raises(ValueError, match="equalise_brightness"):
        stack.SweepStack().configure_brightness(equalise_brightness=1)
    s = inspect.signature(stack.stack_frame).parameters
    assert list(s)[-3:] == ["equalise_brightness", "brightness_pairs", "brightness_points"] and s["equalise_brightness"].default is False


def test_brightness_abi_group(hip_lib):
    """include/mtgs_brightness.h is a group of its own (test_abi.py checks it like every included header, against the reviewed record
    tests/golden/abi_signatures_brightness.txt and the library): its entry points, its constants, and the host checks of the library."""
    from mtgs_amd import _abi, _lib, brightness as M
    abi = _abi.header_abi("mtgs_brightness.h")
    assert sorted(abi.signatures) == ["mtgs_brightness_adjust", "mtgs_brightness_estimate", "mtgs_brightness_estimate_workspace_bytes"]
    assert sorted(_lib.GROUPS["mtgs_brightness.h"]) == sorted(abi.signatures) and not abi.structs
    assert abi.constants == {"MTGS_BRIGHTNESS_MAX_IMAGES": 65535, "MTGS_BRIGHTNESS_MAX_CAMERAS": 16, "MTGS_BRIGHTNESS_MAX_PAIRS": 64,
                             "MTGS_BRIGHTNESS_STRIP_SLABS": 16}
    assert (M.MAX_IMAGES, M.MAX_CAMERAS, M.MAX_PAIRS) == (65535, 16, 64)
    assert _abi.constant("MTGS_RAST_ABI_VERSION") == 29 and _abi.constant("MTGS_RAST_HOT_ABI_VERSION") == 7
    n = C.c_size_t(0)
    assert hip_lib.mtgs_brightness_estimate_workspace_bytes(8, C.byref(n)) == 0 and n.value == 2 * 8 * 16 * 8
    assert hip_lib.mtgs_brightness_estimate_workspace_bytes(0, C.byref(n)) == 1 and b"P outside" in hip_lib.mtgs_rast_last_error()
    one = C.c_void_p(8)                                           # a non-null, aligned address that is never dereferenced
    assert hip_lib.mtgs_brightness_adjust(0, 4, 4, one, 48, 12, 3, 1, one, 0, 0, 0, 0, one, None) == 1
    assert b"C outside" in hip_lib.mtgs_rast_last_error()
    assert hip_lib.mtgs_brightness_adjust(1, 0, 4, one, 48, 12, 3, 1, one, 0, 0, 0, 0, one, None) == 1
    assert b"h and w" in hip_lib.mtgs_rast_last_error()
    assert hip_lib.mtgs_brightness_adjust(1, 4, 4, None, 48, 12, 3, 1, one, 0, 0, 0, 0, one, None) == 1
    assert b"null pointer: src" in hip_lib.mtgs_rast_last_error()
    assert hip_lib.mtgs_brightness_adjust(1, 4, 4, one, 48, 12, 3, 1, one, 2, 0, 0, 0, one, None) == 1
    assert b"factor_stride" in hip_lib.mtgs_rast_last_error()
    assert hip_lib.mtgs_brightness_estimate(1, one, 0, 3, 17, one, 4, 4, one, 1, one, 100, 10, one, one, one, 256, None) == 1
    assert b"C outside [1, 16]" in hip_lib.mtgs_rast_last_error()
    assert hip_lib.mtgs_brightness_estimate(1, one, 0, 3, 2, one, 4, 4, one, 1, one, 0, 10, one, one, one, 256, None) == 1
    assert b"strip < 1" in hip_lib.mtgs_rast_last_error()
    assert hip_lib.mtgs_brightness_estimate(1, one, 0, 3, 2, one, 4, 4, one, 1, one, 100, 10, one, one, one, 8, None) != 0
    assert b"workspace" in hip_lib.mtgs_rast_last_error()
