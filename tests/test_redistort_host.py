"""mtgs_amd.undistort.redistort_image / mtgs_amd.evaldump without a device: the NumPy restatement (tests/redistort_refs.py) gives known
answers that do not depend on any recall of OpenCV, the fixed-point iteration is shown NOT to have converged at the recalled five
iterations on a nuPlan-like lens, the float conversion is the JPEG encoder's, the dump's paths are the reference's strings, and every
refusal names its argument."""
from pathlib import Path

import numpy as np
import pytest
import torch

import mtgs_amd
from mtgs_amd import evaldump as E
from mtgs_amd import undistort as U
from tests import jpeg_refs
from tests import redistort_refs as R

H, W = 13, 17
K = (16.0, 8.0, 7.0, 5.0)                 # powers of two: (j - cx) / fx * fx' + cx' is exact, so the maps below are exact too
ZERO = (0.0, 0.0, 0.0, 0.0)
NUPLAN_K, NUPLAN_D, NUPLAN_SIZE = (1545.0, 1545.0, 959.5, 559.5), (-0.356, 0.173, -0.0002, 0.0003, -0.052), (1080, 1920)


def image(channels=3, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (H, W, channels), dtype=np.uint8)


def shifted(dx=0.0, dy=0.0, iterations=5):
    """the map (j + dx, i + dy): no distortion, K' = K with the principal point moved"""
    return R.redistort_map(K, ZERO, (K[0], K[1], K[2] + dx, K[3] + dy), H, W, iterations)


# ---- known answers of the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iterations", [0, 1, 5, 64])
def test_zero_distortion_with_the_same_camera_returns_the_image(iterations):
    img, m = image(), shifted(iterations=iterations)
    assert np.array_equal(m[..., 0], np.broadcast_to(np.arange(W, dtype=np.float32), (H, W)))
    assert np.array_equal(m[..., 1], np.broadcast_to(np.arange(H, dtype=np.float32)[:, None], (H, W)))
    assert np.array_equal(R.remap(img, m), img) and np.array_equal(R.remap(img[..., 0], m), img[..., 0])
    # the image that is read may have another size: what lies beyond it is 0
    small = img[:9, :11]
    want = np.zeros_like(img)
    want[:9, :11] = small
    assert np.array_equal(R.remap(small, m), want)
    assert np.array_equal(R.redistort_image(small, K, ZERO, K, (H, W), iterations), want)


@pytest.mark.parametrize("dx, dy", [(3, 0), (-2, 0), (0, 4), (0, -1), (5, -3)])
def test_an_integer_shift_returns_the_shifted_image_with_a_zero_border(dx, dy):
    img, m = image(), shifted(dx, dy)
    want = np.zeros_like(img)
    ys, xs = np.arange(H) + dy, np.arange(W) + dx
    oky, okx = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
    want[np.ix_(oky, okx)] = img[np.ix_(ys[oky], xs[okx])]
    assert np.array_equal(R.remap(img, m), want)


def test_half_a_pixel_is_the_rounded_mean_and_the_ties_go_to_even():
    img = image().astype(np.int64)
    right = np.concatenate([img[:, 1:], np.zeros_like(img[:, :1])], axis=1)          # beyond the last column: 0
    below = np.concatenate([img[1:], np.zeros_like(img[:1])], axis=0)
    assert np.array_equal(R.remap(image(), shifted(0.5)), (img + right + 1) >> 1)
    assert np.array_equal(R.remap(image(), shifted(0.0, 0.5)), (img + below + 1) >> 1)
    # 1/64 of a pixel is 0.5 in fixed point: a tie, to the even 32 j -- the image itself; 3/64 is 1.5: to the even 2 -- 30/32 and 2/32
    assert np.array_equal(R.remap(image(), shifted(1.0 / 64)), img)
    assert np.array_equal(R.remap(image(), shifted(3.0 / 64)), (30 * img + 2 * right + 16) >> 5)


def test_no_iteration_is_the_plain_change_of_camera():
    D, new_K = (-0.3, 0.1, 0.01, -0.02, 0.05), (12.0, 9.0, 6.25, 4.5)
    m = R.redistort_map(K, D, new_K, H, W, iterations=0)
    j, i = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
    want = np.stack(np.broadcast_arrays((12.0 * ((j - 7.0) / 16.0) + 6.25).astype(np.float32), (9.0 * ((i - 5.0) / 8.0) + 4.5).astype(np.float32)), -1)
    assert np.array_equal(m, want)
    assert np.array_equal(m, R.redistort_map(K, ZERO, new_K, H, W, iterations=0))               # the lens plays no part
    assert not np.array_equal(m, R.redistort_map(K, D, new_K, H, W, iterations=1))
    with pytest.raises(ValueError, match=r"iterations outside \[0, 64\]"):
        R.redistort_map(K, D, new_K, H, W, iterations=65)


FOLDED_D = (-4.0, 0.0, 0.0, 0.0)           # 1 + k1 r2 < 0 where r2 > 1/4


def test_a_folded_over_lens_returns_to_its_start_at_the_corners():
    """r2 of pixel (i, j) is ((j - 7) / 16)^2 + ((i - 5) / 8)^2: above 1/4 at the four corners, so icdist < 0 in the FIRST iteration
    there and the entry is the plain change of camera; at the centre the iteration runs"""
    plain = R.redistort_map(K, FOLDED_D, K, H, W, iterations=0)
    m = R.redistort_map(K, FOLDED_D, K, H, W, iterations=5)
    j, i = np.meshgrid(np.arange(W), np.arange(H))
    r2 = ((j - 7.0) / 16.0) ** 2 + ((i - 5.0) / 8.0) ** 2
    first = r2 > 0.25
    assert first[0, 0] and first[0, -1] and first[-1, 0] and first[-1, -1] and not first[5, 7] and 0.2 < first.mean() < 0.8
    assert np.array_equal(m[first], plain[first])
    # one iteration: x = x0 / (1 - 4 r2) where that is positive, by hand
    one = R.redistort_map(K, FOLDED_D, K, H, W, iterations=1)
    x0 = (j - 7.0) / 16.0
    with np.errstate(all="ignore"):                                # r2 = 1/4 exactly at (5, 15), (1, 7), (9, 7): icdist is +inf, not negative
        want = (16.0 * (x0 * (1.0 / (1.0 + (-4.0 * r2)))) + 7.0).astype(np.float32)
    assert np.array_equal(one[..., 0][~first], want[~first], equal_nan=True) and np.array_equal(one[..., 0][first], plain[..., 0][first])
    assert (one[..., 0][~first & (j != 7)] != plain[..., 0][~first & (j != 7)]).all()
    # a point that folds over in a LATER iteration goes back to its start too, not to where it was
    x, y = R.inverse_points(K, FOLDED_D, np.array([13.0]), np.array([5.0]), iterations=1)       # x0 = 0.375, r2 = 0.140625
    assert x[0] > 0.5 and 1.0 - 4.0 * x[0] * x[0] < 0                                           # the next icdist is negative
    x2, _ = R.inverse_points(K, FOLDED_D, np.array([13.0]), np.array([5.0]), iterations=2)
    x9, _ = R.inverse_points(K, FOLDED_D, np.array([13.0]), np.array([5.0]), iterations=9)
    assert x2[0] == 0.375 == x9[0]


@pytest.mark.parametrize("D", [(np.nan, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 0.0, np.nan), (0.0, 0.0, 1e300, 1e300, 0.0)])
@pytest.mark.parametrize("iterations", [1, 5])
def test_nan_and_huge_coefficients_give_an_all_zero_frame(D, iterations):
    """NaN: icdist is NaN, NaN < 0 is false, the entry stays NaN.  1e300 in the tangential terms (3x^2 + 2xy + y^2 and its mirror are
    positive definite and no pixel has x0 = y0 = 0 here): dx, dy ~ 1e300 -- one iteration maps beyond float32, a second one makes
    r2 infinite and 0 * inf NaN.  Either way every coordinate is OUTSIDE.  (1e300 in the RADIAL terms does the opposite: icdist
    vanishes and every pixel reads the principal point -- below.)"""
    raw_K = (K[0], K[1], K[2] + 0.25, K[3] + 0.25)
    m = R.redistort_map(raw_K, D, K, H, W, iterations)
    assert (undistort_fixed(m) == -(1 << 30)).all()
    assert not R.remap(image(), m).any() and not R.remap(image().astype(np.float32) / 255, m).any()


def undistort_fixed(m):
    from tests import undistort_refs
    return np.stack([undistort_refs.fixed(m[..., 0]), undistort_refs.fixed(m[..., 1])], -1)


def test_a_huge_radial_term_reads_the_principal_point():
    """icdist = 1 / (1 + 1e300 r2) is about 1e-298 and x = x0 icdist vanishes beside cx'; at pixel (5, 7) r2 = 0, icdist = 1 and x = 0"""
    m = R.redistort_map(K, (1e300, 0.0, 0.0, 0.0), (K[0], K[1], 3.0, 2.0), H, W, iterations=1)
    assert (m[..., 0] == 3.0).all() and (m[..., 1] == 2.0).all()
    assert (R.remap(image(), m) == image()[2, 3]).all()


# ---- the recalled five iterations have not converged -----------------------------------------------------------------------------------
def test_five_iterations_have_not_converged_on_a_nuplan_like_lens_and_twenty_have():
    """the forward model of include/mtgs_undistort.h applied to the inverse returns the pixel it started from: every 8th pixel and
    the borders of 1920 x 1080.  Measured: 0.82 px at 5 iterations (mean 0.027), 5.3e-3 at 10, 2.2e-7 at 20, 4.7e-13 at 40"""
    h, w = NUPLAN_SIZE
    ii, jj = np.unique(np.r_[np.arange(0, h, 8), h - 1]), np.unique(np.r_[np.arange(0, w, 8), w - 1])
    px, py = np.meshgrid(jj.astype(np.float64), ii.astype(np.float64))
    worst, mean = {}, {}
    for n in (5, 10, 20):
        x, y = R.inverse_points(NUPLAN_K, NUPLAN_D, px, py, n)
        u, v = R.forward_pixels(NUPLAN_K, NUPLAN_D, x, y)
        err = np.hypot(u - px, v - py)
        worst[n], mean[n] = float(err.max()), float(err.mean())
        print(f"iterations {n}: worst {worst[n]:.3e} px, mean {mean[n]:.3e} px")
    assert worst[5] > worst[10] > worst[20]
    assert worst[5] > 0.25 and worst[20] < 1e-5
    assert round(worst[5], 2) == 0.82 and mean[5] < 0.05          # the figures the documents state


# ---- the float conversion ------------------------------------------------------------------------------------------------------------
def test_a_float_source_is_converted_as_the_jpeg_encoder_converts():
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    values = np.concatenate([k, np.nextafter(k, np.float32(-1)), np.float32([0.0, 1.0, -0.5, -0.0, 2.0, 1e30, np.nan, np.inf, -np.inf, 0.5])])
    src = np.zeros((H, W, 3), np.float32)
    src.reshape(-1)[:] = np.resize(values, src.size)
    assert src.size >= values.size
    for conversion in ("truncate", "round"):
        want = jpeg_refs.to_u8(src, conversion)
        assert np.array_equal(R.remap(src, shifted(), conversion), want)
        assert np.array_equal(R.to_u8(src, conversion), want)
    t, r = R.to_u8(np.float32([0.0, 1.0, -0.5, 2.0, np.nan, 0.5, np.inf]), "truncate"), R.to_u8(np.float32([0.5, 1.0]), "round")
    assert t.tolist() == [0, 255, 0, 255, 0, 127, 255] and r.tolist() == [128, 255]
    # BEFORE the interpolation: half way between 1.6 / 255 and 2.8 / 255 lies (1 + 2 + 1) >> 1, with "round" (2 + 3 + 1) >> 1 -- the
    # mean 2.2 / 255 converted afterwards would be 2 either way
    pair = np.zeros((1, 2, 1), np.float32)
    pair[0, :, 0] = np.float32(1.6) / 255, np.float32(2.8) / 255
    m = np.zeros((1, 1, 2), np.float32)
    m[0, 0, 0] = 0.5
    assert R.remap(pair, m)[0, 0, 0] == 2 and R.remap(pair, m, "round")[0, 0, 0] == 3
    assert np.array_equal(R.to_u8(image()), image())


# ---- where the dump writes -----------------------------------------------------------------------------------------------------------
def test_the_paths_are_the_reference_strings():
    raw = Path("/data/nuplan/sensor_blobs/2021.05.12.22.00.38_veh-35_01008_01518/CAM_F0/0a1b2c3d4e5f.jpg")
    assert E.eval_dump_paths("sequential", travel_id=3, cam_name="CAM_F0", cam_idx=17) == {"rendered": "traversal_3/CAM_F0/17_rendered.jpg"}
    assert E.eval_dump_paths("sequential_with_gt", 0, "CAM_B0", 5, raw) == {
        "rendered": "traversal_0/CAM_B0/5_rendered.jpg", "gt_processed": "traversal_0/CAM_B0/5_gt_processed.jpg",
        "gt": "traversal_0/CAM_B0/5_gt.jpg", "gt_target": str(raw)}
    assert E.eval_dump_paths("sequential_with_gt", 0, "c", 1, "some/raw.jpg")["gt_target"] == str(Path("some/raw.jpg").absolute())
    assert E.eval_dump_paths("nuplan", raw_path=raw) == {"rendered": "2021.05.12.22.00.38_veh-35_01008_01518/CAM_F0/0a1b2c3d4e5f.jpg"}
    assert E.eval_dump_paths("nuplan", raw_path=str(raw)) == E.eval_dump_paths("nuplan", 1, "x", 2, raw)
    with pytest.raises(ValueError, match="mode must be one of"):
        E.eval_dump_paths("video")
    with pytest.raises(ValueError, match="mode 'sequential' needs cam_name"):
        E.eval_dump_paths("sequential", travel_id=1, cam_idx=2)
    with pytest.raises(ValueError, match="mode 'sequential_with_gt' needs raw_path"):
        E.eval_dump_paths("sequential_with_gt", 1, "c", 2)
    with pytest.raises(ValueError, match="mode 'nuplan' needs raw_path"):
        E.eval_dump_paths("nuplan", 1, "c", 2)
    with pytest.raises(ValueError, match="raw_path must end in"):
        E.eval_dump_paths("nuplan", raw_path="token.jpg")


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument():
    cam = U.undistort_camera(K, (-0.3, 0.1, 0.0, 0.0), (H, W), new_K=K, out_size=(H - 2, W + 3), device="cpu")
    assert cam.size == (H - 2, W + 3) and cam.source_size == (H, W)
    rgb = torch.zeros(H - 2, W + 3, 3)
    with pytest.raises(NotImplementedError, match=r"image has 4 channels: RGBA"):
        U.redistort_image(torch.zeros(H - 2, W + 3, 4), cam)
    with pytest.raises(NotImplementedError, match=r"image has 2 channels"):
        U.redistort_image(torch.zeros(H - 2, W + 3, 2), cam)
    with pytest.raises(TypeError, match="image must be uint8 or float32, got torch.float64"):
        U.redistort_image(rgb.double(), cam)
    with pytest.raises(ValueError, match=r"image must be \[H, W, C\]"):
        U.redistort_image(rgb[..., 0], cam)
    with pytest.raises(ValueError, match=rf"image must be {H - 2} x {W + 3}, the camera's size, got \({H}, {W}, 3\)"):
        U.redistort_image(torch.zeros(H, W, 3), cam)                                 # the RAW size is what is written, not what is read
    for bad in (-1, 65, 5.0, True):
        with pytest.raises(ValueError, match=r"iterations must be an integer in \[0, 64\]"):
            U.redistort_image(rgb, cam, iterations=bad)
        with pytest.raises(ValueError, match=r"iterations must be an integer in \[0, 64\]"):
            U.redistort_map(cam, iterations=bad)
    with pytest.raises(ValueError, match="conversion must be 'truncate' or 'round'"):
        U.redistort_image(rgb, cam, conversion="floor")
    with pytest.raises(ValueError, match=rf"map must be a contiguous float32 \({H}, {W}, 2\)"):
        U.redistort_image(rgb, cam, map=torch.zeros(H - 2, W + 3, 2))
    with pytest.raises(ValueError, match=rf"out must be a contiguous uint8 \({H}, {W}, 3\)"):
        U.redistort_image(rgb, cam, out=torch.zeros(H - 2, W + 3, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="cam is on cpu, image on meta"):
        U.redistort_image(rgb.to("meta"), cam)
    with pytest.raises(TypeError, match="cam must be an UndistortCamera"):
        U.redistort_image(rgb, K)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                    # nothing is computed on the host
        U.redistort_image(rgb, cam)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        U.redistort_map(cam)
    # the dump
    with pytest.raises(ValueError, match="mode must be one of"):
        E.eval_dump(rgb, "video")
    with pytest.raises(ValueError, match="mode 'nuplan' needs cam"):
        E.eval_dump(rgb, "nuplan")
    with pytest.raises(ValueError, match="the camera's size"):
        E.eval_dump(torch.zeros(H, W, 3), "nuplan", cam=cam)
    with pytest.raises(ValueError, match="mode 'nuplan' writes the rendered frame only"):
        E.eval_dump(rgb, "nuplan", gt_image=rgb, cam=cam)
    with pytest.raises(ValueError, match="cam and map belong to mode 'nuplan'"):
        E.eval_dump(rgb, "sequential", cam=cam)
    with pytest.raises(ValueError, match="mode 'sequential_with_gt' needs gt_image"):
        E.eval_dump(rgb, "sequential_with_gt")
    with pytest.raises(ValueError, match="mode 'sequential' writes the rendered frame only"):
        E.eval_dump(rgb, "sequential", gt_image=rgb)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.eval_dump(rgb, "nuplan", cam=cam)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.eval_dump(rgb, "sequential")


def test_the_launchers_check_their_arguments_on_the_host(hip_lib):
    """before any launch: sizes, the iteration count, pointers, alignment, the source's format (no device is touched)"""
    from mtgs_amd import _lib
    def refused(message, h=4, w=4, oh=4, ow=4, cam=8, iterations=5, map=None, src=8, src_float=0, conversion=U._CONVERSIONS["truncate"],
                channels=3, dst=8):
        with pytest.raises(RuntimeError, match="mtgs_redistort_frame.*" + message):
            _lib.call("mtgs_redistort_frame", h, w, oh, ow, cam, iterations, map, src, src_float, conversion, 12, 3, 1, channels, dst, None)
    refused(r"h outside \[1, 16384\] \(0\)", h=0)
    refused(r"w outside \[1, 16384\] \(-3\)", w=-3)
    refused(r"oh outside \[1, 16384\] \(16385\)", oh=U.MAX_SIZE + 1)
    refused(r"ow outside \[1, 16384\] \(0\)", ow=0)
    refused(r"iterations outside \[0, 64\] \(65\)", iterations=65)
    refused(r"iterations outside \[0, 64\] \(-1\)", iterations=-1)
    refused("null pointer: cam", cam=None)
    refused("null pointer: src", src=None)
    refused("null pointer: dst", dst=None)
    refused("cam must be 8-byte aligned", cam=12)
    refused("map must be 4-byte aligned", map=6)
    refused(r"src_float must be 0 or 1 \(2\)", src_float=2)
    refused("src must be 4-byte aligned when src_float is set", src=6, src_float=1)
    refused(r"conversion must be MTGS_PRESENT_U8_TRUNCATE or MTGS_PRESENT_U8_ROUND \(7\)", conversion=7)
    refused(r"channels must be 1 or 3 \(2\)", channels=2)
    refused(r"channels must be 1 or 3 \(4\)", channels=4)
    for args, message in (((0, 4, 8, 5, 8, None), r"oh outside \[1, 16384\] \(0\)"), ((4, 4, 8, 65, 8, None), r"iterations outside \[0, 64\] \(65\)"),
                          ((4, 4, None, 5, 8, None), "null pointer: cam"), ((4, 4, 8, 5, None, None), "null pointer: map"),
                          ((4, 4, 8, 5, 12, None), "map must be 8-byte aligned")):
        with pytest.raises(RuntimeError, match="mtgs_redistort_map.*" + message):
            _lib.call("mtgs_redistort_map", *args)
    assert U.MAX_ITERATIONS == 64 and sorted(_lib.GROUPS["mtgs_redistort.h"]) == ["mtgs_redistort_frame", "mtgs_redistort_map"]


def test_the_package_exports_the_operators():
    for name in ("redistort_image", "redistort_map"):
        assert getattr(mtgs_amd, name) is getattr(U, name) and name in mtgs_amd.__all__ and name in U.__all__
    for name in ("eval_dump", "eval_dump_paths"):
        assert getattr(mtgs_amd, name) is getattr(E, name) and name in mtgs_amd.__all__
    assert E.MODES == ("sequential", "sequential_with_gt", "nuplan")
