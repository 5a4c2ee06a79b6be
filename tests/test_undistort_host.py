"""mtgs_amd.undistort without a device: the NumPy restatement (tests/undistort_refs.py) gives known answers that do not depend on any
recall of OpenCV, the new camera matrix fits the undistorted grid to the image, the half-pixel bookkeeping has its hand values, and
every refusal names its argument."""
import numpy as np
import pytest
import torch

import mtgs_amd
from mtgs_amd import undistort as U
from tests import undistort_refs as R

H, W = 13, 17
K = (16.0, 8.0, 7.0, 5.0)                 # powers of two: (j - cx') / fx' * fx + cx is exact, so the maps below are exact too
ZERO = (0.0, 0.0, 0.0, 0.0)


def image(channels=3, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (H, W, channels), dtype=np.uint8)


def shifted(dx=0.0, dy=0.0):
    """the map (j + dx, i + dy): K' = K with the principal point moved"""
    return R.undistort_map(K, ZERO, (K[0], K[1], K[2] - dx, K[3] - dy), H, W)


# ---- known answers of the restatement ------------------------------------------------------------------------------------------------
def test_zero_distortion_with_the_same_camera_returns_the_image():
    img, m = image(), shifted()
    assert np.array_equal(m[..., 0], np.broadcast_to(np.arange(W, dtype=np.float32), (H, W)))
    assert np.array_equal(m[..., 1], np.broadcast_to(np.arange(H, dtype=np.float32)[:, None], (H, W)))
    assert np.array_equal(R.remap_linear(img, m), img) and np.array_equal(R.remap_nearest(img, m), img)
    assert np.array_equal(R.remap_linear(img[..., 0], m), img[..., 0])
    assert R.valid_mask(m, H, W).all() and R.valid_mask(m, H, W).shape == (H, W, 1)
    # a source of another size: what lies beyond it is 0
    small = img[:9, :11]
    want = np.zeros_like(img)
    want[:9, :11] = small
    assert np.array_equal(R.remap_linear(small, m), want) and np.array_equal(R.remap_nearest(small, m), want)


@pytest.mark.parametrize("dx, dy", [(3, 0), (-2, 0), (0, 4), (0, -1), (5, -3)])
def test_an_integer_shift_returns_the_shifted_image_with_a_zero_border(dx, dy):
    img, m = image(), shifted(dx, dy)
    want = np.zeros_like(img)
    ys, xs = np.arange(H) + dy, np.arange(W) + dx
    oky, okx = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
    want[np.ix_(oky, okx)] = img[np.ix_(ys[oky], xs[okx])]
    assert np.array_equal(R.remap_linear(img, m), want) and np.array_equal(R.remap_nearest(img, m), want)
    valid = np.zeros((H, W, 1), bool)
    valid[np.ix_(oky, okx)] = True
    assert np.array_equal(R.valid_mask(m, H, W), valid)


def test_half_a_pixel_is_the_rounded_mean_of_the_horizontal_neighbours():
    img = image().astype(np.int64)
    right = np.concatenate([img[:, 1:], np.zeros_like(img[:, :1])], axis=1)          # beyond the last column: 0
    assert np.array_equal(R.remap_linear(image(), shifted(0.5)), (img + right + 1) >> 1)
    below = np.concatenate([img[1:], np.zeros_like(img[:1])], axis=0)
    assert np.array_equal(R.remap_linear(image(), shifted(0.0, 0.5)), (img + below + 1) >> 1)


def test_the_ties_of_the_five_fractional_bits():
    img = image().astype(np.int64)
    right = np.concatenate([img[:, 1:], np.zeros_like(img[:, :1])], axis=1)
    # 1/64 of a pixel is 0.5 in fixed point: a tie, to the even 32 j -- the image itself
    m = shifted(1.0 / 64)
    assert np.array_equal(R.fixed(m[..., 0]), np.broadcast_to(32 * np.arange(W), (H, W)))
    assert np.array_equal(R.remap_linear(image(), m), img)
    # 3/64 is 1.5: to the even 2 -- weights 30/32 and 2/32
    m = shifted(3.0 / 64)
    assert np.array_equal(R.fixed(m[..., 0]), np.broadcast_to(32 * np.arange(W) + 2, (H, W)))
    assert np.array_equal(R.remap_linear(image(), m), (30 * img + 2 * right + 16) >> 5)
    # nearest: j + 0.5 is a tie, to the even column
    cols = np.arange(W) + (np.arange(W) % 2)
    assert np.array_equal(R.nearest_index(shifted(0.5)[..., 0]), np.broadcast_to(cols, (H, W)))


def test_a_negative_fixed_point_coordinate_shifts_arithmetically():
    m = shifted(-1.0 / 32)
    sx = R.fixed(m[..., 0])
    assert sx[0, 0] == -1 and (sx[0, 0] >> R.SHIFT, sx[0, 0] & 31) == (-1, 31)
    img = image().astype(np.int64)
    left = np.concatenate([np.zeros_like(img[:, :1]), img[:, :-1]], axis=1)          # column -1: 0
    assert np.array_equal(R.remap_linear(image(), m), (left + 31 * img + 16) >> 5)


@pytest.mark.parametrize("D", [(np.nan, 0, 0, 0), (0, 0, 0, np.inf), (0, 0, 0, 0, np.nan)])
def test_a_non_finite_coefficient_gives_zeros_and_no_valid_pixel(D):
    m = R.undistort_map(K, D, K, H, W)
    assert not np.isfinite(m).any()
    out = R.undistort_frame(K, D, K, (H, W), image=image(), panoptic=image(seed=1), semantic=image(1, seed=2))
    assert not out["image"].any() and not out["panoptic"].any() and not out["semantic"].any() and not out["valid_mask"].any()
    far = np.array([np.nan, np.inf, -np.inf, 2.0 ** 30, -2.0 ** 31, 3e38], np.float32)
    assert (R.fixed(far) == R.FAR).all() and (R.nearest_index(far) == R.FAR).all()
    assert R.nearest_index(np.array([2.0 ** 30 - 64], np.float32))[0] == 2 ** 30 - 64


def test_four_coefficients_are_five_with_k3_zero():
    D4, D5 = (-0.3, 0.1, 0.002, -0.001), (-0.3, 0.1, 0.002, -0.001, 0.0)
    assert np.array_equal(R.undistort_map(K, D4, K, H, W), R.undistort_map(K, D5, K, H, W))
    assert not np.array_equal(R.undistort_map(K, D4, K, H, W), R.undistort_map(K, D5[:4] + (0.05,), K, H, W))


# ---- the new camera matrix -----------------------------------------------------------------------------------------------------------
CAMERAS = {"barrel": ((1545.0, 1545.0, 959.5, 559.5), (-0.356, 0.173, 0.0, 0.0, -0.052), (1080, 1920)),
           "pincushion": ((900.0, 880.0, 330.0, 230.0), (0.12, 0.03, 0.0, 0.0), (480, 640)),
           "tangential": ((700.0, 710.0, 300.5, 260.25), (-0.05, 0.01, 0.004, -0.003, 0.0), (500, 620))}


@pytest.mark.parametrize("name", CAMERAS)
def test_the_optimal_camera_fits_the_undistorted_grid_to_the_image(name):
    """alpha = 1: every undistorted grid point lands in [0, w-1] x [0, h-1] of the new camera and the extremes touch all four borders
    (fp64 arithmetic on values below 2e3: 1e-9 is generous); the roi lies inside the image and holds no invalid pixel's corner"""
    Kc, D, (h, w) = CAMERAS[name]
    new_K, roi = U.optimal_new_camera_matrix(Kc, D, (h, w))
    assert new_K.shape == (3, 3) and new_K.dtype == np.float64 and new_K[2, 2] == 1.0 and new_K[0, 1] == new_K[1, 0] == 0.0
    p = R.undistort_points(Kc, D, R.grid_points(h, w))
    u, v = new_K[0, 0] * p[:, 0] + new_K[0, 2], new_K[1, 1] * p[:, 1] + new_K[1, 2]
    eps = 1e-9
    assert u.min() > -eps and u.max() < w - 1 + eps and v.min() > -eps and v.max() < h - 1 + eps
    assert abs(u.min()) < eps and abs(u.max() - (w - 1)) < eps and abs(v.min()) < eps and abs(v.max() - (h - 1)) < eps
    x, y, rw, rh = roi
    assert 0 <= x and 0 <= y and rw > 0 and rh > 0 and x + rw <= w and y + rh <= h
    # alpha = 0 fits the inner rectangle instead: a longer focal length, and its whole image is the roi up to the rounding
    inner_K, inner_roi = U.optimal_new_camera_matrix(Kc, D, (h, w), alpha=0.0)
    assert inner_K[0, 0] > new_K[0, 0] and inner_K[1, 1] > new_K[1, 1]
    assert inner_roi[2] >= w - 2 and inner_roi[3] >= h - 2


def test_no_distortion_keeps_the_camera():
    new_K, roi = U.optimal_new_camera_matrix((500.0, 400.0, 100.0, 80.0), ZERO, (201, 301))
    assert np.allclose(new_K, [[500, 0, 100], [0, 400, 80], [0, 0, 1]], rtol=0, atol=1e-9)
    assert all(abs(a - b) <= 1 for a, b in zip(roi, (0, 0, 300, 200)))         # ceil and floor of values within an ulp of integers


def test_keep_focal_length_returns_the_camera_and_the_half_pixel_is_kept_in_the_books():
    Kc = np.array([[1545.0, 0, 960.0], [0, 1540.0, 560.0], [0, 0, 1]])
    D = (-0.356, 0.173, 0.001, -0.002, -0.052)
    cam = U.undistort_camera(Kc, D, (108, 192), mode="keep_focal_length", device="cpu")
    assert np.array_equal(cam.new_K, Kc) and np.array_equal(cam.K, Kc) and cam.roi == (0, 0, 192, 108)
    assert cam.source_size == cam.size == (108, 192) and cam.params.dtype == torch.float64
    # by hand: cx and cy go into the map half a pixel smaller, source and new camera alike
    assert cam.params.tolist() == [1545.0, 1540.0, 959.5, 559.5, 1545.0, 1540.0, 959.5, 559.5, -0.356, 0.173, 0.001, -0.002, -0.052]
    # optimal: the matrix of the reduced camera, its principal point half a pixel larger in the returned camera
    Ks = np.array([[154.5, 0, 96.0], [0, 154.0, 56.0], [0, 0, 1]])
    cam = U.undistort_camera(Ks, D, (108, 192), device="cpu")
    want, roi = U.optimal_new_camera_matrix((154.5, 154.0, 95.5, 55.5), D, (108, 192))
    assert cam.mode == "optimal" and cam.roi == roi
    assert cam.params[:4].tolist() == [154.5, 154.0, 95.5, 55.5]
    assert cam.params[4:8].tolist() == [want[0, 0], want[1, 1], want[0, 2], want[1, 2]]
    assert np.array_equal(cam.new_K, want + np.array([[0, 0, 0.5], [0, 0, 0.5], [0, 0, 0]]))
    # a camera of the caller's, in K's convention; four coefficients; another destination size
    cam = U.undistort_camera((10.0, 11.0, 4.0, 3.0), D[:4], (8, 9), new_K=(12.0, 13.0, 5.0, 2.0), out_size=(6, 7), device="cpu")
    assert cam.params.tolist() == [10.0, 11.0, 3.5, 2.5, 12.0, 13.0, 4.5, 1.5, -0.356, 0.173, 0.001, -0.002, 0.0]
    assert np.array_equal(cam.new_K, [[12.0, 0, 5.0], [0, 13.0, 2.0], [0, 0, 1]]) and cam.size == (6, 7) and cam.source_size == (8, 9)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument():
    D = (-0.3, 0.1, 0.0, 0.0, 0.0)
    with pytest.raises(NotImplementedError, match=r"D has 8 coefficients: the rational"):
        U.undistort_camera(K, D + (0.1, 0.0, 0.0), (H, W), device="cpu")
    with pytest.raises(NotImplementedError, match="thin-prism"):
        U.optimal_new_camera_matrix(K, (0.0,) * 12, (H, W))
    with pytest.raises(ValueError, match=r"D must have 4 or 5 coefficients.*got 3"):
        U.undistort_camera(K, D[:3], (H, W), device="cpu")
    with pytest.raises(ValueError, match=rf"size must be at most {U.MAX_SIZE} on a side"):
        U.undistort_camera(K, D, (U.MAX_SIZE + 1, W), device="cpu")
    with pytest.raises(ValueError, match=r"out_size must be at most"):
        U.undistort_camera(K, D, (H, W), out_size=(H, U.MAX_SIZE + 1), device="cpu")
    with pytest.raises(ValueError, match="mode must be"):
        U.undistort_camera(K, D, (H, W), mode="full", device="cpu")
    with pytest.raises(ValueError, match="K must be a 3 x 3 matrix"):
        U.undistort_camera((1.0, 2.0, 3.0), D, (H, W), device="cpu")
    with pytest.raises(ValueError, match="alpha must be"):
        U.optimal_new_camera_matrix(K, D, (H, W), alpha=1.5)
    cam = U.undistort_camera(K, D, (H, W), mode="keep_focal_length", device="cpu")
    rgb = torch.zeros(H, W, 3, dtype=torch.uint8)
    with pytest.raises(NotImplementedError, match=r"x has 4 channels: RGBA"):
        U.undistort_plane(torch.zeros(H, W, 4, dtype=torch.uint8), cam)
    with pytest.raises(NotImplementedError, match=r"image has 4 channels: RGBA"):
        U.undistort_frame(cam, image=torch.zeros(H, W, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match=r"cam is on cpu, x on meta"):
        U.undistort_plane(torch.zeros(H, W, 3, dtype=torch.uint8, device="meta"), cam)
    with pytest.raises(RuntimeError, match=r"cam is on cpu, panoptic on meta"):
        U.undistort_frame(cam, image=rgb, panoptic=torch.zeros(H, W, 3, dtype=torch.uint8, device="meta"))
    with pytest.raises(ValueError, match=rf"x must be {H} x {W}, the camera's source size"):
        U.undistort_plane(torch.zeros(H, W + 1, 3, dtype=torch.uint8), cam)
    with pytest.raises(TypeError, match="x must be uint8, got torch.float32"):
        U.undistort_plane(torch.zeros(H, W, 3), cam)
    with pytest.raises(ValueError, match="cubic is used only in front of UniDepth"):
        U.undistort_plane(rgb, cam, interpolation="cubic")
    with pytest.raises(ValueError, match="out_dtype of a nearest undistortion"):
        U.undistort_plane(rgb, cam, interpolation="nearest", out_dtype=torch.float32)
    with pytest.raises(ValueError, match="ego_mask must be uint8 or bool with one channel"):
        U.undistort_frame(cam, image=rgb, ego_mask=torch.zeros(H, W, dtype=torch.int32))
    with pytest.raises(TypeError, match="cam must be an UndistortCamera"):
        U.undistort_plane(rgb, K)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                    # nothing is computed on the host
        U.undistort_plane(rgb, cam)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        U.undistort_frame(cam, image=rgb)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        U.undistort_map(cam)


def test_the_launcher_checks_its_arguments_on_the_host(hip_lib):
    """before any launch: sizes, the plane count and every record are refused by name (no device is touched)"""
    import ctypes as C
    from mtgs_amd import _lib
    rec = lambda **kw: np.array([tuple({"src": 8, "dst": 8, "src_stride": (0, 0, 0), "op": 0, "elem_bytes": 1, "channels": 3,
                                        "out_float": 0, **kw}[k] for k in U._PLANE.names)], dtype=U._PLANE)
    def refused(message, h=4, w=4, oh=4, ow=4, cam=8, n=1, table=None):
        table = rec() if table is None else table
        with pytest.raises(RuntimeError, match=message):
            _lib.call("mtgs_undistort_frame", h, w, oh, ow, cam, None, n, table.ctypes.data, None)
    refused(r"h outside \[1, 16384\] \(0\)", h=0)
    refused(r"ow outside \[1, 16384\] \(16385\)", ow=U.MAX_SIZE + 1)
    refused(r"n_planes outside \[1, 8\] \(9\)", n=9)
    refused("null pointer: cam", cam=None)
    refused("cam must be 8-byte aligned", cam=12)
    refused(r"planes\[0\]\.op unknown \(3\)", table=rec(op=3))
    refused(r"null pointer: planes\[0\]\.src", table=rec(src=0))
    refused(r"planes\[0\]\.channels must be 1 or 3 for LINEAR \(2\)", table=rec(channels=2))
    refused(r"planes\[0\]\.elem_bytes must be 1 or 4 \(2\)", table=rec(op=1, elem_bytes=2))
    refused(r"planes\[0\]\.src and \.dst must be 4-byte aligned", table=rec(op=1, elem_bytes=4, src=6))
    with pytest.raises(RuntimeError, match="mtgs_undistort_map.*null pointer: map"):
        _lib.call("mtgs_undistort_map", 4, 4, 8, None, None)
    assert hip_lib.mtgs_undistort_map(0, 4, None, None, None) != 0


def test_the_package_exports_the_operators():
    for name in ("optimal_new_camera_matrix", "undistort_camera", "undistort_plane", "undistort_frame", "undistort_map", "UndistortCamera"):
        assert getattr(mtgs_amd, name) is getattr(U, name) and name in mtgs_amd.__all__
    assert (U.TILE_W, U.TILE_H, U.MAX_PLANES, U.MAX_SIZE) == (64, 4, 8, 16384)
