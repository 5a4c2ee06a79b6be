"""Lidar sweeps through the cameras (mtgs_amd/lidar.py, csrc/lidar.hip, include/mtgs_lidar.h) without a GPU: the NumPy restatement
of tests/lidar_refs.py against what the reference's own functions gave (tests/golden/lidar_ref.npz), the header as a group of its
own, the host checks of the C entry points, and what the Python layer refuses before it touches a device."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from mtgs_amd import lidar as L
from tests import lidar_refs as R

ROOT = Path(__file__).resolve().parents[1]
NAMES = ["mtgs_lidar_depth", "mtgs_lidar_depth_workspace_bytes", "mtgs_lidar_paint"]


# ---- the restatement against the reference's recorded outputs -----------------------------------------------------------------------
def test_the_restatement_paints_what_the_reference_painted():
    """Discrete outputs exactly; rgb within 1e-10 absolute: a coordinate up to about 2000 carries a few units of 2^-53 relative,
    about 1e-12 absolute; a bilinear value changes by at most 1 per pixel; summing a handful of such terms stays two orders under
    1e-10 and six orders under 1 / 255."""
    g = R.golden()
    assert (ROOT / "tests" / "golden" / "lidar_ref.npz").stat().st_size < 500_000
    pts, mats, images, masks = g["paint/points"], g["paint/lidar2imgs"], g["paint/images"], g["paint/masks"]
    assert pts.dtype == np.float32 and pts.shape == (6000, 3) and images.shape == (3, 37, 53, 3) and masks.shape == (3, 37, 53, 1)
    got = R.paint_points(pts, mats, images, masks, "bgr")
    assert np.array_equal(got.fov, g["paint/fov"]) and np.array_equal(got.count, g["paint/count"])
    assert np.array_equal(got.labels, g["paint/labels"]) and got.labels.dtype == np.int32
    diff = float(np.abs(got.rgb - g["paint/rgb"]).max())
    print(f"restatement against the reference: rgb max |diff| {diff:.3g} (recorded {float(g['paint/rgb_max_diff']):.3g})")
    assert diff <= 1e-10 and float(g["paint/rgb_max_diff"]) <= 1e-10
    # the case is what it is for: a good share of the points seen by no camera, by one and by several
    shares = [np.mean(got.count == 0), np.mean(got.count == 1), np.mean(got.count >= 2)]
    assert min(shares) > 0.1 and np.array_equal(got.fov, got.count > 0)
    assert np.all(got.rgb[~got.fov] == 0) and np.all(got.labels[~got.fov] == 0)


def test_the_restatement_scatters_what_the_reference_scattered():
    g = R.golden()
    pts, m, K, want = g["depth/points"], g["depth/lidar2cam"], g["depth/K"], g["depth/image"]
    assert m.dtype == K.dtype == np.float32 and want.dtype == np.float32 and want.shape == (37, 53, 1)
    got, winner = R.depth_image(pts, m, K, 53, 37, return_index=True)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert np.array_equal(winner >= 0, want[..., 0] != 0) and winner.dtype == np.int32
    # many collisions: the points that land outnumber the pixels they land in
    landed = sum(int((R.depth_image(pts[i:i + 1], m, K, 53, 37) != 0).any()) for i in range(0, 6000, 7))
    assert landed * 7 > 1.2 * (winner >= 0).sum()
    assert np.array_equal(R.depth_image(pts, m, K, 53, 37, scale=0.005), want * np.float32(0.005))


def test_the_restatement_takes_the_largest_index_and_the_first_camera():
    K = np.array([[32.0, 0, 16], [0, 32.0, 8], [0, 0, 1]])
    E = np.eye(4)
    pts = np.array([[0.0, 0, 4], [0.01, 0, 2], [0.02, 0.01, 8]])                     # all in pixel (16, 8)
    for order in ([0, 1, 2], [2, 1, 0], [1, 2, 0]):
        depth, winner = R.depth_image(pts[order], E, K, 32, 16, return_index=True)
        assert winner[8, 16] == 2 and (winner >= 0).sum() == 1 and depth[8, 16, 0] == np.float32(pts[order][2, 2])
    mats = np.stack([np.vstack([K @ E[:3], [0, 0, 0, 1]])] * 2)
    masks = np.stack([np.full((16, 32), 3, np.uint8), np.full((16, 32), 9, np.uint8)])
    assert list(R.paint_points(pts, mats, None, masks).labels) == [3, 3, 3]
    assert list(R.paint_points(pts, mats, None, masks[::-1]).labels) == [9, 9, 9]
    assert R.paint_points(np.zeros((0, 3)), mats, None, masks).labels.shape == (0,) and not R.depth_image(np.zeros((0, 3)), E, K, 32, 16).any()


def test_ulp_distance():
    one = np.float32(1.0)
    assert R.ulp_distance_f32(np.array([one, -one]), np.array([np.nextafter(one, np.float32(2)), -one])) == 1
    assert R.ulp_distance_f32(np.array([np.float32(0.0)]), np.array([np.float32(-0.0)])) == 0


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_the_header_is_declared_bound_and_exported():
    """include/mtgs_lidar.h is a group of its own (tests/test_abi.py checks every group against its header, its reviewed record
    tests/golden/abi_signatures_lidar.txt and the library): its entry points and its constant."""
    from mtgs_amd import _abi, _lib
    assert sorted(_lib.GROUPS["mtgs_lidar.h"]) == NAMES
    assert L.MAX_CAMERAS == _abi.header_abi("mtgs_lidar.h").constants["MTGS_LIDAR_MAX_CAMERAS"] == 64


def test_the_kernel_file_rounds_every_operation():
    from mtgs_amd import build
    assert build.PER_FILE_FLAGS["lidar.hip"] == ["-ffp-contract=off"]


def test_the_host_checks_name_the_bad_argument(hip_lib):
    size = C.c_size_t(0)
    buf = (C.c_double * 64)()                # stands for every pointer: each call below fails a check, nothing is launched
    depth = dict(N=4, points=buf, f64=1, stride=3, m=buf, K=buf, h=4, w=4, scale=1.0, depth=buf, index=None, ws=buf, ws_bytes=64, stream=None)
    paint = dict(N=4, points=buf, f64=1, stride=3, C=1, m=buf, h=4, w=4, images=buf, reverse=1, masks=buf, rgb=buf, labels=buf, fov=buf,
                 count=buf, stream=None)
    d = lambda **kw: hip_lib.mtgs_lidar_depth(*(depth | kw).values())
    p = lambda **kw: hip_lib.mtgs_lidar_paint(*(paint | kw).values())
    sizes = hip_lib.mtgs_lidar_depth_workspace_bytes
    for refused, message in ((lambda: sizes(0, 4, C.byref(size)), r"h and w must be >= 1 and h \* w < 2\^31 \(0 x 4\)"),
                             (lambda: sizes(65536, 32768, C.byref(size)), r"h \* w < 2\^31 \(65536 x 32768\)"),
                             (lambda: sizes(4, 4, None), r"null pointer: bytes"),
                             (lambda: d(N=-1), r"N outside \[0, 2\^31\) \(-1\)"), (lambda: d(N=1 << 31), r"N outside"),
                             (lambda: d(h=0), r"h and w must be"), (lambda: d(m=None), r"null pointer: lidar2cam"),
                             (lambda: d(K=None), r"null pointer: K"), (lambda: d(depth=None), r"null pointer: depth"),
                             (lambda: d(ws=None), r"null pointer: ws"), (lambda: d(points=None), r"null pointer: points"),
                             (lambda: d(stride=2), r"row_stride < 3 \(2\)"), (lambda: d(ws_bytes=63), r"workspace 63 < 64 bytes"),
                             (lambda: p(N=-1), r"N outside"), (lambda: p(w=0), r"h and w must be"),
                             (lambda: p(C=0), r"C outside \[1, 64\] \(0\)"), (lambda: p(C=65), r"C outside"),
                             (lambda: p(rgb=None), r"images and rgb go together"), (lambda: p(masks=None), r"masks and labels go together"),
                             (lambda: p(points=None), r"null pointer: points"), (lambda: p(m=None), r"null pointer: lidar2imgs"),
                             (lambda: p(fov=None), r"null pointer: fov"), (lambda: p(count=None), r"null pointer: count"),
                             (lambda: p(stride=1), r"row_stride < 3 \(1\)")):
        assert refused() != 0 and re.search(message, hip_lib.mtgs_rast_last_error().decode()), (message, hip_lib.mtgs_rast_last_error())
    assert sizes(37, 53, C.byref(size)) == 0 and size.value == 37 * 53 * 4


# ---- what the Python layer refuses ---------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_with_their_shape():
    pts, m, K = torch.zeros(5, 3), torch.eye(4), torch.eye(3)
    for kw, message in ((dict(points=torch.zeros(5, 4)), r"points must be \[N, 3\], got \(5, 4\)"),
                        (dict(points=torch.zeros(5)), r"points must be \[N, 3\], got \(5,\)"),
                        (dict(lidar2cam=torch.eye(3)), r"lidar2cam must be \[4, 4\] or \[3, 4\], got \(3, 3\)"),
                        (dict(lidar2cam=torch.zeros(2, 4, 4)), r"lidar2cam must be .* got \(2, 4, 4\)"),
                        (dict(K=torch.eye(4)), r"K must be \[3, 3\], got \(4, 4\)"), (dict(width=0), "width must be a positive integer, got 0"),
                        (dict(height=2.5), "height must be a positive integer, got 2.5"),
                        (dict(width=65536, height=32768), r"below 2\^31, got 65536 x 32768")):
        with pytest.raises(ValueError, match=message):
            L.depth_image(**(dict(points=pts, lidar2cam=m, K=K, width=8, height=8) | kw))
    for kw in (dict(points=pts.to(torch.float16)), dict(lidar2cam=m.to(torch.int32)), dict(K=K.to(torch.float16))):
        with pytest.raises(TypeError, match="float32 or float64"):
            L.depth_image(**(dict(points=pts, lidar2cam=m, K=K, width=8, height=8) | kw))
    mats, images, masks = torch.eye(4).repeat(2, 1, 1), torch.zeros(2, 8, 9, 3, dtype=torch.uint8), torch.zeros(2, 8, 9, 1, dtype=torch.uint8)
    for kw, message in ((dict(points=torch.zeros(3, 5)), r"points must be \[N, 3\], got \(3, 5\)"),
                        (dict(lidar2imgs=m), r"lidar2imgs must be \[C, 4, 4\] or \[C, 3, 4\], got \(4, 4\)"),
                        (dict(lidar2imgs=torch.zeros(0, 4, 4)), r"1 to 64 cameras, got \(0, 4, 4\)"),
                        (dict(lidar2imgs=torch.zeros(65, 3, 4)), r"1 to 64 cameras, got \(65, 3, 4\)"),
                        (dict(images=images[:1]), r"images must be \[C, H, W, 3\] with C = 2, got \(1, 8, 9, 3\)"),
                        (dict(images=images[..., :2]), r"images must be .* got \(2, 8, 9, 2\)"),
                        (dict(sem_masks=torch.zeros(2, 8, 9, 2, dtype=torch.uint8)), r"sem_masks must be .* got \(2, 8, 9, 2\)"),
                        (dict(sem_masks=torch.zeros(3, 8, 9, dtype=torch.uint8)), r"sem_masks must be .* got \(3, 8, 9\)"),
                        (dict(sem_masks=torch.zeros(2, 9, 8, dtype=torch.uint8)), r"one size, got \(2, 8, 9, 3\) and \(2, 9, 8\)"),
                        (dict(images=torch.zeros(2, 0, 9, 3, dtype=torch.uint8), sem_masks=None), "height must be a positive integer, got 0"),
                        (dict(images=None, sem_masks=None), "needs images or sem_masks"),
                        (dict(channel_order="gbr"), "channel_order must be 'bgr' or 'rgb', got 'gbr'")):
        with pytest.raises(ValueError, match=message):
            L.paint_points(**(dict(points=pts, lidar2imgs=mats, images=images, sem_masks=masks) | kw))
    for kw in (dict(images=images.float()), dict(sem_masks=masks.to(torch.int32))):
        with pytest.raises(TypeError, match="must be uint8"):
            L.paint_points(**(dict(points=pts, lidar2imgs=mats, images=images, sem_masks=masks) | kw))


def test_cpu_tensors_are_refused():
    pts, m, K = torch.zeros(5, 3), torch.eye(4), torch.eye(3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        L.depth_image(pts, m, K, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        L.paint_points(pts, m[None], torch.zeros(1, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        L.paint_points(torch.zeros(0, 3), m[None], None, torch.zeros(1, 8, 8, dtype=torch.uint8))      # N = 0 is no way around it


def test_the_public_surface():
    import mtgs_amd
    assert mtgs_amd.depth_image is L.depth_image and mtgs_amd.paint_points is L.paint_points and mtgs_amd.PaintedPoints is L.PaintedPoints
    assert {"depth_image", "paint_points", "PaintedPoints"} <= set(mtgs_amd.__all__)
    s = inspect.signature(L.depth_image).parameters
    assert list(s) == ["points", "lidar2cam", "K", "width", "height", "scale", "return_index"]
    assert (s["scale"].default, s["return_index"].default) == (1.0, False)
    s = inspect.signature(L.paint_points).parameters
    assert list(s) == ["points", "lidar2imgs", "images", "sem_masks", "channel_order"]
    assert (s["images"].default, s["sem_masks"].default, s["channel_order"].default) == (None, None, "bgr")
    assert L.PaintedPoints._fields == ("rgb", "labels", "fov", "count")
