"""mtgs_amd.lidar on the device against the NumPy restatement of tests/lidar_refs.py (and, for the recorded cases, against what
the reference's own functions gave): every discrete output -- fov, count, labels, the winner index image, the zero set of the
depth -- equal; depth values equal and in any case within 1 float32 ulp (two fp64 evaluations a few ulps apart round to
neighbouring floats at worst); rgb within 1e-10 (tests/test_lidar_host.py says where that bound comes from).  Every comparison
prints its measured maxima.  Images are 37 x 53 and 64 x 32, N is at most a few thousand."""
import numpy as np
import pytest
import torch

import mtgs_amd
from mtgs_amd import lidar as L
from tests import lidar_refs as R

pytestmark = pytest.mark.gpu
H, W = 37, 53
RGB_BOUND = 1e-10


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def host(t):
    return None if t is None else t.cpu().numpy()


def check_depth(points, m, K, width, height, scale=1.0, what="depth", **kw):
    """depth_image on the device against the restatement; the inputs are NumPy arrays (kw: how the device tensors are made)"""
    make = kw.get("make", dev)
    got, index = L.depth_image(make(points), dev(m), dev(K), width, height, scale=scale, return_index=True)
    torch.cuda.synchronize()
    want, winner = R.depth_image(points, m, K, width, height, scale=scale, return_index=True)
    got, index = host(got), host(index)
    assert got.dtype == np.float32 and got.shape == (height, width, 1) and index.dtype == np.int32 and index.shape == (height, width)
    ulps = R.ulp_distance_f32(np.nan_to_num(got, posinf=0, neginf=0), np.nan_to_num(want, posinf=0, neginf=0))
    print(f"{what}: N={len(points)} {height}x{width} hits={int((winner >= 0).sum())} max depth distance {ulps} ulp, "
          f"bitwise equal: {got.tobytes() == want.tobytes()}")
    assert np.array_equal(index, winner) and np.array_equal(got == 0, want == 0)
    assert np.array_equal(np.isfinite(got), np.isfinite(want)) and ulps <= 1
    assert np.array_equal(got, want, equal_nan=True)
    return got, index


def check_paint(points, mats, images=None, masks=None, order="bgr", what="paint", **kw):
    make = kw.get("make", dev)
    got = L.paint_points(make(points), dev(mats), None if images is None else dev(images), None if masks is None else dev(masks), order)
    torch.cuda.synchronize()
    want = R.paint_points(points, mats, images, masks, order)
    n = len(points)
    fov, count = host(got.fov), host(got.count)
    assert fov.dtype == np.bool_ and fov.shape == (n,) and count.dtype == np.int32 and count.shape == (n,)
    assert np.array_equal(fov, want.fov) and np.array_equal(count, want.count)
    line = f"{what}: N={n} C={len(mats)} seen by 0/1/2+ cameras {int((count == 0).sum())}/{int((count == 1).sum())}/{int((count > 1).sum())}"
    if masks is None:
        assert got.labels is None
    else:
        labels = host(got.labels)
        assert labels.dtype == np.int32 and np.array_equal(labels, want.labels)
    if images is None:
        assert got.rgb is None
    else:
        rgb = host(got.rgb)
        assert rgb.dtype == np.float64 and rgb.shape == (n, 3)
        diff = float(np.abs(rgb - want.rgb).max()) if n else 0.0
        line += f" max |rgb - restatement| {diff:.3g}, bitwise equal: {rgb.tobytes() == want.rgb.tobytes()}"
        assert diff <= RGB_BOUND and np.all(rgb[~fov] == 0)
    print(line)
    return got


def ring(n_cameras, width=W, height=H, f=30.0, seed=5):
    """cameras 50 degrees apart with 82 degrees of view each: neighbours overlap, and up to seven leave a part of the ring unseen"""
    rng = np.random.default_rng(seed)
    return np.stack([R.camera(50.0 * c + 10.0, f, rng.uniform(-0.5, 0.5, 3), width, height)[0] for c in range(n_cameras)])


def textures(n_cameras, width=W, height=H, seed=6):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (n_cameras, height, width, 3), dtype=np.uint8), rng.integers(0, 20, (n_cameras, height, width, 1), dtype=np.uint8))


# ---- the recorded cases: the reference's own outputs --------------------------------------------------------------------------------
def test_golden_paint():
    g = R.golden()
    got = check_paint(g["paint/points"], g["paint/lidar2imgs"], g["paint/images"], g["paint/masks"], what="golden paint")
    assert np.array_equal(host(got.fov), g["paint/fov"]) and np.array_equal(host(got.count), g["paint/count"])
    assert np.array_equal(host(got.labels), g["paint/labels"])
    diff = float(np.abs(host(got.rgb) - g["paint/rgb"]).max())
    print(f"golden paint: max |rgb - reference| {diff:.3g}")
    assert diff <= RGB_BOUND


def test_golden_depth():
    g = R.golden()
    got, index = check_depth(g["depth/points"], g["depth/lidar2cam"], g["depth/K"], W, H, what="golden depth")
    ulps = R.ulp_distance_f32(got, g["depth/image"])
    print(f"golden depth: max distance to the reference {ulps} ulp")
    assert np.array_equal(got == 0, g["depth/image"] == 0) and ulps <= 1 and np.array_equal(got, g["depth/image"])


# ---- point counts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 5000])
def test_point_counts(n):
    pts = R.sweep(np.random.default_rng(100 + n), n)
    for c in (1, 3, 8):
        images, masks = textures(c)
        got = check_paint(pts, ring(c), images, masks, what=f"counts N={n} C={c}")
        assert got.rgb.shape == (n, 3) and got.labels.shape == (n,)
    _, E, K = R.camera(20.0, 30.0, (0.1, -0.2, 0.3), W, H)
    got, index = check_depth(pts, E, K, W, H, what=f"counts N={n}")
    if n == 0:
        assert not got.any() and (index == -1).all()


# ---- collisions --------------------------------------------------------------------------------------------------------------------
_K64 = np.array([[32.0, 0, 0], [0, 16.0, 0], [0, 0, 1.0]])           # 64 x 32: u = 32 x0 / x2, v = 16 x1 / x2, powers of two throughout
_E = np.eye(4)[:3]


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_the_largest_index_wins_in_one_pixel(order):
    """300 points in pixel (20, 9) at indices spread over 2000 (eight workgroups, 32 waves), the rest behind the camera; their
    depths ascend, descend or are shuffled with the index, so "the nearest wins" and "the first wins" both fail"""
    rng = np.random.default_rng(3)
    n, k = 2000, 300
    pts = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(-9, -1, n)], -1)
    where = np.sort(rng.choice(n, k, replace=False))
    z = 2.0 + np.arange(k) / 64.0
    z = {"ascending": z, "descending": z[::-1], "shuffled": rng.permutation(z)}[order]
    pts[where] = np.stack([(20.25 / 32) * z, (9.5 / 16) * z, z], -1)
    got, index = check_depth(pts, _E, _K64, 64, 32, what=f"one pixel, depths {order}")
    assert index[9, 20] == where[-1] and (index >= 0).sum() == 1 and got[9, 20, 0] == np.float32(z[-1])
    assert where[-1] - where[0] > 1500


@pytest.mark.parametrize("corner", ["first", "last"])
def test_every_point_in_one_corner(corner):
    rng = np.random.default_rng(4)
    n = 1000
    z = rng.uniform(1, 50, n)
    u, v = (rng.uniform(0, 1, n), rng.uniform(0, 1, n)) if corner == "first" else (rng.uniform(63, 64, n), rng.uniform(31, 32, n))
    pts = np.stack([u / 32 * z, v / 16 * z, z], -1)
    got, index = check_depth(pts, _E, _K64, 64, 32, what=f"every point in the {corner} pixel")
    y, x = (0, 0) if corner == "first" else (31, 63)
    assert (index >= 0).sum() == 1 and index[y, x] == n - 1


# ---- decision boundaries, from dyadic values: every product and sum below is exact ----------------------------------------------------
def test_depth_decision_boundaries():
    below = lambda v: np.nextafter(v, 0.0)
    tiny = 5e-324                                            # the smallest positive double
    cases = [                 # (x0, x1, x2), expected pixel (x, y) or None; row y = case number keeps them apart
        ((0.0, 1 / 16, 1.0), (0, 1)),                        # u exactly 0
        ((2.0, 2 / 16, 1.0), None),                          # u exactly W
        ((below(2.0), 3 / 16, 1.0), (63, 3)),                # u just below W
        ((-1 / 64, 4 / 16, 1.0), None),                      # u = -0.5: out, although truncation would give 0
        ((-1 / 1024, 5 / 16, 1.0), None),                    # u = -1 / 32
        ((1.0, 6 / 16, 0.0), None),                          # cam_2 exactly 0
        ((0.0, 0.0, tiny), (0, 0)),                          # the smallest positive cam_2: u = v = 0, the depth rounds to 0.0f
        ((1.0, 2.0, 1.0), None),                             # v exactly H
        ((1.0, below(2.0), 1.0), (32, 31)),                  # v just below H
        ((1.0, -1 / 32, 1.0), None),                         # v = -0.5
        ((0.5, 7 / 16, -1.0), None),                         # behind the camera
    ]
    pts = np.array([c[0] for c in cases])
    got, index = check_depth(pts, _E, _K64, 64, 32, what="depth boundaries")
    for i, (_, pixel) in enumerate(cases):
        assert ((index == i).sum() == 1 and index[pixel[1], pixel[0]] == i) if pixel else not (index == i).any(), (i, cases[i])
    assert index[0, 0] == 6 and got[0, 0, 0] == 0.0          # a hit whose float32 depth is zero: the index image still names it


def test_depth_negative_zero_is_inside():
    """u = -0.0 >= 0 holds and (int)-0.0 = 0: a first matrix row of negative zeros gives cam_0 = -0.0, K's row keeps the sign"""
    E = np.array([[-0.0, -0.0, -0.0, -0.0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]])
    K = np.array([[32.0, -0.0, -0.0], [0, 16.0, 0], [0, 0, 1.0]])
    pts = np.array([[1.0, 0.25, 1.0], [3.0, 0.5, 2.0]])
    with np.errstate(all="ignore"):
        cam0 = R.row34(E[0], pts)
    assert np.all(cam0 == 0) and np.all(np.signbit(cam0)) and np.all(np.signbit(R.row33(K[0], [cam0, pts[:, 1], pts[:, 2]])))
    got, index = check_depth(pts, E, K, 64, 32, what="u = -0.0")
    assert index[4, 0] == 1 and (index >= 0).sum() == 1 and got[4, 0, 0] == 2.0          # both points: pixel (0, 4)


def _nx_for(target, size):
    """a double nx in [0, 1) whose ix = (((nx 2 - 1) + 1) / 2) (size - 1) is EXACTLY `target`, found among the neighbours of
    target / (size - 1); None if there is none (size - 1 is odd for both sides of the 64 x 32 image, so nx is not dyadic)"""
    for towards in (1.0, 0.0):
        nx = np.float64(target) / (size - 1)
        for _ in range(64):
            if (((nx * 2 - 1) + 1) / 2) * (size - 1) == target:
                return float(nx)
            nx = np.nextafter(nx, towards)
    return None


def test_paint_decision_boundaries():
    """64 x 32, one camera whose matrix is [64 0 0 0; 0 32 0 0; 0 0 1 0]: with x2 = 1, nx = x0 and ny = x1 exactly"""
    mats = np.array([[[64.0, 0, 0, 0], [0, 32.0, 0, 0], [0, 0, 1.0, 0], [0, 0, 0, 1.0]]])
    images, masks = textures(1, 64, 32, seed=9)
    tenth = 0.1                                              # the double nearest to 0.1: p_2 > 0.1 is false for it
    ties_x = {k: _nx_for(k + 0.5, 64) for k in (2, 3, 10, 11, 30, 31, 44, 45)}
    ties_y = {k: _nx_for(k + 0.5, 32) for k in (2, 3, 14, 15, 20, 21)}
    whole_x = {k: _nx_for(float(k), 64) for k in (1, 7, 32, 62)}
    assert ties_x[31] == 0.5 and ties_y[15] == 0.5           # the two dyadic ties: 31.5 -> 32, 15.5 -> 16
    found = lambda d: {k: v for k, v in d.items() if v is not None}
    ties_x, ties_y, whole_x = found(ties_x), found(ties_y), found(whole_x)
    assert any(k % 2 == 0 for k in ties_x) and any(k % 2 for k in ties_x) and any(k % 2 == 0 for k in ties_y) and whole_x
    pts = [(0.0, 0.0, tenth * 1.0), (0.0, 0.0, np.nextafter(tenth, 1.0)),     # p_2 exactly 0.1 (out), the next double (in)
           (0.0, 0.25, 1.0), (0.25, 0.0, 1.0), (0.0, 0.0, 1.0),               # nx exactly 0, ny exactly 0, both
           (1.0, 0.5, 1.0), (np.nextafter(1.0, 0.0), 0.5, 1.0),               # nx exactly 1 (out), just below (ix rounds to W - 1)
           (0.5, 1.0, 1.0), (0.5, np.nextafter(1.0, 0.0), 1.0),
           (-1 / 1024, 0.5, 1.0), (0.5, -1 / 1024, 1.0), (-0.0, -0.0, 1.0)]
    n_fixed = len(pts)
    pts += [(v, 0.25, 1.0) for v in ties_x.values()] + [(0.25, v, 1.0) for v in ties_y.values()] + [(v, 0.75, 1.0) for v in whole_x.values()]
    pts = np.array(pts)
    got = check_paint(pts, mats, images, masks, what="paint boundaries")
    fov, labels, rgb = host(got.fov), host(got.labels), host(got.rgb)
    assert list(fov[:n_fixed]) == [False, True, True, True, True, False, True, False, True, False, False, True]
    assert fov[n_fixed:].all()
    texel = lambda y, x: images[0, y, x, ::-1].astype(np.float64) / 255.0
    assert labels[4] == masks[0, 0, 0, 0] and np.array_equal(rgb[4], texel(0, 0)) and np.array_equal(rgb[11], texel(0, 0))
    assert labels[6] == masks[0, 16, 63, 0] and labels[8] == masks[0, 31, 32, 0]            # iy = 15.5 -> 16, ix = 31.5 -> 32
    at = n_fixed
    even = lambda k: k if k % 2 == 0 else k + 1                                      # k + 0.5 goes to the even neighbour
    for k in ties_x:
        assert labels[at] == masks[0, 8, even(k), 0], ("ix", k)                      # iy = 0.25 * 31 = 7.75 -> 8
        at += 1
    for k in ties_y:
        assert labels[at] == masks[0, even(k), 16, 0], ("iy", k)                     # ix = 0.25 * 63 = 15.75 -> 16
        at += 1
    for k in whole_x:                                                                # ix on an integer: fx = 0, two texels of one column
        fy = 0.75 * 31 - 23
        assert labels[at] == masks[0, 23, k, 0] and np.allclose(rgb[at], texel(23, k) * (1 - fy) + texel(24, k) * fy, rtol=0, atol=1e-15)
        at += 1


# ---- non-finite points ---------------------------------------------------------------------------------------------------------------
def test_non_finite_points_write_nothing_and_are_seen_by_nothing():
    rng = np.random.default_rng(11)
    pts = R.sweep(rng, 1500).astype(np.float64)
    bad = np.sort(rng.choice(1500, 90, replace=False))
    clean = pts.copy()
    for j, i in enumerate(bad):
        pts[i, rng.integers(0, 3) if j % 2 else slice(None)] = (np.nan, np.inf, -np.inf)[j % 3]
    clean[bad] = (0.0, 0.0, -1e6)                            # behind or beside every camera and far away: seen by nothing either
    mats = ring(3)
    images, masks = textures(3)
    got = check_paint(pts, mats, images, masks, what="non-finite paint")
    ref = L.paint_points(dev(clean), dev(mats), dev(images), dev(masks))
    assert not host(got.fov)[bad].any() and not host(got.count)[bad].any() and not host(got.labels)[bad].any() and not host(got.rgb)[bad].any()
    assert not host(ref.fov)[bad].any()
    for a, b in zip(got, ref):
        assert torch.equal(a, b)                             # the other points' results are unchanged
    _, E, K = R.camera(20.0, 30.0, (0.1, -0.2, 0.3), W, H)
    depth, index = check_depth(pts, E, K, W, H, what="non-finite depth")
    keep = np.setdiff1d(np.arange(1500), bad)
    d2, i2 = L.depth_image(dev(pts[keep]), dev(E), dev(K), W, H, return_index=True)
    assert not np.isin(index, bad).any() and np.isfinite(depth).all()
    assert np.array_equal(depth, host(d2)) and np.array_equal(index >= 0, host(i2) >= 0)
    assert np.array_equal(index[index >= 0], keep[host(i2)[host(i2) >= 0]])


# ---- strides and dtypes --------------------------------------------------------------------------------------------------------------
def test_strides_and_dtypes():
    rng = np.random.default_rng(12)
    p32 = R.sweep(rng, 777)
    mats, (images, masks) = ring(3), textures(3)
    _, E, K = R.camera(20.0, 30.0, (0.1, -0.2, 0.3), W, H)
    strided = lambda a: dev(np.concatenate([a, rng.uniform(-9, 9, (len(a), 1)).astype(a.dtype)], 1))[:, :3]
    transposed = lambda a: dev(a.T.copy()).T                                        # coordinates not contiguous: copied by the wrapper
    base_p, base_d = None, None
    for name, points, make in (("float32", p32, dev), ("float64 of the same values", p32.astype(np.float64), dev),
                               ("float32 [N, 4][:, :3]", p32, strided), ("float64 [N, 4][:, :3]", p32.astype(np.float64), strided),
                               ("float32 transposed", p32, transposed)):
        assert make is dev or not make(points).is_contiguous()
        got = check_paint(points, mats, images, masks, what=name, make=make)
        d = check_depth(points, E, K, W, H, what=name, make=make)
        if base_p is None:
            base_p, base_d = got, d
        assert all(torch.equal(a, b) for a, b in zip(got, base_p)) and all(np.array_equal(a, b) for a, b in zip(d, base_d)), name
    p64 = rng.uniform(-20, 20, (500, 3)) + 1e-9                                     # not representable in float32
    assert not np.array_equal(p64, p64.astype(np.float32))
    check_paint(p64, mats, images, masks, what="float64 points")
    check_depth(p64, E, K, W, H, what="float64 points")
    # a float32 matrix gives what its float64 copy gives, [3, 4] what [4, 4] gives
    m32, E32, K32 = mats.astype(np.float32), E.astype(np.float32), K.astype(np.float32)
    a = L.paint_points(dev(p32), dev(m32), dev(images), dev(masks))
    for other in (dev(m32.astype(np.float64)), dev(m32)[:, :3], dev(m32.astype(np.float64))[:, :3]):
        assert all(torch.equal(x, y) for x, y in zip(a, L.paint_points(dev(p32), other, dev(images), dev(masks))))
    check_paint(p32, m32, images, masks, what="float32 matrices")
    a = L.depth_image(dev(p32), dev(E32), dev(K32), W, H)
    for e, k in ((dev(E32.astype(np.float64)), dev(K32.astype(np.float64))), (dev(E32)[:3], dev(K32)), (dev(E32), dev(K32.astype(np.float64)))):
        assert torch.equal(a, L.depth_image(dev(p32), e, k, W, H))
    check_depth(p32, E32, K32, W, H, what="float32 matrices")


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("n", [1, 2])
def test_a_column_strided_view_of_one_row_is_read_as_its_copy(n, dtype):
    """points = wide[:, ::2]: the coordinates are two elements apart.  One such row has no row stride to tell it by (torch reports any
    stride for a single row) and must be copied like two; read in place, (x, 50, y) lies outside every camera.  The backing rows hold
    six elements, so nothing is read outside the allocation either way.  Bitwise against the contiguous copy, and the restatement."""
    w, h = 32, 16
    points = np.array([[10.0, 0.5, 0.2], [8.0, -1.0, -0.3]], dtype=dtype)[:n]
    cams = [R.camera(yaw, 20.0, (0.0, 0.0, 0.0), w, h) for yaw in (0.0, 5.0)]
    mats, (_, E, K) = np.stack([c[0] for c in cams]), cams[0]
    images, masks = textures(2, w, h)

    def view(a):
        wide = torch.full((len(a), 6), 50.0, dtype=torch.from_numpy(a).dtype, device="cuda")
        wide[:, ::2] = dev(a)
        return wide[:, ::2]

    v = view(points)
    assert v.stride(1) == 2 and v.shape == (n, 3) and not v.is_contiguous() and torch.equal(v, dev(points))
    depth, index = L.depth_image(v, dev(E), dev(K), w, h, return_index=True)
    depth_c, index_c = L.depth_image(v.contiguous(), dev(E), dev(K), w, h, return_index=True)
    assert torch.equal(depth, depth_c) and torch.equal(index, index_c) and int((index >= 0).sum()) == n
    painted, painted_c = (L.paint_points(p, dev(mats), dev(images), dev(masks)) for p in (v, v.contiguous()))
    assert all(torch.equal(a, b) for a, b in zip(painted, painted_c)) and painted.count.tolist() == [2] * n
    check_depth(points, E, K, w, h, what=f"one column-strided view, N={n}", make=view)
    check_paint(points, mats, images, masks, what=f"one column-strided view, N={n}", make=view)


# ---- channel order and partial inputs -------------------------------------------------------------------------------------------------
def test_channel_order_and_partial_inputs():
    pts = R.sweep(np.random.default_rng(13), 900)
    mats, (images, masks) = ring(3), textures(3)
    both = check_paint(pts, mats, images, masks, "bgr", what="images and masks")
    rgb_order = check_paint(pts, mats, images, masks, "rgb", what="channel_order rgb")
    assert torch.equal(rgb_order.rgb, both.rgb.flip(1)) and torch.equal(rgb_order.labels, both.labels)
    flipped = check_paint(pts, mats, images[..., ::-1], masks, "rgb", what="flipped images, rgb")
    assert torch.equal(flipped.rgb, both.rgb)
    only_images = check_paint(pts, mats, images, None, what="images only")
    only_masks = check_paint(pts, mats, None, masks, what="masks only")
    squeezed = check_paint(pts, mats, None, masks[..., 0], what="masks [C, H, W]")
    assert torch.equal(only_images.rgb, both.rgb) and torch.equal(only_masks.labels, both.labels) and torch.equal(squeezed.labels, both.labels)
    for part in (only_images, only_masks, squeezed):
        assert torch.equal(part.fov, both.fov) and torch.equal(part.count, both.count)
    assert int(both.fov.sum()) > 300 and int((both.count > 1).sum()) > 20


# ---- the first camera ------------------------------------------------------------------------------------------------------------------
def test_the_label_is_the_first_seeing_cameras():
    pts = R.sweep(np.random.default_rng(14), 600)
    one = ring(1)
    mats = np.concatenate([one, one])                        # identical geometry
    masks = np.stack([np.full((H, W, 1), 3, np.uint8), np.full((H, W, 1), 9, np.uint8)])
    a = check_paint(pts, mats, None, masks, what="first camera (3, 9)")
    b = check_paint(pts, mats, None, masks[::-1], what="first camera (9, 3)")
    fov = host(a.fov)
    assert 50 < fov.sum() < 550 and set(host(a.count)) == {0, 2}
    assert np.array_equal(host(a.labels), np.where(fov, 3, 0)) and np.array_equal(host(b.labels), np.where(fov, 9, 0))
    # a camera that does not see the point is passed over: behind one that looks the other way the second camera labels
    turned = one.copy()
    turned[0, :3] = -turned[0, :3]
    c = check_paint(pts, np.concatenate([turned, one]), None, masks, what="a turned camera first")
    by_turned = host(L.paint_points(dev(pts), dev(turned), None, dev(masks[:1])).fov)
    assert not (fov & by_turned).any() and np.array_equal(host(c.labels), np.where(fov, 9, np.where(by_turned, 3, 0)))


# ---- scale and return_index -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 0.005])
def test_scale_and_return_index(scale):
    pts = R.sweep(np.random.default_rng(15), 3000)
    _, E, K = R.camera(20.0, 30.0, (0.1, -0.2, 0.3), W, H)
    got, index = check_depth(pts, E, K, W, H, scale=scale, what=f"scale {scale}")
    alone = L.depth_image(dev(pts), dev(E), dev(K), W, H, scale=scale)
    assert isinstance(alone, torch.Tensor) and np.array_equal(host(alone), got)
    unscaled = host(L.depth_image(dev(pts), dev(E), dev(K), W, H))
    assert np.array_equal(got, unscaled * np.float32(scale)) and (index >= 0).sum() > 300
    hit = index >= 0
    with np.errstate(all="ignore"):
        cam = [R.row34(E[r], pts.astype(np.float64)) for r in range(3)]
    assert np.array_equal(unscaled[..., 0][hit], R.row33(K[2], cam)[index[hit]].astype(np.float32))


# ---- reproducibility -------------------------------------------------------------------------------------------------------------------
def test_runs_and_graph_replays_are_bitwise_equal():
    rng = np.random.default_rng(16)
    pts = dev(R.sweep(rng, 4000))
    other = dev(R.sweep(rng, 4000))
    mats, (images, masks) = dev(ring(3)), tuple(dev(a) for a in textures(3))
    _, E, K = (dev(a) for a in R.camera(20.0, 30.0, (0.1, -0.2, 0.3), W, H))
    run = lambda p: (*L.depth_image(p, E, K, W, H, return_index=True), *L.paint_points(p, mats, images, masks))
    first, second, want_other = run(pts), run(pts), run(other)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    assert not torch.equal(first[0], want_other[0])
    static = pts.clone()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        run(static)
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        outs = run(static)
    for points, want in ((other, want_other), (pts, first), (pts, first)):
        static.copy_(points)
        for o in outs:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(outs, want))


# ---- the consumers -----------------------------------------------------------------------------------------------------------------------
def test_image_metrics_take_the_depth_image():
    rng = np.random.default_rng(17)
    pts = R.sweep(rng, 3000)
    _, E, K = R.camera(20.0, 30.0, (0.1, -0.2, 0.3), W, H)
    lidar_depth = L.depth_image(dev(pts), dev(E), dev(K), W, H)
    pred = dev(rng.uniform(0, 1, (H, W, 3)).astype(np.float32))
    gt = dev(rng.uniform(0, 1, (H, W, 3)).astype(np.float32))
    pred_depth = dev(rng.uniform(3, 30, (H, W, 1)).astype(np.float32))
    m = mtgs_amd.image_metrics(pred, gt, pred_depth=pred_depth, lidar_depth=lidar_depth)
    exact = mtgs_amd.image_metrics(pred, gt, pred_depth=lidar_depth.clone(), lidar_depth=lidar_depth)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(m[k])) for k in ("psnr", "depth_RMSE", "depth_absRel", "depth_delta1"))
    assert float(m["depth_RMSE"]) > 0 and float(exact["depth_RMSE"]) == 0


def test_painted_points_seed_the_cloud():
    """paint_points -> fov & (labels < 10) -> pointcloud.prepare_seed_cloud: the colour format goes straight in"""
    rng = np.random.default_rng(18)
    pts = np.concatenate([R.sweep(rng, 1500), R.sweep(rng, 1500)])               # two sweeps of one place
    pts[:, :2] = np.round(pts[:, :2] * 2) / 2 + rng.normal(0, 0.02, (3000, 2))  # clustered: the outlier filter keeps a good share
    mats, (images, masks) = ring(3), textures(3)
    points = dev(pts.astype(np.float32))
    painted = L.paint_points(points, dev(mats), dev(images), dev(masks))
    keep = painted.fov & (painted.labels < 10)
    assert 100 < int(keep.sum()) < int(painted.fov.sum())
    cloud = mtgs_amd.prepare_seed_cloud(points[keep], painted.rgb[keep], voxel_size=0.15)
    torch.cuda.synchronize()
    n = cloud["xyz"].shape[0]
    assert 0 < n <= int(keep.sum()) and cloud["xyz"].dtype == torch.float32 and cloud["rgb"].dtype == torch.uint8 and cloud["rgb"].shape == (n, 3)
    assert int(cloud["rgb"].max()) > 128 and bool(torch.isfinite(cloud["xyz"]).all())
    seeded = mtgs_amd.seed_gaussians(cloud, sh_degree=3)
    assert seeded["means"].shape == (n, 3)
