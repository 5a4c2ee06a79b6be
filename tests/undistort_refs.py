"""The lens undistortion of a training frame, restated in NumPy (include/mtgs_undistort.h has the same definition).

[RECALLED] cv2 was not available to run: this is OpenCV's rule as recalled -- initUndistortRectifyMap(K, D, None, K', size, CV_32FC2)
followed by remap with INTER_LINEAR / INTER_NEAREST on 8-bit planes, BORDER_CONSTANT 0 -- and it is the project's DEFINITION, not a
claim about OpenCV's bytes.  tests/test_undistort_host.py pins it with known answers that need no recall (identity, integer shifts,
half-pixel averages, the rounding ties).  Everything after the one fp64 map is integer arithmetic.

K = (fx, fy, cx, cy), D = (k1, k2, p1, p2[, k3]), new_K = (fx', fy', cx', cy'); sizes are (rows, columns)."""
import numpy as np

FAR = -(1 << 30)            # the coordinate of a map entry that is non-finite or has !(|f| < 2^30): outside every source
SHIFT, ONE = 5, 32          # INTER_BITS: five fractional bits


def coefficients(D):
    d = [float(v) for v in D]
    if len(d) not in (4, 5):
        raise ValueError(f"D must have 4 or 5 coefficients, got {len(d)}")
    k1, k2, p1, p2 = d[:4]
    return k1, k2, p1, p2, (d[4] if len(d) == 5 else 0.0)


def undistort_map(K, D, new_K, H, W):
    """float32 [H, W, 2] = (mapx, mapy): fp64, one rounding per operation, in the header's order, then one rounding to float32"""
    fx, fy, cx, cy = (np.float64(v) for v in K)
    nfx, nfy, ncx, ncy = (np.float64(v) for v in new_K)
    k1, k2, p1, p2, k3 = (np.float64(v) for v in coefficients(D))
    j = np.arange(W, dtype=np.float64)[None, :]
    i = np.arange(H, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        x, y = np.broadcast_arrays((j - ncx) / nfx, (i - ncy) / nfy)
        x2, y2 = x * x, y * y
        r2 = x2 + y2
        _2xy = 2.0 * x * y
        kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
        xd = x * kr + p1 * _2xy + p2 * (r2 + 2.0 * x2)
        yd = y * kr + p1 * (r2 + 2.0 * y2) + p2 * _2xy
        return np.stack([(fx * xd + cx).astype(np.float32), (fy * yd + cy).astype(np.float32)], axis=-1)


def _coord(f):
    """integral float32 -> int64, FAR where !(|f| < 2^30) (NaN and infinities included)"""
    with np.errstate(invalid="ignore"):
        near = np.abs(f) < np.float32(2.0 ** 30)
    return np.where(near, np.where(near, f, 0).astype(np.int64), FAR)


def fixed(m):
    """rint(m * 32.0f) in float32, ties to even, as an integer: sx or sy"""
    with np.errstate(all="ignore"):
        return _coord(np.rint(m.astype(np.float32) * np.float32(ONE)))


def nearest_index(m):
    return _coord(np.rint(m.astype(np.float32)))


def _taps(src, iy, ix):
    """src [h, w, C] at integer coordinates [H, W], 0 outside, as int64 [H, W, C]"""
    h, w = src.shape[:2]
    inside = (iy >= 0) & (iy < h) & (ix >= 0) & (ix < w)
    v = src[np.clip(iy, 0, h - 1), np.clip(ix, 0, w - 1)].astype(np.int64)
    return np.where(inside[..., None], v, 0), inside


def _with_channels(img):
    img = np.asarray(img)
    return (img[:, :, None], True) if img.ndim == 2 else (img, False)


def remap_linear(img, m):
    """uint8 [h, w] or [h, w, C] through the map m [H, W, 2] -> uint8 [H, W(, C)]"""
    src, flat = _with_channels(img)
    assert src.dtype == np.uint8
    sx, sy = fixed(m[..., 0]), fixed(m[..., 1])
    ix, iy, a, b = sx >> SHIFT, sy >> SHIFT, (sx & (ONE - 1))[..., None], (sy & (ONE - 1))[..., None]
    total = ((ONE - a) * (ONE - b) * ONE * _taps(src, iy, ix)[0] + a * (ONE - b) * ONE * _taps(src, iy, ix + 1)[0]
             + (ONE - a) * b * ONE * _taps(src, iy + 1, ix)[0] + a * b * ONE * _taps(src, iy + 1, ix + 1)[0])
    out = ((total + 16384) >> 15).astype(np.uint8)
    return out[..., 0] if flat else out


def remap_nearest(img, m):
    """uint8 / int32 / bool [h, w(, C)] through the map -> [H, W(, C)], 0 outside"""
    src, flat = _with_channels(img)
    v, _ = _taps(src, nearest_index(m[..., 1]), nearest_index(m[..., 0]))
    out = v.astype(src.dtype)
    return out[..., 0] if flat else out


def valid_mask(m, h, w, ego=None):
    """bool [H, W, 1]: the nearest remap of an all-255 plane, astype(bool); with `ego` (nonzero on the ego vehicle) also ego == 0 there"""
    plane = np.full((h, w), 255, np.uint8) if ego is None else np.where(np.asarray(ego).reshape(h, w) != 0, 0, 255).astype(np.uint8)
    return remap_nearest(plane, m).astype(bool)[:, :, None]


def to_float(img_u8):
    return img_u8.astype(np.float32) / np.float32(255.0)


def undistort_frame(K, D, new_K, size, image=None, ego_mask=None, panoptic=None, semantic=None, image_float=False):
    """the planes of mtgs_amd.undistort.undistort_frame; K and new_K are the map's own (no half-pixel bookkeeping here)"""
    m = undistort_map(K, D, new_K, *size)
    first = next(v for v in (image, ego_mask, panoptic, semantic) if v is not None)
    h, w = first.shape[:2]
    out = {"valid_mask": valid_mask(m, h, w, ego_mask)}
    if image is not None:
        out["image"] = remap_linear(image, m)
        if image_float:
            out["image"] = to_float(out["image"])
    if panoptic is not None:
        out["panoptic"] = remap_nearest(panoptic, m)
    if semantic is not None:
        out["semantic"] = remap_nearest(semantic, m)
    return out


def outside_share(K, D, new_K, size, h, w):
    """the share of destination pixels whose nearest source pixel is outside the source"""
    return 1.0 - float(valid_mask(undistort_map(K, D, new_K, *size), h, w).mean())


# ---- the new camera matrix [RECALLED]: getOptimalNewCameraMatrix -----------------------------------------------------------------
def undistort_points(K, D, pts, iterations=5):
    """pixels [N, 2] -> normalised undistorted coordinates [N, 2]: the fixed-point iteration of the inverse model, fp64"""
    fx, fy, cx, cy = (float(v) for v in K)
    k1, k2, p1, p2, k3 = coefficients(D)
    x0, y0 = (pts[:, 0] - cx) / fx, (pts[:, 1] - cy) / fy
    x, y = x0.copy(), y0.copy()
    for _ in range(iterations):
        r2 = x * x + y * y
        icdist = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
        x, y = (x0 - dx) * icdist, (y0 - dy) * icdist
    return np.stack([x, y], axis=1)


def grid_points(h, w, n=9):
    g = np.arange(n, dtype=np.float64)
    xs, ys = np.meshgrid(g * (w - 1) / (n - 1), g * (h - 1) / (n - 1))
    return np.stack([xs.ravel(), ys.ravel()], axis=1)             # row-major: index y * n + x
