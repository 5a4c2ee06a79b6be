"""The re-distortion of a rendered frame into the raw camera, restated in NumPy (include/mtgs_redistort.h has the same definition).

[RECALLED] cv2 was not available to run: this is OpenCV's rule as recalled -- initInverseRectificationMap(K, D, None, K', size) as a
fixed number of fixed-point iterations of the inverse lens model, followed by remap with INTER_LINEAR on an 8-bit image,
BORDER_CONSTANT 0 -- and it is the project's DEFINITION, not a claim about OpenCV's bytes.  tests/test_redistort_host.py pins it with
known answers that need no recall.  The sampling is tests/undistort_refs.py's remap_linear, unchanged; a float32 source is converted
tap by tap BEFORE the interpolation, by tests/jpeg_refs.py's to_u8.

K = (fx, fy, cx, cy) is the RAW camera (the image that is written), new_K = (fx', fy', cx', cy') the camera of the image that is
read, D = (k1, k2, p1, p2[, k3]); sizes are (rows, columns)."""
import numpy as np

from tests import jpeg_refs, undistort_refs

MAX_ITERATIONS = 64


def inverse_points(K, D, px, py, iterations=5):
    """raw pixels (px, py: arrays of one shape) -> normalised undistorted coordinates (x, y): `iterations` fixed-point iterations of
    the inverse model in fp64, one rounding per operation, in the header's order.  A point whose 1 / (1 + radial) turns negative --
    the model has folded over -- goes back to its start (x0, y0) and stops there; the others go on."""
    if not 0 <= iterations <= MAX_ITERATIONS:
        raise ValueError(f"iterations outside [0, {MAX_ITERATIONS}]: {iterations}")
    fx, fy, cx, cy = (np.float64(v) for v in K)
    k1, k2, p1, p2, k3 = (np.float64(v) for v in undistort_refs.coefficients(D))
    with np.errstate(all="ignore"):
        x0, y0 = np.broadcast_arrays((np.asarray(px, np.float64) - cx) / fx, (np.asarray(py, np.float64) - cy) / fy)
        x, y = x0.copy(), y0.copy()
        live = np.ones(x0.shape, bool)
        for _ in range(iterations):
            r2 = x * x + y * y
            icdist = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
            folded = live & (icdist < 0)
            dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
            dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
            step = live & ~folded
            x, y = np.where(step, (x0 - dx) * icdist, np.where(folded, x0, x)), np.where(step, (y0 - dy) * icdist, np.where(folded, y0, y))
            live = step
    return x, y


def redistort_map(K, D, new_K, H, W, iterations=5):
    """float32 [H, W, 2] = (mapx, mapy) over the RAW image of H x W: where each of its pixels lies in the image that is read"""
    nfx, nfy, ncx, ncy = (np.float64(v) for v in new_K)
    x, y = inverse_points(K, D, np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None], iterations)
    x, y = np.broadcast_arrays(x, y)
    with np.errstate(all="ignore"):
        return np.stack([(nfx * x + ncx).astype(np.float32), (nfy * y + ncy).astype(np.float32)], axis=-1)


def forward_pixels(K, D, x, y):
    """include/mtgs_undistort.h's closed form: normalised undistorted (x, y) -> raw pixels, fp64"""
    fx, fy, cx, cy = (np.float64(v) for v in K)
    k1, k2, p1, p2, k3 = (np.float64(v) for v in undistort_refs.coefficients(D))
    x2, y2 = x * x, y * y
    r2 = x2 + y2
    _2xy = 2.0 * x * y
    kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
    xd = x * kr + p1 * _2xy + p2 * (r2 + 2.0 * x2)
    yd = y * kr + p1 * (r2 + 2.0 * y2) + p2 * _2xy
    return fx * xd + cx, fy * yd + cy


def to_u8(img, conversion="truncate"):
    """the source as the taps see it: uint8 as it is, float32 through the JPEG encoder's conversion"""
    img = np.asarray(img)
    return img if img.dtype == np.uint8 else jpeg_refs.to_u8(img, conversion)


def remap(img, m, conversion="truncate"):
    """uint8 or float32 [h, w(, C)] through the map m [H, W, 2] -> uint8 [H, W(, C)]"""
    return undistort_refs.remap_linear(to_u8(img, conversion), m)


def redistort_image(img, K, D, new_K, size, iterations=5, conversion="truncate"):
    """mtgs_amd.undistort.redistort_image: `size` = (H, W) of the raw image that is written; K and new_K are the map's own"""
    return remap(img, redistort_map(K, D, new_K, size[0], size[1], iterations), conversion)
