"""The two definitions of include/mtgs_brightness.h restated in NumPy (no torch), in exactly their operation order.

adjust_brightness: the 8-bit HSV round trip [RECALLED -- the project's definition, pinned by the known answers of
tests/test_brightness_host.py, not by OpenCV]: integers for RGB -> HSV, fp64 for the scaling, float32 arrays for HSV -> RGB so that
every operation rounds once.  estimate_factors: adjust_brightness_single_frame with the sample of tests/lidar_refs.paint_points (one
body on the device too) -- tests/golden/make_brightness_golden.py checks it against the reference's own function and records the
result in tests/golden/brightness_ref.npz; tests/test_brightness_host.py checks it against that record and
tests/test_gpu_brightness.py checks the kernels against it, bit for bit."""
from pathlib import Path

import numpy as np

from tests.lidar_refs import _f64, row34

GOLDEN = Path(__file__).resolve().parent / "golden" / "brightness_ref.npz"
NUPLAN_PAIRS = ((0, 1, 0), (0, 2, 1), (1, 3, 0), (2, 4, 1), (3, 5, 0), (4, 6, 1), (5, 7, 0), (6, 7, 1))
HSV_SHIFT = 12


def tables():
    """(sdiv, hdiv) int64 [256]: rint, ties to even, of the double quotients; entry 0 is 0"""
    i = np.arange(1, 256, dtype=np.float64)
    sdiv, hdiv = np.zeros(256, dtype=np.int64), np.zeros(256, dtype=np.int64)
    sdiv[1:] = np.rint((255 << HSV_SHIFT) / i).astype(np.int64)
    hdiv[1:] = np.rint((180 << HSV_SHIFT) / (6.0 * i)).astype(np.int64)
    return sdiv, hdiv


SDIV, HDIV = tables()


def rgb_to_hsv(rgb):
    """uint8 [..., 3] (r, g, b) -> int64 (h, s, v) arrays, 0 <= h < 180"""
    c = np.asarray(rgb).astype(np.int64)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    v, vmin = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    d = v - vmin
    s = (d * SDIV[v] + 2048) >> HSV_SHIFT
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * d, r - g + 4 * d))
    h = (h * HDIV[d] + 2048) >> HSV_SHIFT                      # NumPy's >> on a negative int64 is arithmetic
    h = np.where(h < 0, h + 180, h)
    return h, s, v


def scale_v(v, factor):
    """V' = (uint8) trunc(min(max(v * factor, 0), 255)) in fp64; a NaN product gives 0 (the defined deviation)"""
    with np.errstate(all="ignore"):
        x = v.astype(np.float64) * np.float64(factor)
        x = np.where(np.isnan(x), 0.0, np.minimum(np.maximum(x, 0.0), 255.0))
    return np.trunc(x).astype(np.int64)


def hsv_to_rgb(h, s, v):
    """int (h, s, v) -> uint8 [..., 3] (r, g, b): float32 throughout, one rounding per operation"""
    f32 = np.float32
    hf = h.astype(f32) * f32(6.0 / 180.0)
    sf = s.astype(f32) * (f32(1.0) / f32(255.0))
    vf = v.astype(f32) * (f32(1.0) / f32(255.0))
    fl = np.floor(hf)
    f = hf - fl
    sector = fl.astype(np.int64)
    one = f32(1.0)
    tab = np.stack([vf, vf * (one - sf), vf * (one - sf * f), vf * (one - sf * (one - f))], axis=-1)
    assert tab.dtype == np.float32
    order = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])       # (b, g, r) per sector
    assert sector.min() >= 0 and sector.max() <= 5
    bgr = np.take_along_axis(tab, order[sector], axis=-1)
    bgr = np.where((s == 0)[..., None], vf[..., None], bgr)
    byte = np.clip(np.rint(bgr * f32(255.0)), 0, 255).astype(np.uint8)
    return byte[..., ::-1]


def adjust_brightness(images, factors, channel_order="rgb"):
    """uint8 [h, w, 3] with one factor, or [C, h, w, 3] with one factor or C of them -> uint8 of the same shape"""
    img = np.asarray(images)
    assert img.dtype == np.uint8 and img.shape[-1] == 3
    fac = np.asarray(factors, dtype=np.float64)
    if fac.ndim == 1:
        assert img.ndim == 4 and fac.shape[0] == img.shape[0]
        return np.stack([adjust_brightness(img[c], fac[c], channel_order) for c in range(img.shape[0])])
    rgb = (img[..., ::-1] if channel_order == "bgr" else img).reshape(-1, 3)
    out = np.empty_like(rgb)
    for at in range(0, rgb.shape[0], 1 << 20):                     # a million pixels at a time: the intermediates stay small
        h, s, v = rgb_to_hsv(rgb[at:at + (1 << 20)])
        out[at:at + (1 << 20)] = hsv_to_rgb(h, s, scale_v(v, fac))
    out = out.reshape(img.shape)
    return np.ascontiguousarray(out[..., ::-1] if channel_order == "bgr" else out)


def unit_float(x):
    """(float)byte / 255.0f, one correctly rounded float32 division"""
    return np.asarray(x).astype(np.float32) / np.float32(255.0)


# ---- the estimate -----------------------------------------------------------------------------------------------------------------
def numpy_sum(a):
    """np.add.reduce of a contiguous float64 array of at most 128 values, restated: NumPy's pairwise sum below its block size"""
    a = [np.float64(x) for x in a]
    n = len(a)
    assert n <= 128
    if n < 8:
        res = np.float64(0.0)
        for x in a:
            res = res + x
        return res
    r = a[:8]
    i = 8
    while i + 8 <= n:
        r = [r[j] + a[i + j] for j in range(8)]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for x in a[i:]:
        res = res + x
    return res


def sample_v(points, lidar2imgs, images):
    """(see bool [C, N], V int64 [C, N]): per camera the field-of-view test and V = max_k (uint8) trunc(value_k * 255.0) of the
    bilinear sample, the operations of tests/lidar_refs.paint_points"""
    x, mats, images = _f64(points).reshape(-1, 3), _f64(lidar2imgs), np.asarray(images)
    C, (h, w) = mats.shape[0], images.shape[1:3]
    see_all, v_all = np.zeros((C, x.shape[0]), dtype=bool), np.zeros((C, x.shape[0]), dtype=np.int64)
    with np.errstate(all="ignore"):
        for c in range(C):
            p = [row34(mats[c, r], x) for r in range(3)]
            see = p[2] > 0.1
            z = np.minimum(np.maximum(p[2], 1e-5), 99999.0)
            nx, ny = (p[0] / z) / w, (p[1] / z) / h
            see &= (nx < 1) & (nx >= 0) & (ny < 1) & (ny >= 0)
            s = np.nonzero(see)[0]
            ix = (((nx[s] * 2 - 1) + 1) / 2) * (w - 1)
            iy = (((ny[s] * 2 - 1) + 1) / 2) * (h - 1)
            xf, yf = np.floor(ix), np.floor(iy)
            fx, fy = ix - xf, iy - yf
            x0, y0 = np.clip(xf.astype(np.int64), 0, w - 1), np.clip(yf.astype(np.int64), 0, h - 1)
            x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
            t = lambda yy, xx: images[c][yy, xx].astype(np.float64) / 255.0
            w00, w01, w10, w11 = ((1 - fx) * (1 - fy))[:, None], (fx * (1 - fy))[:, None], ((1 - fx) * fy)[:, None], (fx * fy)[:, None]
            value = ((t(y0, x0) * w00 + t(y0, x1) * w01) + t(y1, x0) * w10) + t(y1, x1) * w11
            see_all[c] = see
            v_all[c, s] = (value * 255.0).astype(np.uint8).astype(np.int64).max(axis=1) if s.size else 0
    return see_all, v_all


def strip_columns(w, strip, left):
    """Python's [:strip] (left) or [-strip:] of w columns"""
    return range(w)[:strip] if left else range(w)[-strip:]


def pair_stats(points, lidar2imgs, images, pairs=NUPLAN_PAIRS, strip=100):
    """int64 [P, 5] = n, s1, s2, strip1, strip2 per pair"""
    images = np.asarray(images)
    see, V = sample_v(points, lidar2imgs, images)
    w = images.shape[2]
    vmax = images.max(axis=-1).astype(np.int64)                                    # [C, h, w]
    out = np.zeros((len(pairs), 5), dtype=np.int64)
    for p, (a, b, side) in enumerate(pairs):
        both = see[a] & see[b]
        ca, cb = strip_columns(w, strip, side == 0), strip_columns(w, strip, side != 0)
        out[p] = (both.sum(), V[a][both].sum(), V[b][both].sum(), vmax[a][:, ca.start:ca.stop].sum(), vmax[b][:, cb.start:cb.stop].sum())
    return out


def solve_factors(stats, C, h, w, pairs=NUPLAN_PAIRS, strip=100, min_overlap=10):
    """float64 [C]: the reference's chain over the pairs in fp64, then the division by NumPy's mean"""
    f64 = np.float64
    factor, has = [f64(1.0)] * C, {0}
    n_strip = f64(h * min(strip, w))
    with np.errstate(all="ignore"):
        for (a, b, _), (n, s1, s2, t1, t2) in zip(pairs, np.asarray(stats).tolist()):
            if n >= min_overlap:
                v_ratio = (f64(s1) / f64(n)) / (f64(s2) / f64(n))
            else:
                v_ratio = (f64(t1) / n_strip) / (f64(t2) / n_strip)
            ratio = (factor[a] if a in has else f64(1.0)) * v_ratio
            factor[b] = (factor[b] + ratio) / f64(2.0) if b in has else ratio
            has.add(b)
        mean = numpy_sum(factor) / f64(C)
        return np.array([x / mean for x in factor], dtype=np.float64)


def estimate_factors(points, lidar2imgs, images, pairs=NUPLAN_PAIRS, strip=100, min_overlap=10):
    """(factors float64 [C], stats int64 [P, 5])"""
    images = np.asarray(images)
    stats = pair_stats(points, lidar2imgs, images, pairs, strip)
    return solve_factors(stats, images.shape[0], images.shape[1], images.shape[2], pairs, strip, min_overlap), stats


def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}
