"""A NumPy restatement of mtgs_amd.frame (include/mtgs_frame.h): the reference of tests/test_frame_host.py and
tests/test_gpu_frame.py, written from the definitions, without PIL and without mtgs_amd.

  * weights / coefficients: Pillow's precompute_coeffs (and normalize_coeffs_8bpc) for the BILINEAR filter, in Python floats
  * bilinear_u8: the two-pass 8-bit resample, clip8((2^21 + sum k px) >> 22) per pass, ROUNDED to uint8 between the passes
  * bilinear_f32: mode "F": ss = 0.0; ss += (double)px * k in tap order, every product and sum rounded once (NumPy does not fuse),
    the horizontal result rounded to float32 before the vertical pass
  * nearest: the source index by REPEATED ADDITION of in / out in double, then a gather
  * frame_masks: the panoptic split, the invalid fills and the label mask at FULL size, as custom_dataset.py:203-274 has them
A pass whose size does not change is the identity.  tests/test_frame_host.py compares all of it with Pillow bit for bit.

frame_inputs(seed, h, w) draws the planes every test and tests/golden/make_frame_golden.py use: an RGB image with a saturated 0
corner, a saturated 255 corner and a one-pixel checkerboard band (the clip8 and rounding edges), a depth in [0, 6e4] with exact
zeros, a semantic map with 255s, an instance map above 2^16 and a bool mask.
"""
import zlib

import numpy as np

BITS = 22
GOLDEN_SHAPES = (((37, 53), (18, 26)), ((37, 53), (27, 39)), ((64, 100), (64, 50)), ((9, 9), (4, 9)), ((9, 9), (9, 4)), ((31, 47), (46, 70)),
                 ((5, 7), (1, 1)), ((400, 7), (3, 7)), ((7, 400), (7, 3)))         # ((h, w), (out h, out w))


def frame_inputs(seed, h, w):
    rng = np.random.default_rng([seed, h, w])
    image = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    image[:h // 3, :w // 3] = 0
    image[h - h // 3:, w - w // 3:] = 255
    band = (yy >= h // 3) & (yy < h - h // 3) & (xx < w // 2)
    image[band] = (255 * ((yy + xx) & 1)).astype(np.uint8)[band][:, None]
    depth = rng.uniform(0.0, 6e4, (h, w)).astype(np.float32)
    depth[rng.random((h, w)) < 0.2] = 0.0
    semantic = rng.integers(0, 20, (h, w), dtype=np.uint8)
    semantic[rng.random((h, w)) < 0.1] = 255
    instance = rng.integers(0, 70000, (h, w), dtype=np.int32)
    mask = rng.random((h, w)) < 0.5
    return {"image": image, "depth": depth, "semantic_map": semantic, "instance_map": instance, "mask": mask}


def checksum(planes):
    """crc32 over the planes of frame_inputs, in key order: tells a changed random stream from a changed resampler"""
    crc = 0
    for key in sorted(planes):
        crc = zlib.crc32(np.ascontiguousarray(planes[key]).tobytes(), crc)
    return crc


# ---- BILINEAR ----------------------------------------------------------------------------------------------------------------------
def weights(in_size, out_size):
    """per output position (xmin, [normalised double weights]): precompute_coeffs with the triangle filter of support 1"""
    scale = in_size / out_size
    filterscale = scale if scale > 1.0 else 1.0
    support = 1.0 * filterscale
    ss = 1.0 / filterscale
    out = []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        k, ww = [], 0.0
        for x in range(xmax):
            v = (x + xmin - center + 0.5) * ss
            if v < 0.0:
                v = -v
            v = 1.0 - v if v < 1.0 else 0.0
            k.append(v)
            ww += v
        if ww != 0.0:
            k = [v / ww for v in k]
        out.append((xmin, k))
    return out


def coefficients(in_size, out_size):
    """normalize_coeffs_8bpc: (xmin, [int(0.5 + w 2^22)]); the weights of this filter are never negative"""
    return [(xmin, [int(0.5 + v * (1 << BITS)) for v in k]) for xmin, k in weights(in_size, out_size)]


def _pass_u8(img, out_size, axis):
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((out_size,) + src.shape[1:], np.uint8)
    for xx, (xmin, k) in enumerate(coefficients(src.shape[0], out_size)):
        acc = np.full(src.shape[1:], 1 << (BITS - 1), np.int64)
        for j, kk in enumerate(k):
            acc += src[xmin + j] * kk
        out[xx] = np.clip(acc >> BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def bilinear_u8(img, oh, ow):
    """uint8 [H, W] or [H, W, C] -> [oh, ow(, C)]: horizontal, rounded to 8 bits, then vertical"""
    x = img if ow == img.shape[1] else _pass_u8(img, ow, 1)
    return np.ascontiguousarray(x if oh == img.shape[0] else _pass_u8(x, oh, 0))


def _pass_f32(img, out_size, axis):
    src = np.moveaxis(img, axis, 0)
    out = np.empty((out_size,) + src.shape[1:], np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for xx, (xmin, k) in enumerate(weights(src.shape[0], out_size)):
            ss = np.zeros(src.shape[1:], np.float64)
            for j, kk in enumerate(k):
                ss = ss + src[xmin + j].astype(np.float64) * np.float64(kk)
            out[xx] = ss.astype(np.float32)
    return np.moveaxis(out, 0, axis)


def bilinear_f32(img, oh, ow):
    """float32 [H, W] -> [oh, ow]"""
    x = img if ow == img.shape[1] else _pass_f32(img, ow, 1)
    return np.ascontiguousarray(x if oh == img.shape[0] else _pass_f32(x, oh, 0))


def to_float(img_u8):
    """get_gt_img: one correctly rounded float32 division per byte"""
    return img_u8.astype(np.float32) / np.float32(255.0)


# ---- NEAREST -----------------------------------------------------------------------------------------------------------------------
def nearest_index(in_size, out_size):
    step = in_size / out_size
    out, xo = [], step * 0.5
    for _ in range(out_size):
        out.append(min(int(xo), in_size - 1))
        xo += step
    return np.array(out, np.int64)


def nearest(img, oh, ow):
    return np.ascontiguousarray(img[nearest_index(img.shape[0], oh)][:, nearest_index(img.shape[1], ow)])


def resize_frame(data, oh, ow, image_float=False):
    """_resize_data over a dict of arrays"""
    out = {}
    for key, x in data.items():
        flat = x[..., 0] if x.ndim == 3 and x.shape[2] == 1 else x
        if key == "image":
            r = bilinear_u8(flat, oh, ow)
            r = to_float(r) if image_float else r
        elif key == "depth":
            r = bilinear_f32(flat, oh, ow)
        else:
            r = nearest(flat, oh, ow)
        out[key] = r[..., None] if flat is not x else r
    return out


# ---- the masks, at full size ---------------------------------------------------------------------------------------------------------
def frame_masks(panoptic=None, semantic=None, valid=None, labels=(255,)):
    """(instance_map int32 [H, W, 1] or None, semantic_map uint8 [H, W, 1], mask bool [H, W, 1])"""
    instance = None
    if panoptic is not None:
        p = panoptic.astype(np.int32)
        instance = (p[:, :, 0] + p[:, :, 1] * 256)[:, :, None]
        sem = panoptic[:, :, 2][:, :, None].copy()
    else:
        sem = semantic.reshape(semantic.shape[0], semantic.shape[1], 1).copy()
    ok = np.ones(sem.shape, bool) if valid is None else valid.reshape(sem.shape).astype(bool)
    if instance is not None:
        instance[~ok] = 0
    sem[~ok] = 255
    mask = ok & np.logical_not(np.isin(sem, list(labels)))
    return instance, sem, mask
