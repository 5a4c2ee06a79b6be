"""The two definitions of include/mtgs_lidar.h restated in NumPy, in exactly their operation order: every product and sum is an
element-wise fp64 operation of its own (no matmul, so no BLAS summation order), and "the largest index wins" is np.maximum.at.
tests/golden/make_lidar_golden.py checks this restatement against the reference's own functions and records the result in
tests/golden/lidar_ref.npz; tests/test_lidar_host.py checks it against that record and tests/test_gpu_lidar.py checks the kernels
against it."""
from pathlib import Path
from typing import NamedTuple, Optional

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden" / "lidar_ref.npz"


class Painted(NamedTuple):
    rgb: Optional[np.ndarray]
    labels: Optional[np.ndarray]
    fov: np.ndarray
    count: np.ndarray


def _f64(a):
    return np.asarray(a).astype(np.float64)         # float32 -> float64 is exact


def row34(m, x):
    """((m0 x0 + m1 x1) + m2 x2) + m3 for points x [N, 3]"""
    return ((m[0] * x[:, 0] + m[1] * x[:, 1]) + m[2] * x[:, 2]) + m[3]


def row33(k, c):
    return (k[0] * c[0] + k[1] * c[1]) + k[2] * c[2]


def depth_image(points, lidar2cam, K, width, height, scale=1.0, return_index=False):
    x, m, k = _f64(points).reshape(-1, 3), _f64(lidar2cam), _f64(K)
    winner = np.full(height * width, -1, dtype=np.int64)
    q2_all = np.zeros(x.shape[0])
    with np.errstate(all="ignore"):
        cam = [row34(m[r], x) for r in range(3)]
        q = [row33(k[r], cam) for r in range(3)]
        u, v = q[0] / q[2], q[1] / q[2]
        keep = (cam[2] > 0) & (v >= 0) & (v < height) & (u >= 0) & (u < width)      # every comparison is false on NaN
        idx = np.nonzero(keep)[0]
        pix = v[idx].astype(np.int64) * width + u[idx].astype(np.int64)             # truncation, after the tests
        q2_all = q[2]
    np.maximum.at(winner, pix, idx)
    hit = winner >= 0
    depth = np.zeros(height * width, dtype=np.float32)
    depth[hit] = q2_all[winner[hit]].astype(np.float32)
    depth = depth * np.float32(scale)
    depth = depth.reshape(height, width, 1)
    return (depth, winner.astype(np.int32).reshape(height, width)) if return_index else depth


def paint_points(points, lidar2imgs, images=None, sem_masks=None, channel_order="bgr"):
    x, mats = _f64(points).reshape(-1, 3), _f64(lidar2imgs)
    N, C = x.shape[0], mats.shape[0]
    if images is not None:
        images = np.asarray(images)
        h, w = images.shape[1:3]
    if sem_masks is not None:
        sem_masks = np.asarray(sem_masks).reshape(C, *np.asarray(sem_masks).shape[1:3])
        h, w = sem_masks.shape[1:3]
    assert images is not None or sem_masks is not None, "the image size comes from the images or the masks"
    total = np.zeros((N, 3))
    count = np.zeros(N, dtype=np.int32)
    labels = np.zeros(N, dtype=np.int32)
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
            if sem_masks is not None:
                first = count[s] == 0
                lx = np.clip(np.rint(ix[first]).astype(np.int64), 0, w - 1)        # np.rint: ties to even
                ly = np.clip(np.rint(iy[first]).astype(np.int64), 0, h - 1)
                labels[s[first]] = sem_masks[c, ly, lx]
            if images is not None:
                xf, yf = np.floor(ix), np.floor(iy)
                fx, fy = ix - xf, iy - yf
                x0, y0 = np.clip(xf.astype(np.int64), 0, w - 1), np.clip(yf.astype(np.int64), 0, h - 1)
                x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)      # beyond the image only with weight 0
                img = images[c][..., ::-1] if channel_order == "bgr" else images[c]
                t = lambda yy, xx: img[yy, xx].astype(np.float64) / 255.0
                w00, w01, w10, w11 = ((1 - fx) * (1 - fy))[:, None], (fx * (1 - fy))[:, None], ((1 - fx) * fy)[:, None], (fx * fy)[:, None]
                value = ((t(y0, x0) * w00 + t(y0, x1) * w01) + t(y1, x0) * w10) + t(y1, x1) * w11
                total[s] = total[s] + value
            count[s] += 1
    fov = count > 0
    rgb = None
    if images is not None:
        rgb = np.zeros((N, 3))
        rgb[fov] = total[fov] / count[fov][:, None].astype(np.float64)
    return Painted(rgb, labels if sem_masks is not None else None, fov, count)


def camera(yaw_deg, f, offset, width, height):
    """(lidar -> image [4, 4], lidar -> camera [4, 4], K [3, 3]) of a camera looking along (cos yaw, sin yaw, 0) of the lidar
    frame, x to its right, y down, the principal point in the middle"""
    a = np.deg2rad(yaw_deg)
    E = np.eye(4)
    E[:3, :3] = [[np.sin(a), -np.cos(a), 0.0], [0.0, 0.0, -1.0], [np.cos(a), np.sin(a), 0.0]]
    E[:3, 3] = offset
    K = np.eye(4)
    K[0, 0] = K[1, 1] = f
    K[0, 2], K[1, 2] = width / 2, height / 2
    return K @ E, E, K[:3, :3]


def sweep(rng, n):
    """n float32 points of a ring of 3 to 30 m around the sensor, 2 m below to 4 m above it"""
    r, a = rng.uniform(3.0, 30.0, n), rng.uniform(0.0, 2 * np.pi, n)
    return np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-2.0, 4.0, n)], -1).astype(np.float32)


def ulp_distance_f32(a, b):
    """the largest distance in float32 units in the last place between two finite float32 arrays"""
    def key(v):
        i = np.ascontiguousarray(v, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    a, b = np.asarray(a), np.asarray(b)
    return int(np.abs(key(a) - key(b)).max()) if a.size else 0


def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}
