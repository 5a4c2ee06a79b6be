"""The crop decision of include/mtgs_crop.h (mtgs_crop_select) written out in NumPy fp32, and the inputs the host and the GPU
tests share.  NumPy rounds every fp32 operation once and fuses nothing, which is the stated arithmetic."""
import functools

import numpy as np

RPY, POS, SIZE = (0.3, -0.2, 1.1), (3.0, -2.0, 1.0), (40.0, 10.0, 25.0)
EXTENT = (50.0, 7.5, 50.0)


def within_np(points, box15):
    """bool [N]: q_k = ((m_k0 x + m_k1 y) + m_k2 z) + m_k3 in fp32, kept iff -h_k < q_k < h_k for k = 0..2 (box15: the 3x4
    world->box matrix by rows, then the half sizes)."""
    p = np.asarray(points)
    box15 = np.asarray(box15)
    assert p.dtype == np.float32 and box15.dtype == np.float32 and box15.shape == (15,)
    m, h = box15[:12].reshape(3, 4), box15[12:]
    x, y, z = p[:, 0:1], p[:, 1:2], p[:, 2:3]
    with np.errstate(invalid="ignore", over="ignore"):
        q = ((m[:, 0] * x + m[:, 1] * y) + m[:, 2] * z) + m[:, 3]
        assert q.dtype == np.float32
        return ((-h < q) & (q < h)).all(axis=1)


def random_box():
    from mtgs_amd.crop import OrientedBox
    return OrientedBox.from_params(POS, RPY, SIZE)


@functools.lru_cache(maxsize=None)
def random_points(n, seed=0):
    """uniform in +-EXTENT, float32 [n, 3] (read-only: shared between tests)"""
    p = ((np.random.default_rng(seed).random((n, 3)) * 2 - 1) * np.array(EXTENT)).astype(np.float32)
    p.setflags(write=False)
    return p
