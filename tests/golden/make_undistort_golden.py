"""Writes tests/golden/undistort_frame_64x48.jpg: a 64 x 48 (width x height) baseline JPEG, 4:2:0, quality 90, of a smooth ramp with
a little noise, written by the project's own encoder model (tests/jpeg_refs.py).  The chain test of tests/test_gpu_undistort.py
decodes, undistorts and resizes it.  Run from the repository root: python -m tests.golden.make_undistort_golden"""
from pathlib import Path

import numpy as np

from tests import jpeg_refs

H, W, SEED = 48, 64, 6448


def image():
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = np.stack([4 * xx, 5 * yy, 2 * (xx + yy)], axis=-1)
    return np.clip(ramp + np.random.default_rng(SEED).integers(-12, 13, (H, W, 3)), 0, 255).astype(np.uint8)


if __name__ == "__main__":
    out = Path(__file__).resolve().parent / "undistort_frame_64x48.jpg"
    out.write_bytes(jpeg_refs.encode(image(), 90, "4:2:0"))
    print(out, out.stat().st_size, "bytes")
