"""Writes tests/golden/brightness_ref.npz: the inputs of one eight-camera scene with what the reference's OWN
adjust_brightness_single_frame (nuplan_scripts/utils/nuplan_utils_custom.py) computes for them, so that the pin on the estimate
travels without the reference.  Inputs and recorded results only; no line of the reference is copied: at generation time the
function is cut out of its file with `ast` (as make_lidar_golden.py cuts its functions) and called with points= so that no file is
read.

cv2 is not installed, so the function is given a stand-in `cv2` in its namespace whose cvtColor returns V = max over the last axis
in channel 2 and zeros for H and S, and records every array it is handed.  The function reads only `[..., 2]` of the result, and V
of an 8-bit RGB -> HSV conversion IS max(R, G, B) by the definition of HSV, so the stand-in is faithful for everything the function
computes.

    points float32 [N, 3]   lidar2imgs float64 [8, 4, 4]   images uint8 [8, 37, 120, 3] (BGR)   cameras: the reference's names
    factors float64 [8]: info['cams'][name]['v_adjust'] in camera order
    used_count, used_s1, used_s2 int64 [8]: per pair, the number of pixels the stand-in was handed and the sums of their V for cam1
        and cam2 -- the overlap's where it had at least 10 points, the two strips' otherwise
    pairs int32 [8, 3]: the reference's `matches` and `overlapped_regions` as (cam1, cam2, side)

The maker asserts that tests/brightness_refs.py reproduces the reference on these inputs EXACTLY: the counts, the sums and the bits
of the eight factors; that some pairs overlap and at least two fall back to the strips.  A seed that puts a sample within rounding of
an integer times 1/255, so that the truncation to a byte flips between the reference's grid_sample and the restatement, fails the
assertion: choose another.

Run from the repository root: python tests/golden/make_brightness_golden.py /path/to/MTGS [--seed S]"""
import argparse
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
H, W, N, F = 37, 120, 6000, 86.0
CAMERAS = ("CAM_F0", "CAM_L0", "CAM_R0", "CAM_L1", "CAM_R1", "CAM_L2", "CAM_R2", "CAM_B0")
# half a field of view is 35 degrees: neighbours 55 degrees apart share 15; L1 -> L2 and R1 -> R2 are 75 apart and share nothing
YAWS = (0.0, 55.0, -55.0, 110.0, -110.0, 185.0, -185.0, 180.0)


class StandInCv2:
    COLOR_RGB2HSV = "RGB2HSV"

    def __init__(self):
        self.seen = []

    def cvtColor(self, a, code):
        assert code == self.COLOR_RGB2HSV and a.dtype == np.uint8 and a.shape[-1] == 3
        self.seen.append(a.copy())
        out = np.zeros_like(a)
        out[..., 2] = a.max(axis=-1)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference", type=Path, help="a checkout of OpenDriveLab/MTGS")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    from make_lidar_golden import cut
    from tests import brightness_refs as B
    from tests import lidar_refs as R

    cv2 = StandInCv2()
    ref = cut(a.reference / "nuplan_scripts" / "utils" / "nuplan_utils_custom.py", "adjust_brightness_single_frame",
              {"np": np, "torch": torch, "cv2": cv2, "os": None, "load_lidar": None, "NUPLAN_SENSOR_ROOT": None})
    rng = np.random.default_rng(a.seed)
    pts = R.sweep(rng, N)
    mats = np.stack([R.camera(y, F, rng.uniform(-0.3, 0.3, 3), W, H)[0] for y in YAWS])
    # smooth images of different brightness per camera, so that the factors differ, with noise on top
    gain = rng.uniform(0.5, 1.0, len(YAWS))
    ramp = np.linspace(0.3, 1.0, W)[None, :, None] * np.linspace(0.6, 1.0, H)[:, None, None]
    images = np.stack([np.clip(255 * g * ramp * rng.uniform(0.7, 1.0, (H, W, 3)), 0, 255).astype(np.uint8) for g in gain])
    info = {"cams": {name: {} for name in CAMERAS}}
    ref(info, mats.copy(), [im.copy() for im in images], pts.copy())
    factors = np.array([info["cams"][name]["v_adjust"] for name in CAMERAS], dtype=np.float64)
    P = len(B.NUPLAN_PAIRS)
    assert len(cv2.seen) == 2 * P
    used = np.array([[cv2.seen[2 * p].shape[1], cv2.seen[2 * p].max(axis=-1).astype(np.int64).sum(),
                      cv2.seen[2 * p + 1].max(axis=-1).astype(np.int64).sum()] for p in range(P)], dtype=np.int64)
    assert all(cv2.seen[2 * p].shape == cv2.seen[2 * p + 1].shape for p in range(P))

    mine, stats = B.estimate_factors(pts, mats, images)
    overlap = stats[:, 0] >= 10
    want = np.where(overlap[:, None], stats[:, :3], np.concatenate([np.full((P, 1), H * min(100, W)), stats[:, 3:]], axis=1))
    assert np.array_equal(want, used), f"counts or sums differ: another seed\n{want}\n{used}"
    assert np.array_equal(mine.view(np.int64), factors.view(np.int64)), f"factors differ\n{mine}\n{factors}"
    assert overlap.sum() >= 3 and (~overlap).sum() >= 2, stats[:, 0]
    path = Path(__file__).resolve().parent / "brightness_ref.npz"
    np.savez_compressed(path, points=pts, lidar2imgs=mats, images=images, cameras=np.array(CAMERAS), factors=factors,
                        used_count=used[:, 0], used_s1=used[:, 1], used_s2=used[:, 2], pairs=np.array(B.NUPLAN_PAIRS, dtype=np.int32))
    print(f"overlap counts {stats[:, 0].tolist()}, {int((~overlap).sum())} pairs on the strips, factors {np.round(factors, 4).tolist()}; "
          f"{path.stat().st_size} bytes")


if __name__ == "__main__":
    main()
