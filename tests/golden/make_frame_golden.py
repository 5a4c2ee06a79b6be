"""Writes tests/golden/frame_ref.npz: Pillow's OWN outputs for the shapes of tests.frame_refs.GOLDEN_SHAPES, so that the pin on
Image.resize travels to a machine without Pillow.  Recorded results only: the inputs are tests.frame_refs.frame_inputs(seed, h, w),
drawn again by the tests from the seed stored in the file (with a crc32 of the planes, which tells a changed random stream from a
changed resampler).

    seed int64   pillow str (PIL.__version__)
    <h>x<w>_<oh>x<ow>/crc          uint32   crc32 of the input planes
    <h>x<w>_<oh>x<ow>/image        uint8   [oh, ow, 3]   Image.fromarray(image).resize((ow, oh), BILINEAR)            mode RGB
    <h>x<w>_<oh>x<ow>/depth        float32 [oh, ow]      ... of the depth, BILINEAR                                  mode F
    <h>x<w>_<oh>x<ow>/semantic_map uint8   [oh, ow]      ... NEAREST                                                 mode L
    <h>x<w>_<oh>x<ow>/instance_map int32   [oh, ow]      ... NEAREST                                                 mode I
    <h>x<w>_<oh>x<ow>/mask         bool    [oh, ow]      ... NEAREST                                                 mode 1

The maker asserts that tests/frame_refs.py reproduces every recorded plane bit for bit.

Run from the repository root: python tests/golden/make_frame_golden.py [--seed S]"""
import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))


def pillow_resize(a, oh, ow, resample):
    """what CustomInputDataset._resize_numpy_image does with one [H, W] or [H, W, 3] array"""
    from PIL import Image
    got = np.array(Image.fromarray(a).resize((ow, oh), resample=resample), dtype=a.dtype)
    return got.view(np.uint8) != 0 if a.dtype == np.bool_ else got      # a mode "1" image comes back with True as the byte 255


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    import PIL
    from PIL import Image
    from tests import frame_refs as R

    out = {"seed": np.int64(a.seed), "pillow": np.str_(PIL.__version__)}
    for (h, w), (oh, ow) in R.GOLDEN_SHAPES:
        planes = R.frame_inputs(a.seed, h, w)
        name = f"{h}x{w}_{oh}x{ow}"
        out[f"{name}/crc"] = np.uint32(R.checksum(planes))
        mine = R.resize_frame(planes, oh, ow)
        for key, x in planes.items():
            got = pillow_resize(x, oh, ow, Image.Resampling.BILINEAR if key in ("image", "depth") else Image.Resampling.NEAREST)
            assert got.dtype == x.dtype and got.tobytes() == mine[key].tobytes(), (name, key)
            out[f"{name}/{key}"] = got
    path = Path(__file__).resolve().parent / "frame_ref.npz"
    np.savez_compressed(path, **out)
    print(f"Pillow {PIL.__version__}, seed {a.seed}: {len(R.GOLDEN_SHAPES)} shapes, {path.stat().st_size} bytes")


if __name__ == "__main__":
    main()
