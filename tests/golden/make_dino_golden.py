"""Writes tests/golden/dino_preprocess.npz: what Pillow itself makes of seeded 8-bit inputs, for the preprocessing of the DINOv2
similarity metric (include/mtgs_dino.h, sections 1-2).  Needs PIL and NumPy only; run once, where Pillow is installed:

    python tests/golden/make_dino_golden.py

Per case `HxW_S`: in_* the uint8 image [H, W, 3], out_* Pillow's BILINEAR resize (short side to S, the long one int(S * long / short))
and centre crop [S, S, 3], mask_in_* a 0 / 1 mask [H, W], mask_out_* Pillow's NEAREST resize of the 0 / 255 byte image and the same
crop.  The 128 x 228 -> 518 case keeps rows STRIP[0] .. STRIP[1] - 1 of the cropped outputs only.  The larger inputs draw from 16 random
levels so that the file stays small.
"""
from pathlib import Path

import numpy as np
import PIL
from PIL import Image

CASES = [(67, 131, 56, False), (40, 30, 56, False), (200, 333, 56, True), (56, 90, 56, False), (2000, 61, 56, True), (128, 228, 518, True)]
STRIP = (200, 264)


def resized_size(H, W, S):
    short, long_ = (H, W) if H <= W else (W, H)
    if short == S:
        return H, W
    new_long = int(S * long_ / short)
    return (S, new_long) if H <= W else (new_long, S)


def crop(x, S):
    top, left = int(round((x.shape[0] - S) / 2.0)), int(round((x.shape[1] - S) / 2.0))
    return x[top:top + S, left:left + S]


def main():
    out = {"pillow_version": np.array(PIL.__version__)}
    for n, (H, W, S, palette) in enumerate(CASES):
        rng = np.random.RandomState(100 + n)
        img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
        if palette:
            img = rng.randint(0, 256, 16).astype(np.uint8)[img >> 4]
        mask = (rng.rand(H, W) > 0.3).astype(np.uint8)
        oh, ow = resized_size(H, W, S)
        res = np.asarray(Image.fromarray(img, "RGB").resize((ow, oh), Image.BILINEAR)) if (oh, ow) != (H, W) else img
        mres = np.asarray(Image.fromarray(mask * 255, "L").resize((ow, oh), Image.NEAREST)) if (oh, ow) != (H, W) else mask * 255
        res, mres = crop(res, S), crop(mres, S)
        if S == 518:
            res, mres = res[STRIP[0]:STRIP[1]], mres[STRIP[0]:STRIP[1]]
        key = f"{H}x{W}_{S}"
        out.update({f"in_{key}": img, f"out_{key}": res, f"mask_in_{key}": mask, f"mask_out_{key}": (mres != 0).astype(np.uint8)})
    path = Path(__file__).resolve().parent / "dino_preprocess.npz"
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
