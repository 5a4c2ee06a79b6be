"""Writes tests/golden/jpeg_pillow.npz: a subset of the cases of tests/test_jpeg_host.py with the bytes Pillow (12.2.0, with
libjpeg-turbo) saves for them, so that the pin on libjpeg's integer path travels to machines without this Pillow.

    img/<kind>/<h>x<w>                      uint8 [h, w, 3], tests.jpeg_refs.image_of(kind, h, w)
    jpg/<kind>/<h>x<w>/<quality>/<420|444>  the bytes of Image.fromarray(img).save(buf, "JPEG", quality=, subsampling=)
    default/<kind>/<h>x<w>                  the bytes of Image.fromarray(img).save(buf, "JPEG"): quality 75, 4:2:0

Run from the repository root: python tests/golden/make_jpeg_golden.py"""
import io
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
SIZES = [(1, 1), (7, 5), (16, 16), (17, 33), (31, 9), (9, 31), (40, 48)]
KINDS = ("noise", "ramp", "blocks")
QUALITIES = (1, 75, 100)


def main():
    import PIL
    from PIL import Image, features
    from tests import jpeg_refs as R
    assert features.check_feature("libjpeg_turbo"), "this Pillow was not built with libjpeg-turbo"
    arrays = {}

    def save(img, **kw):
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, "JPEG", **kw)
        return np.frombuffer(buf.getvalue(), dtype=np.uint8)

    for h, w in SIZES:
        for kind in KINDS:
            img = arrays[f"img/{kind}/{h}x{w}"] = R.image_of(kind, h, w)
            for q in QUALITIES:
                for s in R.SUBSAMPLINGS:
                    arrays[f"jpg/{kind}/{h}x{w}/{q}/{s.replace(':', '')}"] = save(img, quality=q, subsampling=s)
    arrays["default/noise/17x33"] = save(arrays["img/noise/17x33"])
    out = Path(__file__).resolve().parent / "jpeg_pillow.npz"
    np.savez_compressed(out, **arrays)
    print(f"Pillow {PIL.__version__}, libjpeg-turbo {features.version('jpg')}: {len(arrays)} arrays, {out.stat().st_size} bytes")


if __name__ == "__main__":
    main()
