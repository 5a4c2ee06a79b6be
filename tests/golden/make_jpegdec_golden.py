"""Writes tests/golden/jpegdec_pillow.npz: JPEG files as Pillow (12.2.0, with libjpeg-turbo) saves them and the pixels the same
Pillow decodes from them, so that the pin on libjpeg's integer decode path travels to machines without this Pillow.

    names, jpg, jpg_bytes   the files' names, their bytes (Image.fromarray(img).save(..., "JPEG", **options)) end to end, their lengths
    pix, shapes             np.array(Image.open(the file)), uint8 [h, w, 3], end to end, and each (h, w)

    <name> = grid/<kind>/<h>x<w>/<quality>/<444|422|420>      tests.jpegdec_refs.image_of(kind, h, w): every size, kind, quality and subsampling
             narrow/<kind>/<h>x<w>/<75|100>/<...>             noise and ramp at the sizes whose chroma is one or two samples wide
             opt/<option>/<h>x<w>/75/<444|420>                noise with optimize=True, restart_marker_blocks=1 | 3, restart_marker_rows=1
             worst                                            tests.jpegdec_refs.worst_image(): quality 95, 4:2:0, optimize=True

Files saved with optimize=True go through a file: Pillow's save into a BytesIO fails on large noisy images ("Suspension not allowed
here").  Run from the repository root: python tests/golden/make_jpegdec_golden.py"""
import io
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
SUBS = {"444": 0, "422": 1, "420": 2}
OPTIONS = {"optimize": dict(optimize=True), "rmb1": dict(restart_marker_blocks=1), "rmb3": dict(restart_marker_blocks=3),
           "rmr1": dict(restart_marker_rows=1)}


def main():
    import PIL
    from PIL import Image, features
    from tests import jpegdec_refs as D
    assert features.check_feature("libjpeg_turbo"), "this Pillow was not built with libjpeg-turbo"
    files = {}

    def add(name, img, **kw):
        with tempfile.TemporaryDirectory() as tmp:
            path = Path(tmp) / "x.jpg"
            Image.fromarray(img).save(path, "JPEG", **kw)
            data = path.read_bytes()
        files[name] = (data, np.array(Image.open(io.BytesIO(data))))

    for h, w in D.SIZES:
        for kind in D.KINDS:
            for q in D.QUALITIES:
                for s, sub in SUBS.items():
                    add(f"grid/{kind}/{h}x{w}/{q}/{s}", D.image_of(kind, h, w), quality=q, subsampling=sub)
    for h, w in D.NARROW:                                      # chroma one or two samples wide: replicated, not interpolated
        for kind in ("noise", "ramp"):
            for q in (75, 100):
                for s, sub in SUBS.items():
                    add(f"narrow/{kind}/{h}x{w}/{q}/{s}", D.image_of(kind, h, w), quality=q, subsampling=sub)
    for option, kw in OPTIONS.items():
        for h, w, s in ((31, 50, "444"), (31, 50, "420"), (48, 65, "420")):
            add(f"opt/{option}/{h}x{w}/75/{s}", D.image_of("noise", h, w), quality=75, subsampling=SUBS[s], **kw)
    add("worst", D.worst_image(), quality=D.WORST["quality"], subsampling=D.WORST["subsampling"], optimize=D.WORST["optimize"])
    # one blob of files and one of pixels, files of the same quality and subsampling side by side: their headers then compress away
    names = sorted(files, key=lambda n: (n.split("/")[-2:], n))
    jpg, pix = [files[n][0] for n in names], [files[n][1] for n in names]
    out = Path(__file__).resolve().parent / "jpegdec_pillow.npz"
    np.savez_compressed(out, names=np.array(names), jpg=np.frombuffer(b"".join(jpg), dtype=np.uint8), jpg_bytes=np.array([len(d) for d in jpg]),
                        pix=np.concatenate([p.reshape(-1) for p in pix]), shapes=np.array([p.shape[:2] for p in pix]))
    print(f"Pillow {PIL.__version__}, libjpeg-turbo {features.version('jpg')}: {len(names)} files, {out.stat().st_size} bytes")

if __name__ == "__main__":
    main()
