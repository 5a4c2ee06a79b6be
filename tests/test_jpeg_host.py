"""JPEG encoding (mtgs_amd/jpeg.py, csrc/jpeg.hip, include/mtgs_jpeg.h) without a GPU: the NumPy encoder of tests/jpeg_refs.py
against Pillow's whole files (where this Pillow is installed) and against the recorded fixture (everywhere), the header as a group
of its own, the host-built file header, the capacity bound, and what the Python layer refuses before it touches a device."""
import ctypes as C
import inspect
import io
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from mtgs_amd import jpeg as J
from mtgs_amd import present as P
from tests import jpeg_refs as R

ROOT = Path(__file__).resolve().parents[1]
NAMES = ["mtgs_jpeg_encode", "mtgs_jpeg_header", "mtgs_jpeg_sizes"]
CASES = [(kind, h, w, q, s) for h, w in R.SIZES for q in R.QUALITIES for s in R.SUBSAMPLINGS for kind in R.KINDS]


def pillow():
    """PIL.Image of a Pillow built with libjpeg-turbo, or a skip that says what is missing"""
    Image = pytest.importorskip("PIL.Image", reason="Pillow is not installed")
    from PIL import features
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("this Pillow was not built with libjpeg-turbo")
    return Image


def pillow_bytes(Image, image, **kw):
    buf = io.BytesIO()
    Image.fromarray(image).save(buf, "JPEG", **kw)
    return buf.getvalue()


# ---- the reference against Pillow ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h, w", R.SIZES, ids=lambda v: str(v))
def test_the_reference_writes_pillows_whole_file(h, w):
    Image = pillow()
    for kind, hh, ww, q, s in CASES:
        if (hh, ww) == (h, w):
            want = pillow_bytes(Image, R.image_of(kind, h, w), quality=q, subsampling=s)
            assert R.encoded(kind, h, w, q, s) == want, (kind, h, w, q, s)


def test_a_default_save_is_quality_75_at_420():
    """the evaluation dump's Image.save(path.jpg) without arguments"""
    Image = pillow()
    for kind, (h, w) in (("noise", (17, 33)), ("ramp", (64, 50)), ("blocks", (31, 9))):
        assert pillow_bytes(Image, R.image_of(kind, h, w)) == R.encoded(kind, h, w, 75, "4:2:0")


def test_the_reference_writes_the_recorded_files():
    """unconditional: Pillow 12.2.0's bytes as tests/golden/make_jpeg_golden.py recorded them"""
    cases, (default_image, default_bytes) = R.golden()
    assert len(cases) == 7 * 3 * 3 * 2 and (ROOT / "tests" / "golden" / "jpeg_pillow.npz").stat().st_size < 200_000
    for (kind, h, w, q, s), (image, want) in cases.items():
        assert np.array_equal(image, R.image_of(kind, h, w))
        assert R.encoded(kind, h, w, q, s) == want, (kind, h, w, q, s)
    assert R.encode(default_image) == default_bytes


def test_the_block_kinds_reach_what_they_are_for():
    """the alternating 8 x 8 blocks give DC differences of the largest category; noise at quality 100 gives stuffed bytes"""
    blocks = R.component_blocks(R.image_of("blocks", 16, 16), 100, "4:4:4")[0][0]
    assert abs(int(blocks[0, 1, 0]) - int(blocks[0, 0, 0])) >= 1024          # category 11
    assert R.encoded("noise", 64, 50, 100, "4:4:4")[R.HEADER_BYTES:].count(b"\xff\x00") > 0


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_the_header_is_declared_bound_and_exported():
    """include/mtgs_jpeg.h is a group of its own (tests/test_abi.py checks every group against its header, its reviewed record
    tests/golden/abi_signatures_jpeg.txt and the library): its entry points and its constants."""
    from mtgs_amd import _lib
    assert sorted(_lib.GROUPS["mtgs_jpeg.h"]) == NAMES
    assert J.HEADER_BYTES == R.HEADER_BYTES == 623 and J.BLOCK_BITS == R.BLOCK_BITS == 1660


def test_the_host_checks_name_the_bad_argument(hip_lib):
    size = C.c_size_t(0)
    buf = (C.c_uint8 * 700)()
    meta = (C.c_int64 * 2)()
    raw = (C.c_uint8 * (4096 + 16))()
    aligned = C.c_void_p((C.addressof(raw) + 15) & ~15)            # the workspace must be 16-byte aligned
    valid = dict(image=buf, is_float=0, conversion=0, h=8, w=8, sy=24, sx=3, sc=1, sub=0, header=buf, data=buf, capacity=700, meta=meta,
                 ws=aligned, ws_bytes=4096, stream=None)
    encode = lambda **kw: hip_lib.mtgs_jpeg_encode(*(valid | kw).values())     # every call below fails a check: nothing is launched
    sizes, header = hip_lib.mtgs_jpeg_sizes, hip_lib.mtgs_jpeg_header
    for refused, message in ((lambda: sizes(0, 8, 0, C.byref(size), None), r"h and w outside \[1, 65535\]"),
                             (lambda: sizes(8, 65536, 0, C.byref(size), None), r"h and w outside"),
                             (lambda: sizes(8, 8, 2, C.byref(size), None), r"subsampling 2 is not implemented"),
                             (lambda: sizes(65535, 65535, 1, C.byref(size), None), r"too many blocks"),
                             (lambda: header(8, 8, 0, 0, buf, 700), r"quality outside \[1, 100\]"),
                             (lambda: header(8, 8, 101, 0, buf, 700), r"quality outside"),
                             (lambda: header(8, 8, 75, 0, None, 700), r"null pointer: header"),
                             (lambda: header(8, 8, 75, 0, buf, 622), r"header_capacity 622 < 623"),
                             (lambda: encode(image=None), r"null pointer: image"), (lambda: encode(conversion=2), r"conversion must be"),
                             (lambda: encode(sy=-1), r"negative stride"), (lambda: encode(header=None), r"null pointer: header"),
                             (lambda: encode(data=None), r"null pointer: data"), (lambda: encode(meta=None), r"meta must be"),
                             (lambda: encode(ws=None), r"null pointer: ws"), (lambda: encode(ws_bytes=16), r"workspace 16 < \d+ bytes"),
                             (lambda: encode(sub=2), r"subsampling 2"), (lambda: encode(h=0), r"h and w outside")):
        assert refused() != 0 and re.search(message, hip_lib.mtgs_rast_last_error().decode()), (message, hip_lib.mtgs_rast_last_error())


# ---- the file header and the capacity ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", R.SUBSAMPLINGS)
def test_the_host_built_header(hip_lib, s):
    for h, w in R.SIZES + [(512, 910), (1080, 1920), (65535, 3)]:
        for q in (1, 25, 49, 50, 51, 75, 100):
            data = J.header(h, w, q, s)
            assert data == R.header(h, w, q, s) and len(data) == J.HEADER_BYTES
    parts, at = R.segments(J.header(512, 910, 40, s))
    assert at == J.HEADER_BYTES and [m for m, _ in parts] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDA]
    assert parts[0][1] == b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"           # 1.01, no units, density 1:1, no thumbnail
    for index, base in enumerate((R.LUMA_Q, R.CHROMA_Q)):
        assert parts[1 + index][1][0] == index and list(parts[1 + index][1][1:]) == list(R.quant_table(base, 40)[R.ZIGZAG])
    sof = parts[3][1]
    assert sof[0] == 8 and int.from_bytes(sof[1:3], "big") == 512 and int.from_bytes(sof[3:5], "big") == 910
    assert list(sof[5:]) == [3, 1, 0x22 if s == "4:2:0" else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]
    assert [p[0] for _, p in parts[4:8]] == [0x00, 0x10, 0x01, 0x11] and parts[8][1] == bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    # the tables of quality 100 are all ones, those of quality 1 all 255
    assert set(R.segments(J.header(8, 8, 100, s))[0][1][1][1:]) == {1} and set(R.segments(J.header(8, 8, 1, s))[0][2][1][1:]) == {255}


def test_the_capacity_bounds_every_file(hip_lib):
    for kind, h, w, q, s in CASES:
        ws, capacity = J.sizes(h, w, s)
        assert capacity == R.capacity(h, w, s) >= len(R.encoded(kind, h, w, q, s)) and ws % 16 == 0
    # the longest codes: 11 bits for a DC category, 16 for an AC symbol; categories up to 11 and 10
    longest = lambda table: max(length for _, length in R.huffman_codes(table).values())
    assert max(longest(R.DC_LUMA), longest(R.DC_CHROMA)) + 11 == 22 and max(longest(R.AC_LUMA), longest(R.AC_CHROMA)) + 10 == 26
    assert J.BLOCK_BITS == 22 + 63 * 26
    assert J.sizes(512, 910, "4:2:0")[1] == 623 + 2 * -(-(32 * 57 * 6 * 1660) // 8) + 2


# ---- what the Python layer refuses ---------------------------------------------------------------------------------------------------
def test_unsupported_options_are_refused_by_name():
    rgb = torch.zeros((8, 8, 3), dtype=torch.uint8)
    for kw, name in ((dict(subsampling="4:2:2"), "subsampling='4:2:2'"), (dict(subsampling=1), "subsampling=1"), (dict(optimize=True), "optimize=True"),
                     (dict(progressive=True), "progressive=True"), (dict(quality=0), "quality=0"), (dict(quality=101), "quality=101"),
                     (dict(quality=75.0), "quality=75.0"), (dict(restart_interval=4), "restart_interval=4")):
        with pytest.raises(NotImplementedError, match=re.escape(name)):
            J.encode_jpeg(rgb, **kw)
    for channels in (1, 4):
        with pytest.raises(NotImplementedError, match=f"{channels} channel"):
            J.encode_jpeg(torch.zeros((8, 8, channels), dtype=torch.uint8))
    with pytest.raises(ValueError, match="conversion"):
        J.encode_jpeg(rgb, conversion="floor")
    with pytest.raises(TypeError, match="uint8 or float32"):
        J.encode_jpeg(rgb.to(torch.float16))
    with pytest.raises(ValueError, match=r"\[H, W, 3\]"):
        J.encode_jpeg(rgb[0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        J.encode_jpeg(rgb, optimize=False, progressive=False)             # the defaults of Pillow's save are accepted


def test_the_public_surface():
    import mtgs_amd
    assert mtgs_amd.encode_jpeg is J.encode_jpeg and mtgs_amd.JpegStream is J.JpegStream
    assert {"encode_jpeg", "JpegStream"} <= set(mtgs_amd.__all__)
    for fn in (P.viewer_frame, P.render_frame):
        assert inspect.signature(fn).parameters["jpeg_quality"].default is None
    s = inspect.signature(J.encode_jpeg).parameters
    assert (s["quality"].default, s["subsampling"].default, s["conversion"].default) == (75, "4:2:0", "truncate")
    assert s["conversion"].kind is s["out"].kind is s["capacity"].kind is inspect.Parameter.KEYWORD_ONLY


def test_to_u8_is_the_two_conversions_of_the_presented_frame():
    x = np.array([np.nan, -1.0, 0.0, 0.4 / 255, 0.6 / 255, 1.2 / 255, 100.6 / 255, 1.0, 2.0], dtype=np.float32)
    assert list(R.to_u8(x, "truncate")) == [0, 0, 0, 0, 0, 1, 100, 255, 255]
    assert list(R.to_u8(x, "round")) == [0, 0, 0, 0, 1, 1, 101, 255, 255]
