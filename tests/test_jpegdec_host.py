"""JPEG decoding (mtgs_amd/jpegdec.py, csrc/jpegdec.hip, include/mtgs_jpegdec.h) without a GPU: the NumPy decoder of
tests/jpegdec_refs.py against Pillow's pixels in the recorded fixture (everywhere) and against live Pillow (where this Pillow is
installed), the host parser's fields and refusals, the synchronisation model's fixed point, and the header as a group of its own."""
import ctypes as C
import inspect
import io
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from mtgs_amd import jpegdec as J
from tests import jpeg_refs as R
from tests import jpegdec_refs as D

ROOT = Path(__file__).resolve().parents[1]
NAMES = ["mtgs_jpegdec_decode", "mtgs_jpegdec_sizes"]
SUBS = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}
GOLDEN = D.golden()


def pillow():
    Image = pytest.importorskip("PIL.Image", reason="Pillow is not installed")
    from PIL import features
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("this Pillow was not built with libjpeg-turbo")
    return Image


def save(Image, image, tmp_path=None, **kw):
    if tmp_path is not None:                    # optimize=True on large noisy images fails into a BytesIO: through a file
        Image.fromarray(image).save(tmp_path / "x.jpg", "JPEG", **kw)
        return (tmp_path / "x.jpg").read_bytes()
    buf = io.BytesIO()
    Image.fromarray(image).save(buf, "JPEG", **kw)
    return buf.getvalue()


# ---- the model against Pillow -------------------------------------------------------------------------------------------------------
def test_the_model_decodes_every_recorded_file_as_pillow_did():
    """unconditional, no tolerance, no case left out: Pillow 12.2.0's pixels as tests/golden/make_jpegdec_golden.py recorded them"""
    assert len(GOLDEN) == 433 and (ROOT / "tests" / "golden" / "jpegdec_pillow.npz").stat().st_size < 620_000
    for name, (data, want) in GOLDEN.items():
        got = D.decode(data)
        assert got.shape == want.shape and np.array_equal(got, want), name
    cells = {f"grid/{kind}/{h}x{w}/{q}/{s}" for kind in D.KINDS for h, w in D.SIZES for q in D.QUALITIES for s in ("444", "422", "420")}
    assert len(cells) == 360 and cells <= set(GOLDEN)                         # the whole grid of the device tests
    assert sum(name.startswith("narrow/") for name in GOLDEN) == 12 * len(D.NARROW)
    kinds = {name.split("/")[1] for name in GOLDEN if "/" in name}
    assert kinds >= {"noise", "ramp", "blocks", "constant", "checker", "optimize", "rmb1", "rmb3", "rmr1"} and "worst" in GOLDEN


@pytest.mark.parametrize("h, w", D.SIZES + D.NARROW + [(2, 2), (4, 5)], ids=lambda v: str(v))
def test_the_model_equals_live_pillow(h, w, tmp_path):
    """every kind, quality and subsampling, plain and at quality 75 with the options; the small sizes cover chroma one and two samples wide,
    which libjpeg replicates instead of interpolating"""
    Image = pillow()
    for kind in D.KINDS:
        image = D.image_of(kind, h, w)
        for q in D.QUALITIES:
            for s in SUBS.values():
                for kw in ({}, dict(optimize=True), dict(restart_marker_blocks=3), dict(restart_marker_rows=1))[:4 if q == 75 else 1]:
                    data = save(Image, image, tmp_path if kw.get("optimize") else None, quality=q, subsampling=s, **kw)
                    assert np.array_equal(D.decode(data), np.array(Image.open(io.BytesIO(data)))), (kind, q, s, kw)


def test_the_recorded_worst_case_is_the_file_of_the_issue(tmp_path):
    Image = pillow()
    data = save(Image, D.worst_image(), tmp_path, quality=95, subsampling=2, optimize=True)
    assert data == GOLDEN["worst"][0]


# ---- the parser ---------------------------------------------------------------------------------------------------------------------
def test_parse_jpeg_reads_pillows_files():
    for name, (data, pixels) in GOLDEN.items():
        info, f = J.parse_jpeg(data), D.read(data)
        assert (info.height, info.width, 3) == pixels.shape, name
        assert info.subsampling == f.subsampling and info.restart_interval == f.restart, name
        assert (info.scan_offset, info.scan_length) == (f.scan_offset, len(f.scan)), name
        assert data[info.scan_offset + info.scan_length:] == b"\xff\xd9", name
        assert np.array_equal(info.quant, np.stack([f.quant[t] for t in f.tq])) and info.quant.shape == (3, 64)
        for (tc, th), (bits, vals) in f.huff.items():
            assert info.huffman[("dc", "ac")[tc] + str(th)] == (tuple(bits), tuple(vals)), name
        assert [tuple(s) for s in info.selectors] == [tuple(s) for s in f.selectors] == [(0, 0), (1, 1), (1, 1)]
        assert info.tables.dtype == np.int32 and info.tables.shape == (J.TABLE_WORDS,)
    subs = {J.parse_jpeg(GOLDEN[f"grid/ramp/17x17/75/{s}"][0]).subsampling for s in ("444", "422", "420")}
    assert subs == {"4:4:4", "4:2:2", "4:2:0"}
    assert J.parse_jpeg(GOLDEN["opt/rmb3/31x50/75/420"][0]).restart_interval == 3
    assert J.parse_jpeg(GOLDEN["opt/rmr1/31x50/75/420"][0]).restart_interval == 4          # a row of MCUs of 16 pixels
    assert J.parse_jpeg(GOLDEN["opt/optimize/31x50/75/420"][0]).huffman["ac0"] != (tuple(R.AC_LUMA[0]), tuple(R.AC_LUMA[1]))


def test_parse_jpeg_reads_the_encoders_own_header():
    for s in ("4:2:0", "4:4:4"):
        image = R.image_of("noise", 17, 33)
        data = R.encode(image, 40, s)
        info = J.parse_jpeg(data)
        assert (info.height, info.width, info.subsampling, info.restart_interval) == (17, 33, s, 0)
        assert info.scan_offset == R.HEADER_BYTES and info.scan_length == len(data) - R.HEADER_BYTES - 2
        assert np.array_equal(info.quant[0], R.quant_table(R.LUMA_Q, 40)) and np.array_equal(info.quant[2], R.quant_table(R.CHROMA_Q, 40))
        for name, table in (("dc0", R.DC_LUMA), ("ac0", R.AC_LUMA), ("dc1", R.DC_CHROMA), ("ac1", R.AC_CHROMA)):
            assert info.huffman[name] == (tuple(table[0]), tuple(table[1]))


def test_the_packed_tables_decode_every_code():
    """the words the kernels read, by the kernels' own rule: the fast table on 10 bits, then maxcode / valoff / huffval"""
    K = J._K
    for name in ("grid/noise/48x65/75/420", "opt/optimize/48x65/75/420", "worst"):
        info = J.parse_jpeg(GOLDEN[name][0])
        t = info.tables
        for slot, key in enumerate(("dc0", "dc1", "ac0", "ac1")):
            for symbol, (code, length) in R.huffman_codes(info.huffman[key]).items():
                for tail in (0, (1 << (16 - length)) - 1):
                    window = (code << (16 - length)) | tail
                    fast = int(t[K["MTGS_JPEGDEC_FAST_AT"] + slot * 1024 + (window >> 6)])
                    if length <= J.FAST_BITS:
                        assert fast == (length << 8) | symbol
                        continue
                    assert fast == 0
                    found = next(l for l in range(11, 17) if (window >> (16 - l)) <= t[K["MTGS_JPEGDEC_MAXCODE_AT"] + slot * 18 + l])
                    at = ((window >> (16 - found)) + int(t[K["MTGS_JPEGDEC_VALOFF_AT"] + slot * 18 + found])) & 255
                    assert found == length and t[K["MTGS_JPEGDEC_HUFFVAL_AT"] + slot * 256 + at] == symbol
            assert t[K["MTGS_JPEGDEC_FAST_AT"] + slot * 1024 + 1023] == 0          # all ones is no code
        assert list(t[K["MTGS_JPEGDEC_SLOT_AT"]:][:6]) == [0, 2, 1, 3, 1, 3]


def test_progressive_and_grayscale_files_are_refused():
    Image = pillow()
    rgb = D.image_of("noise", 17, 17)
    for data, error, message in (
            (save(Image, rgb, progressive=True), NotImplementedError, r"progressive DCT \(SOF2\)"),
            (save(Image, rgb[..., 0]), NotImplementedError, r"grayscale"),
    ):
        with pytest.raises(error, match=message):
            J.parse_jpeg(data)


def test_cmyk_files_are_refused():
    Image = pillow()
    buf = io.BytesIO()
    Image.fromarray(D.image_of("noise", 17, 17)).convert("CMYK").save(buf, "JPEG")
    with pytest.raises(NotImplementedError, match="four components"):
        J.parse_jpeg(buf.getvalue())


def test_damaged_and_foreign_headers_are_refused_by_name():
    data = GOLDEN["grid/noise/31x50/75/420"][0]
    with pytest.raises(ValueError, match="cut short"):
        J.parse_jpeg(data[:len(data) // 2])                                    # inside the scan: no EOI
    with pytest.raises(ValueError, match="cut short"):
        J.parse_jpeg(data[:300])                                               # inside a segment
    with pytest.raises(ValueError, match="no SOI"):
        J.parse_jpeg(b"\x89PNG" + data)
    at = data.index(b"\xff\xdb")
    patched = bytearray(data[:at + 2] + (2 + 129).to_bytes(2, "big") + b"\x10" + bytes(128) + data[at + 4 + 65:])
    with pytest.raises(NotImplementedError, match="16-bit quantisation table"):
        J.parse_jpeg(bytes(patched))
    sof = data.index(b"\xff\xc0")
    for byte, value, message in ((sof + 1, 0xC1, r"extended sequential DCT \(SOF1\)"), (sof + 1, 0xC9, "arithmetic coding"),
                                 (sof + 4, 12, "12-bit"), (sof + 11, 0x12, "sampling factors 1x2, 1x1, 1x1"),
                                 (sof + 14, 0x21, "sampling factors 2x2, 2x1, 1x1")):
        changed = bytearray(data)
        changed[byte] = value
        with pytest.raises(NotImplementedError, match=message):
            J.parse_jpeg(bytes(changed))
    two_scans = data[:-2] + data[data.index(b"\xff\xda"):]
    with pytest.raises(NotImplementedError, match="more than one scan"):
        J.parse_jpeg(two_scans)
    dnl = data[:-2] + b"\xff\xdc\x00\x04\x00\x1f\xff\xd9"
    with pytest.raises(NotImplementedError, match="DNL"):
        J.parse_jpeg(dnl)
    for marker, name in ((0xC8, "JPG extension"), (0xF0, "0xf0"), (0xFD, "0xfd"), (0xDE, "hierarchical"), (0xDF, "EXP")):
        foreign = data[:2] + bytes([0xFF, marker, 0, 4, 0, 0]) + data[2:]
        with pytest.raises(NotImplementedError, match=name):
            J.parse_jpeg(foreign)
    adobe = data[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00" + data[data.index(b"\xff\xdb"):]     # no JFIF, transform 0
    with pytest.raises(NotImplementedError, match="Adobe transform 0"):
        J.parse_jpeg(adobe)


def segments_of(data):
    """[(marker, the whole segment's bytes)] up to and including SOS, and the rest"""
    at, out = 2, []
    while True:
        marker, length = data[at + 1], int.from_bytes(data[at + 2:at + 4], "big")
        out.append((marker, data[at:at + 2 + length]))
        at += 2 + length
        if marker == 0xDA:
            return out, data[at:]


def test_merged_tables_comments_and_fill_bytes_are_accepted():
    data, pixels = GOLDEN["grid/noise/31x50/75/420"]
    segments, rest = segments_of(data)
    dht = [s for m, s in segments if m == 0xC4]
    dqt = [s for m, s in segments if m == 0xDB]
    assert len(dht) == 4 and len(dqt) == 2
    one_dht = b"\xff\xc4" + (2 + sum(len(s) - 4 for s in dht)).to_bytes(2, "big") + b"".join(s[4:] for s in dht)
    one_dqt = b"\xff\xdb" + (2 + sum(len(s) - 4 for s in dqt)).to_bytes(2, "big") + b"".join(s[4:] for s in dqt)
    segment = lambda marker, payload: bytes([0xFF, marker]) + (2 + len(payload)).to_bytes(2, "big") + payload
    com, app1 = segment(0xFE, b"hello \xff\xd9 you"), segment(0xE1, b"http://ns.adobe.com/xap/1.0/\x00<x/>")
    out, merged = b"\xff\xd8", False
    for marker, s in segments:
        if marker in (0xC4, 0xDB):
            if marker == 0xC4 and not merged:
                out, merged = out + com + b"\xff\xff\xff" + one_dht, True      # fill bytes in front of the marker
            elif marker == 0xDB and one_dqt:
                out, one_dqt = out + one_dqt + app1, b""
        else:
            out += s
    out += rest
    assert out != data
    info, plain = J.parse_jpeg(out), J.parse_jpeg(data)
    assert np.array_equal(info.tables, plain.tables) and info.huffman == plain.huffman and info.scan_length == plain.scan_length
    assert out[info.scan_offset:info.scan_offset + info.scan_length] == data[plain.scan_offset:plain.scan_offset + plain.scan_length]
    assert np.array_equal(D.decode(out), pixels)
    try:                                                          # and Pillow reads the rearranged file alike, where it is installed
        from PIL import Image
    except ImportError:
        return
    assert np.array_equal(np.array(Image.open(io.BytesIO(out))), pixels)


# ---- the fixed point ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, bits", [("worst", 256), ("grid/noise/48x65/75/444", 128), ("opt/rmb3/48x65/75/420", 64),
                                        ("grid/ramp/31x50/75/422", 32)])
def test_converged_entries_are_the_serial_decoders_states(name, bits):
    f = D.read(GOLDEN[name][0])
    entries, serial = D.entries(f, bits), D.serial_states(f, bits)
    assert len(entries) == len(serial) == len(D.subsequences(f, bits)) > 8 and entries == serial
    guesses = [(b, 0, 0) for b, _, _ in D.subsequences(f, bits)]
    assert entries != guesses                                     # and the guesses were not right to begin with


def test_the_suite_holds_the_serial_worst_case():
    """the 48 x 65 noise file of quality 95 at 4:2:0 with optimised tables never synchronises: one step per subsequence"""
    f = D.read(GOLDEN["worst"][0])
    for bits in (256, 1024):
        assert D.steps(f, bits) == len(D.subsequences(f, bits)) == {256: 104, 1024: 26}[bits]
    easy = D.read(GOLDEN["grid/ramp/48x65/75/444"][0])
    assert D.steps(easy, 256) < len(D.subsequences(easy, 256)) // 2           # while an ordinary file synchronises at once


# ---- the C ABI and the Python layer --------------------------------------------------------------------------------------------------
def test_the_header_is_declared_bound_and_exported():
    from mtgs_amd import _lib
    assert sorted(_lib.GROUPS["mtgs_jpegdec.h"]) == NAMES
    assert (J.TABLE_WORDS, J.FAST_BITS, J.RUN, J.STATUS_WORDS) == (5464, 10, 256, 4)
    assert J.SUBSEQUENCE_BITS in (512, 1024, 2048, 4096)


def test_the_host_checks_name_the_bad_argument(hip_lib):
    size = C.c_size_t(0)
    buf = (C.c_uint8 * 4096)()
    raw = (C.c_uint8 * (1 << 16))()
    aligned = C.c_void_p((C.addressof(raw) + 15) & ~15)
    valid = dict(scan=buf, scan_bytes=100, tables=buf, h=8, w=8, sub=0, ri=0, bits=0, out=buf, is_float=0, sy=24, sx=3, sc=1, status=buf,
                 ws=aligned, ws_bytes=16, stream=None)
    decode = lambda **kw: hip_lib.mtgs_jpegdec_decode(*(valid | kw).values())     # every call below fails a check: nothing is launched
    sizes = hip_lib.mtgs_jpegdec_sizes
    for refused, message in ((lambda: sizes(0, 8, 0, 0, 100, 0, C.byref(size)), r"h and w outside \[1, 65535\]"),
                             (lambda: sizes(8, 8, 3, 0, 100, 0, C.byref(size)), r"subsampling 3 is not implemented"),
                             (lambda: sizes(8, 8, 0, -1, 100, 0, C.byref(size)), r"restart_interval outside"),
                             (lambda: sizes(8, 8, 0, 0, 0, 0, C.byref(size)), r"scan_bytes outside"),
                             (lambda: sizes(8, 8, 0, 0, 1 << 27, 0, C.byref(size)), r"scan_bytes outside"),
                             (lambda: sizes(8, 8, 0, 0, 100, 48, C.byref(size)), r"subsequence_bits must be a multiple of 32"),
                             (lambda: sizes(8, 8, 0, 0, 100, 0, None), r"null pointer: ws_bytes"),
                             (lambda: decode(scan=None), r"null pointer: scan"), (lambda: decode(tables=None), r"tables must be"),
                             (lambda: decode(out=None), r"null pointer: out"), (lambda: decode(sy=-1), r"negative stride"),
                             (lambda: decode(status=None), r"status must be"), (lambda: decode(ws=None), r"null pointer: ws"),
                             (lambda: decode(), r"workspace 16 < \d+ bytes"), (lambda: decode(bits=16), r"subsequence_bits"),
                             (lambda: decode(h=0), r"h and w outside")):
        assert refused() != 0 and re.search(message, hip_lib.mtgs_rast_last_error().decode()), (message, hip_lib.mtgs_rast_last_error())
    assert sizes(1080, 1920, 2, 0, 400_000, 1024, C.byref(size)) == 0 and size.value % 16 == 0
    small = size.value
    assert sizes(1080, 1920, 2, 0, 400_000, 512, C.byref(size)) == 0 and size.value > small       # more subsequences


def test_the_python_layer_checks_before_it_touches_a_device():
    data = GOLDEN["grid/ramp/17x17/75/420"][0]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        J.decode_jpeg(J.upload_jpeg(data, device="cpu"))
    with pytest.raises(TypeError, match="bytes, a host uint8 tensor or array, or a DeviceJpeg"):
        J.decode_jpeg("frame.jpg")
    with pytest.raises(TypeError, match="uint8"):
        J.decode_jpeg(torch.zeros(8, dtype=torch.int32))
    with pytest.raises(ValueError, match="subsequence_bits"):
        J.decode_jpeg(data, subsequence_bits=100)
    with pytest.raises(ValueError, match="cut short"):
        J.decode_jpeg(np.frombuffer(data[:200], dtype=np.uint8))
    host = J.upload_jpeg(torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()), device="cpu")
    assert host.scan.numel() == host.info.scan_length and host.tables.dtype == torch.int32
    assert bytes(host.scan.numpy()) == data[host.info.scan_offset:-2]


def test_the_public_surface(hip_lib):
    import mtgs_amd
    assert mtgs_amd.decode_jpeg is J.decode_jpeg and mtgs_amd.parse_jpeg is J.parse_jpeg and mtgs_amd.upload_jpeg is J.upload_jpeg
    assert {"decode_jpeg", "parse_jpeg", "upload_jpeg"} <= set(mtgs_amd.__all__)
    s = inspect.signature(J.decode_jpeg).parameters
    assert [s[k].default for k in ("image_float", "out", "workspace", "subsequence_bits", "return_status")] == [False, None, None, None, False]
    assert all(s[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("image_float", "out", "workspace", "subsequence_bits", "return_status"))
    info = J.parse_jpeg(GOLDEN["grid/noise/48x65/100/444"][0])
    assert J.sizes(info) % 16 == 0 and J.sizes(info, 256) > J.sizes(info, 4096)
