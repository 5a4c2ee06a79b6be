"""The indexed PNG file of include/mtgs_png.h on the host: tests/png_refs.py (the NumPy restatement the kernels must equal) is pinned
to Pillow, zlib.decompress and zlib.adler32; mtgs_amd.png.parse_png reads what the restatement wrote and refuses everything else by
name; the two depth rules equal the reference's NumPy lines at their rounding edges.  No GPU."""
import io
import struct
import zlib

import numpy as np
import pytest
from PIL import Image

from mtgs_amd import png as P
from tests import png_refs as R


def cases():
    rng = np.random.default_rng(5)
    out = {}
    for shape in [(1, 1), (2, 3), (17, 65), (1, 1, 3), (5, 64, 3), (17, 63, 3)]:
        out[("noise",) + shape] = rng.integers(0, 256, shape, dtype=np.uint8)
        out[("labels",) + shape] = (rng.integers(0, 256, shape, dtype=np.uint8) >> 6) * 60
        out[("zero",) + shape] = np.zeros(shape, dtype=np.uint8)
    runs = np.concatenate([np.full(n, v, np.uint8) for v, n in enumerate([2, 3, 4, 258, 259, 260, 261, 517, 1, 1, 600], start=1)])
    out[("runs", 1, len(runs))] = runs[None]
    return out


CASES = cases()


def chunks_of(data):
    at, out = 8, []
    while at < len(data):
        n, name = struct.unpack(">I4s", data[at:at + 8])
        assert zlib.crc32(data[at + 4:at + 8 + n]) == struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0]
        out.append((name, data[at + 8:at + 8 + n]))
        at += 12 + n
    return out


@pytest.mark.parametrize("filter", [0, 1, 2])
@pytest.mark.parametrize("segment_bytes", [16, 64, 8192])
def test_the_restatement_writes_files_that_pillow_and_zlib_read(filter, segment_bytes):
    for key, image in CASES.items():
        for order in ("rgb", "bgr"):
            details = {}
            data = R.encode(image, filter, segment_bytes, order, details)
            want = image[..., ::-1] if order == "bgr" and image.ndim == 3 else image
            assert np.array_equal(np.array(Image.open(io.BytesIO(data))), want), key
            assert [c[0] for c in chunks_of(data)] == [b"IHDR", b"mtIX", b"IDAT", b"IEND"]
            stream = details["stream"].tobytes()
            assert zlib.decompress(details["payload"]) == stream, key
            assert details["payload"][-4:] == struct.pack(">I", zlib.adler32(stream))
            assert np.array_equal(R.decode(data, order), image), key                   # the indexed reader, segment by segment
            info = P.parse_png(data)
            assert (info.height, info.width, info.channels) == R.file_pixels(image).shape
            assert (info.filter, info.segment_bytes) == (("none", "sub", "up")[filter], segment_bytes)
            assert info.offsets == details["offsets"] and info.eob == details["eob"]
            assert info.lit_lengths == details["lit_lengths"] and info.has_distance == any(details["lit_lengths"][257:])
            assert data[info.payload_offset:info.payload_offset + info.payload_length] == details["payload"]


def test_the_token_rule_at_the_run_lengths():
    def lengths(n):
        return [v for kind, v in R.tokens_of(np.zeros(n, np.uint8)) if kind == "M"], sum(kind == "L" for kind, _ in R.tokens_of(np.zeros(n, np.uint8)))
    assert lengths(1) == ([], 1) and lengths(2) == ([], 2) and lengths(3) == ([], 3) and lengths(4) == ([3], 1)
    assert lengths(259) == ([258], 1) and lengths(260) == ([258], 2) and lengths(261) == ([258], 3) and lengths(262) == ([258, 3], 1)
    assert lengths(517) == ([258, 258], 1) and lengths(518) == ([258, 258], 2)
    for n in (1, 2, 5, 259, 262, 600):                   # every position decides alone, and the tokens cover the run
        matches, literals = lengths(n)
        assert sum(matches) + literals == n


def test_the_code_edges():
    details = {}
    R.encode(np.zeros((4, 40), np.uint8), 0, 64, "rgb", details)                       # two used symbols besides end-of-block
    assert sorted(s for s, n in enumerate(details["lit_lengths"]) if n) == [0, 256, 257 + R.length_symbol(40)[0]]
    R.encode((np.arange(600) * 37 % 256).astype(np.uint8).reshape(6, 100), 0, 64, "rgb", details)   # no run of 4: no distance code
    assert not any(details["lit_lengths"][257:])
    R.encode(np.arange(256, dtype=np.uint8).reshape(1, 256), 0, 8192, "rgb", details)
    assert all(details["lit_lengths"][:257])                                          # all 256 byte values and end-of-block
    image = R.fibonacci_image()
    data = R.encode(image, 0, 512, "rgb", details)
    assert all(kind == "L" for seg in details["tokens"] for kind, _ in seg)           # literals only: the histogram is the bytes'
    counts = np.bincount(details["stream"], minlength=256)
    assert image.size > 70000 and max(R.build_lengths(list(counts) + [1], 64)) == 22  # the limit is forced ...
    assert max(details["lit_lengths"]) == 15                                          # ... and kept
    assert np.array_equal(np.array(Image.open(io.BytesIO(data))), image) and np.array_equal(R.decode(data), image)
    assert P.parse_png(data).lit_lengths == details["lit_lengths"]


@pytest.mark.parametrize("limit, counts", [(15, [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584, 4181]),
                                           (7, [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89]), (7, [5, 0, 0, 9]), (7, [0, 3]), (15, [4] * 286)])
def test_the_builder_gives_a_complete_limited_code(limit, counts):
    lengths = R.build_lengths(counts, limit)
    used = [n for n in lengths if n]
    assert len(used) == sum(c > 0 for c in counts) and max(used) <= limit
    assert all((n > 0) == (c > 0) for n, c in zip(lengths, counts))
    if len(used) > 1:
        assert sum(1 << (limit - n) for n in used) == 1 << limit                      # Kraft: complete, as zlib demands
    by_count = sorted((-c, s) for s, c in enumerate(counts) if c)
    assert [lengths[s] for _, s in by_count] == sorted(used)                          # shorter codes to the larger counts


def with_chunks(chunks):
    return R.SIGNATURE + b"".join(R.chunk(name, body) for name, body in chunks)


def test_foreign_and_unsupported_files_are_refused_by_name():
    image = CASES[("noise", 5, 64, 3)]
    data = R.encode(image, 1, 64)
    ihdr, index, idat, iend = chunks_of(data)
    saved = io.BytesIO()
    Image.fromarray(image).save(saved, format="PNG")
    with pytest.raises(NotImplementedError, match="no mtIX chunk: not written by this encoder: decode on the host"):
        P.parse_png(saved.getvalue())
    with pytest.raises(NotImplementedError, match="no mtIX"):
        P.parse_png(with_chunks([ihdr, idat, iend]))

    def header(depth=8, colour=2, interlace=0):
        return (b"IHDR", struct.pack(">IIBBBBB", 64, 5, depth, colour, 0, 0, interlace))
    for bad, match in [(header(depth=16), "16-bit"), (header(colour=3), "palette"), (header(colour=6), "alpha"), (header(colour=4), "alpha"),
                       (header(interlace=1), "interlaced")]:
        with pytest.raises(NotImplementedError, match=match):
            P.parse_png(with_chunks([bad, index, idat, iend]))
    half = len(idat[1]) // 2
    with pytest.raises(NotImplementedError, match="several IDAT"):
        P.parse_png(with_chunks([ihdr, index, (b"IDAT", idat[1][:half]), (b"IDAT", idat[1][half:]), iend]))
    for filter, name in [(3, "Average"), (4, "Paeth")]:
        body = index[1][:4] + struct.pack("<I", filter) + index[1][8:]
        with pytest.raises(NotImplementedError, match=name):
            P.parse_png(with_chunks([ihdr, (b"mtIX", body), idat, iend]))
    for cut in (7, 20, 40, len(data) // 2, len(data) - 13, len(data) - 1):
        with pytest.raises(ValueError, match="cut short|not a PNG"):
            P.parse_png(data[:cut])
    with pytest.raises(ValueError, match="cut short"):
        P.parse_png(with_chunks([ihdr, index, (b"IDAT", idat[1][:6]), iend]))


def test_fill_crcs_completes_a_device_file():
    data = R.encode(CASES[("labels", 17, 65)], 2, 16)
    blank = bytearray(data)
    at = 8
    for name, body in chunks_of(data):
        if name in (b"mtIX", b"IDAT"):
            blank[at + 8 + len(body):at + 12 + len(body)] = bytes(4)                   # as the device leaves them
        at += 12 + len(body)
    assert bytes(blank) != data and P.fill_crcs(bytes(blank)) == data


# ---- the two depth rules -------------------------------------------------------------------------------------------------------------
def edge_depths():
    f = np.float32
    values = [0.0, 0.05, 0.1, np.nextafter(f(0.1), f(0)), np.nextafter(f(0.1), f(1)), 80.0, np.nextafter(f(80), f(100)),
              np.nextafter(f(80), f(0)), 2.56, np.nextafter(f(2.56), f(0)), np.nextafter(f(2.56), f(3)), 5.12, 25.6, 76.8,
              np.nextafter(f(76.8), f(0)), 79.999, 1.0, 0.999999, 12.345, -1.0, 81.0, 1e9, np.inf, -np.inf, np.nan, 2.555, 2.5599999]
    return np.array(values, dtype=np.float32)


def reference_depth_image(depth, raw_height, raw_width, x, y, w, h, max_range):
    """generate_dense_depth.py:239-244, its lines as they stand (NaN left out: its cast is no defined byte)"""
    depth = depth.copy()
    depth[depth > max_range] = 0
    depth[depth < 0.1] = 0
    depth_image = np.zeros((raw_height, raw_width, 3), dtype=np.uint8)
    depth_image[y:y+h, x:x+w, 0] = ((depth * 100) % 256).astype(np.uint8)
    depth_image[y:y+h, x:x+w, 1] = ((depth * 100) // 256).astype(np.uint8)
    return depth_image


def test_the_depth_rules_equal_the_references_lines_at_the_rounding_edges():
    values = edge_depths()
    t = values * np.float32(100)
    assert any(v == 256 for v in t) and any(255 < v < 256 for v in t) and np.float32(0.1) in values and np.float32(80) in values
    depth = np.resize(values, (4, 9))
    finite = np.where(np.isnan(depth), np.float32(0), depth)
    for max_range in (80, 60.5):
        got = R.depth_image(depth, (7, 12), (2, 1, 9, 4), max_range)
        assert np.array_equal(got, reference_depth_image(finite, 7, 12, 2, 1, 9, 4, max_range))
        assert got[:, :, 2].max() == 0 and got[0].max() == 0 and got[:, :2].max() == 0   # zero outside the window
    assert np.isnan(depth).any() and (R.depth_image(depth, (4, 9), (0, 0, 9, 4))[np.isnan(depth)] == 0).all()
    image = np.random.default_rng(3).integers(0, 256, (6, 5, 3), dtype=np.uint8)
    depth_img = image.astype(np.float32)                                              # custom_dataset.py:166-168
    want = (depth_img[:, :, 0] + (depth_img[:, :, 1] * 256.0)) * 0.01
    back = R.depth_from_image(image)
    assert back.dtype == np.float32 and back.shape == (6, 5, 1) and np.array_equal(back[:, :, 0].view(np.uint32), want.view(np.uint32))


def test_encode_depth_png_refuses_a_range_beyond_two_bytes():
    import torch
    with pytest.raises(NotImplementedError, match="max_range"):
        P.encode_depth_png(torch.zeros(2, 2), max_range=655.36)
    with pytest.raises(NotImplementedError, match="Paeth|paeth"):
        P.encode_png(torch.zeros(2, 2, dtype=torch.uint8), filter="paeth")
