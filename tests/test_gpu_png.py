"""mtgs_amd.png on the device (csrc/png.hip): every file is compared BYTE FOR BYTE with tests/png_refs.py, the restatement that
tests/test_png_host.py pins to Pillow and zlib; Pillow and zlib read it back; decode_png returns the input and decode_depth_png the
reference's NumPy rule bit for bit -- at the smallest shapes that can still go wrong."""
import io
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

import mtgs_amd
from mtgs_amd import png as P
from tests import png_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILTERS = {"none": 0, "sub": 1, "up": 2}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_file(got: bytes, want: bytes, what=""):
    if got != want:
        at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError(f"{what}: {len(got)} bytes against {len(want)}, first difference at byte {at}: "
                             f"{got[max(at - 4, 0):at + 8].hex()} against {want[max(at - 4, 0):at + 8].hex()}")


def round_trip(image, filter="sub", segment_bytes=16, order="rgb", what=""):
    """the device file of `image` against the restatement's, Pillow, zlib, and the device reader; returns the file"""
    what = what or f"{image.shape} {filter} {segment_bytes} {order}"
    data = mtgs_amd.encode_png(dev(image), filter, segment_bytes, order)
    same_file(data, R.encode(image, FILTERS[filter], segment_bytes, order), what)
    in_file_order = image[..., ::-1] if order == "bgr" and image.ndim == 3 else image
    assert np.array_equal(np.array(Image.open(io.BytesIO(data))), in_file_order), what
    info = P.parse_png(data)
    stream = R.row_stream(R.file_pixels(image, order), FILTERS[filter]).tobytes()
    assert zlib.decompress(data[info.payload_offset:info.payload_offset + info.payload_length]) == stream, what
    pixels, status = mtgs_amd.decode_png(data, order, return_status=True)
    assert status.tolist() == [0, len(info.offsets), len(info.offsets), 1], what
    assert pixels.dtype == torch.uint8 and np.array_equal(pixels.cpu().numpy(), image), what
    if image.ndim == 3:
        depth = mtgs_amd.decode_depth_png(data)
        want = R.depth_from_image(in_file_order[..., ::-1])                           # what cv2.imread hands the reference
        assert depth.dtype == torch.float32 and tuple(depth.shape) == want.shape
        assert np.array_equal(depth.cpu().numpy().view(np.uint32), want.view(np.uint32)), what
    return data


def labels(rng, shape):
    """a few values in runs of random length: literals, short and long matches"""
    n = int(np.prod(shape))
    values = np.repeat(rng.integers(0, 5, n, dtype=np.uint8) * 50, rng.integers(1, 9, n))[:n]
    return values.reshape(shape)


# ---- shapes: W in 1, 2, 3, 63, 64, 65; H in 1, 2, 17; gray and RGB; the three filters; both orders ------------------------------------
@pytest.mark.parametrize("h", [1, 2, 17])
@pytest.mark.parametrize("filter", list(FILTERS))
def test_files_and_pixels_at_the_small_shapes(h, filter):
    rng = np.random.default_rng(100 * h + FILTERS[filter])
    for w in (1, 2, 3, 63, 64, 65):
        for shape in ((h, w), (h, w, 3)):
            for order in ("rgb", "bgr"):
                round_trip(labels(rng, shape), filter, 16, order)
            round_trip(rng.integers(0, 256, shape, dtype=np.uint8), filter, 16, "bgr")


# ---- segment layout ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("segment_bytes, segments_per_row", [(P.MIN_SEGMENT_BYTES, 5), (65, 1), (64, 2), (P.MAX_SEGMENT_BYTES, 1)])
def test_segment_layouts(segment_bytes, segments_per_row):
    """a row stream of 65 bytes: the minimum, one segment equal to the row, and 64, which leaves a 1-byte last segment"""
    rng = np.random.default_rng(7)
    for filter in FILTERS:
        image = labels(rng, (3, 64))
        data = round_trip(image, filter, segment_bytes)
        assert len(P.parse_png(data).offsets) == 3 * segments_per_row
    image = labels(rng, (3, 21, 3))                      # 64 bytes: exactly one segment of 64, four of 16
    assert len(P.parse_png(round_trip(image, "sub", min(segment_bytes, 64))).offsets) == 3 * -(-64 // min(segment_bytes, 64))
    with pytest.raises(ValueError, match="segment_bytes"):
        mtgs_amd.encode_png(dev(image), "sub", P.MIN_SEGMENT_BYTES - 1)


# ---- run lengths ----------------------------------------------------------------------------------------------------------------------
def test_run_lengths_and_runs_that_must_split():
    lengths = [2, 3, 4, 258, 259, 260, 261, 517, 1, 1, 600, 5]
    runs = np.concatenate([np.full(n, v, np.uint8) for v, n in enumerate(lengths, start=1)])[None]
    details = {}
    R.encode(runs, 0, 8192, "rgb", details)
    matches = [v for kind, v in details["tokens"][0] if kind == "M"]
    assert matches == [3, 257, 258, 258, 258, 258, 258, 258, 258, 83, 4]         # 260 and 261 end in literals, 517 = 1 + 258 + 258
    round_trip(runs, "none", 8192)
    R.encode(runs, 0, 512, "rgb", details)                # the runs of 517 and 600 bytes cross a segment start: they split
    assert sum(len(seg) for seg in details["tokens"]) > len(details["tokens"]) + 20
    for seg, (start, n) in zip(details["tokens"], R.segments(1, runs.size + 1, 512)):
        assert seg[0][0] == "L" and sum(v if kind == "M" else 1 for kind, v in seg) == n
    round_trip(runs, "none", 512)
    round_trip(runs, "sub", 512)
    round_trip(np.zeros((3, 700), np.uint8), "none", 512)              # a run through the filter byte 0 ...
    rising = (2 * np.arange(1, 6, dtype=np.uint8))[:, None] * np.ones((1, 300), np.uint8)
    data = round_trip(rising, "up", 512)                               # ... and through the filter byte 2: every byte of the stream is 2
    assert set(R.row_stream(R.file_pixels(rising), 2).reshape(-1)) == {2} and len(data) < 200


# ---- code edges -----------------------------------------------------------------------------------------------------------------------
def test_code_edges():
    info = P.parse_png(round_trip(np.zeros((4, 40), np.uint8), "none", 64))            # all zero: two used symbols and end-of-block
    assert sum(n > 0 for n in info.lit_lengths) == 3 and info.has_distance
    info = P.parse_png(round_trip((np.arange(600) * 37 % 256).astype(np.uint8).reshape(6, 100), "none", 64))
    assert not info.has_distance and not any(info.lit_lengths[257:])                   # no run: no distance code
    info = P.parse_png(round_trip(np.arange(256, dtype=np.uint8).reshape(1, 256), "none", 8192))
    assert all(info.lit_lengths[:257])                                                 # all 256 byte values
    info = P.parse_png(round_trip(np.arange(256, dtype=np.uint8)[::-1].reshape(2, 128).copy(), "up", 16))
    assert sum(n > 0 for n in info.lit_lengths) > 100


def test_a_fibonacci_histogram_forces_the_15_bit_limit():
    image = R.fibonacci_image()
    info = P.parse_png(round_trip(image, "none", 512))
    counts = np.bincount(R.row_stream(R.file_pixels(image), 0).reshape(-1), minlength=256)
    assert max(R.build_lengths(list(counts) + [1], 64)) == 22 and max(info.lit_lengths) == 15


# ---- the stream's size ------------------------------------------------------------------------------------------------------------------
def test_random_bytes_stay_within_the_capacity():
    image = np.random.default_rng(11).integers(0, 256, (40, 50, 3), dtype=np.uint8)
    for segment_bytes in (16, 512):
        data = round_trip(image, "none", segment_bytes)
        ws, capacity, _ = P.sizes(40, 50, 3, segment_bytes)
        assert image.size < len(data) <= capacity and ws > 0                           # incompressible, and inside the bound


@pytest.mark.parametrize("short", [1, 2, 13, 700])
def test_a_short_capacity_sets_overflow_and_stays_inside(short):
    image = np.random.default_rng(12).integers(0, 256, (20, 31, 3), dtype=np.uint8)
    want = R.encode(image, 1, 64)
    capacity, guard = len(want) - short, 64
    buffer = torch.full((capacity + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    out = P.PngStream(buffer[:capacity], torch.zeros(2, dtype=torch.int64, device=DEV))
    stream = mtgs_amd.encode_png(dev(image), "sub", 64, to="device", out=out)
    assert stream is out and int(stream.overflow) == 1 and int(stream.nbytes) == len(want)
    assert bytes(buffer[capacity:].cpu().numpy()) == b"\xa5" * guard                   # nothing behind the buffer
    on_device, info = bytearray(want), P.parse_png(want)                              # the file as the device leaves it: the CRC-32
    on_device[info.payload_offset - 12:info.payload_offset - 8] = bytes(4)             # fields of mtIX and IDAT are the host's
    on_device[info.payload_offset + info.payload_length:info.payload_offset + info.payload_length + 4] = bytes(4)
    assert bytes(buffer[:capacity].cpu().numpy()) == bytes(on_device[:capacity])       # and what fits is the file's start
    with pytest.raises(RuntimeError, match="overflow"):
        stream.tobytes()
    exact = mtgs_amd.encode_png(dev(image), "sub", 64, to="device", capacity=len(want))  # exactly enough: no overflow
    assert int(exact.overflow) == 0 and exact.tobytes() == want


# ---- layouts --------------------------------------------------------------------------------------------------------------------------
def test_strided_and_negative_input_strides_and_a_strided_out():
    rng = np.random.default_rng(13)
    big = labels(rng, (40, 50, 4))
    view = dev(big)[3:37:2, 5:47:3, 1:]                                                # every stride non-contiguous
    image = big[3:37:2, 5:47:3, 1:]
    assert not view.is_contiguous()
    want = R.encode(image, 1, 16)
    same_file(mtgs_amd.encode_png(view, "sub", 16), want, "a view")
    same_file(mtgs_amd.encode_png(view.permute(1, 0, 2), "up", 16), R.encode(image.transpose(1, 0, 2), 2, 16), "transposed")
    same_file(mtgs_amd.encode_png(view[:, :, 0], "sub", 16), R.encode(image[:, :, 0], 1, 16), "one channel of a view")
    for flip, flipped in (("y", image[::-1]), ("x", image[:, ::-1]), ("yx", image[::-1, ::-1])):
        same_file(mtgs_amd.encode_png(view, "sub", 16, flip=flip), R.encode(flipped, 1, 16), f"negative strides: {flip}")
    frame = torch.full((20, 30, 4), 0xA5, dtype=torch.uint8, device=DEV)
    out = frame[1:18, 2:16, :3]
    assert mtgs_amd.decode_png(want, out=out) is out
    assert np.array_equal(out.cpu().numpy(), image)
    frame[1:18, 2:16, :3] = 0xA5
    assert int((frame != 0xA5).sum()) == 0                                              # nothing beside the view
    plane = torch.full((17, 40), np.float32(-1), device=DEV)
    out = plane[:, 3:31:2].unsqueeze(-1)
    assert mtgs_amd.decode_depth_png(want, out=out) is out
    assert np.array_equal(out.cpu().numpy(), R.depth_from_image(image[..., ::-1]))
    plane[:, 3:31:2] = -1
    assert int((plane != -1).sum()) == 0


# ---- repeatability ----------------------------------------------------------------------------------------------------------------------
def test_encoding_twice_gives_identical_bytes():
    image = dev(labels(np.random.default_rng(14), (60, 131, 3)))
    first = mtgs_amd.encode_png(image, "sub", 64)
    for _ in range(3):
        assert mtgs_amd.encode_png(image, "sub", 64) == first


def test_capture_and_replay_follow_the_pixels():
    rng = np.random.default_rng(15)
    first, second = labels(rng, (20, 48, 3)), rng.integers(0, 256, (20, 48, 3), dtype=np.uint8)
    image = dev(first)
    cached = P.upload_png(R.encode(first, 1, 64))
    pixels = torch.zeros((20, 48, 3), dtype=torch.uint8, device=DEV)
    workspace = torch.empty(P.sizes(20, 48, 3, 64)[2], dtype=torch.uint8, device=DEV)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):                      # warm-up on the capture stream: the workspace exists
        out = mtgs_amd.encode_png(image, "sub", 64, to="device")
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    eager = out.tobytes()
    graph = torch.cuda.CUDAGraph()
    allocations = lambda: torch.cuda.memory_stats()["allocation.all.allocated"]
    with torch.cuda.graph(graph, stream=stream):
        before = allocations()
        assert mtgs_amd.encode_png(image, "sub", 64, to="device", out=out) is out
        assert mtgs_amd.decode_png(cached, out=pixels, workspace=workspace) is pixels
        assert allocations() == before                   # nothing was allocated for the file or the pixels
    for now in (second, first):
        image.copy_(dev(now))
        out.data.zero_()
        out.meta.zero_()
        pixels.zero_()
        graph.replay()
        torch.cuda.synchronize()
        same_file(out.tobytes(), R.encode(now, 1, 64), "replay")
        assert np.array_equal(pixels.cpu().numpy(), first)
    assert out.tobytes() == eager


def test_no_host_read_in_encode_and_decode():
    image = labels(np.random.default_rng(16), (20, 48))
    tensor = dev(image)
    mtgs_amd.encode_png(tensor, to="device")             # the workspace of the shape
    cached = P.upload_png(R.encode(image, 1, P.SEGMENT_BYTES))
    pixels = torch.empty((20, 48), dtype=torch.uint8, device=DEV)
    workspace = torch.empty(P.sizes(20, 48, 1)[2], dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        stream = mtgs_amd.encode_png(tensor, to="device")
        mtgs_amd.decode_png(cached, out=pixels, workspace=workspace)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    same_file(stream.tobytes(), R.encode(image, 1, P.SEGMENT_BYTES))
    assert np.array_equal(pixels.cpu().numpy(), image)


# ---- corruption -------------------------------------------------------------------------------------------------------------------------
def test_a_flipped_payload_byte_is_reported_and_stays_inside():
    image = labels(np.random.default_rng(17), (12, 40, 3))
    data = R.encode(image, 1, 32)
    info = R.parse(data)
    clean = R.inflate_segments(info)[0]
    chosen = None
    for at in range(info["first_token_bit"] // 8 + 1, len(info["payload"]) - 8):       # chosen on the CPU: the restatement's reader
        broken = bytearray(info["payload"])                                          # stays inside every segment and the payload
        broken[at] ^= 0x10
        stream, good, inside = R.inflate_segments(info, bytes(broken))
        if inside and not np.array_equal(stream, clean):
            chosen = (at, bytes(broken), stream, good)
            break
    assert chosen is not None
    at, broken, stream, good = chosen
    png = P.upload_png(data)
    png.payload[at] = png.payload[at] ^ 0x10
    assert bytes(png.payload.cpu().numpy()) == broken
    need = P.sizes(12, 40, 3, 32)[2]
    arena = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    frame = torch.full((14, 44, 3), 0xA5, dtype=torch.uint8, device=DEV)
    out, status = mtgs_amd.decode_png(png, out=frame[1:13, 2:42], workspace=arena[:need], return_status=True)
    error, decoded, expected, adler_ok = status.tolist()
    assert adler_ok == 0 and error & P.ERR_ADLER and expected == len(info["offsets"])
    assert decoded == good and (decoded == expected or error & P.ERR_SEGMENT)
    assert bytes(arena[need:].cpu().numpy()) == b"\xa5" * 64                           # nothing behind the workspace
    assert np.array_equal(out.cpu().numpy(), R.unfilter(stream, 12, 40, 3, 1))          # the same wrong pixels as the restatement
    frame[1:13, 2:42] = 0xA5
    assert int((frame != 0xA5).sum()) == 0                                              # nothing outside out


# ---- the two depth rules ------------------------------------------------------------------------------------------------------------------
def test_depth_files_equal_the_references_rule():
    f = np.float32
    edges = np.array([0.0, 0.05, 0.1, np.nextafter(f(0.1), f(0)), 80.0, np.nextafter(f(80), f(100)), 2.56, np.nextafter(f(2.56), f(0)),
                      5.12, 76.8, np.nextafter(f(76.8), f(0)), 79.999, -1.0, 81.0, np.inf, np.nan, 60.5, 60.51], dtype=np.float32)
    rng = np.random.default_rng(18)
    depth = rng.uniform(0, 90, (17, 33)).astype(np.float32)
    depth[:2].flat[:len(edges)] = edges
    depth[5:9, 4:30] = np.float32(12.34)                                             # a flat wall: runs
    for raw_size, roi, max_range, filter in [((17, 33), (0, 0, 33, 17), 80, "sub"), ((30, 41), (5, 9, 33, 17), 60.5, "up"),
                                             ((18, 34), (1, 1, 33, 17), 80, "none")]:
        image = R.depth_image(depth, raw_size, roi, max_range)
        data = mtgs_amd.encode_depth_png(dev(depth), raw_size, roi, max_range, filter=filter, segment_bytes=32)
        same_file(data, R.encode(image, FILTERS[filter], 32, "bgr"), f"depth {raw_size} {roi}")
        assert np.array_equal(np.array(Image.open(io.BytesIO(data)))[..., ::-1], image)
        back = mtgs_amd.decode_depth_png(data)
        want = R.depth_from_image(image)
        assert np.array_equal(back.cpu().numpy().view(np.uint32), want.view(np.uint32))
        assert np.array_equal(mtgs_amd.decode_png(data, "bgr").cpu().numpy(), image)
    x, y, w, h = roi
    kept = (depth >= f(0.1)) & (depth <= f(80))
    error = np.abs(want[y:y + h, x:x + w, 0] - depth)[kept]
    assert error.max() < 0.0101 and (want[y:y + h, x:x + w, 0][~kept] == 0).all()     # centimetres, truncated: not the identity
    strided = dev(np.repeat(depth, 2, axis=1))[:, ::2]
    same_file(mtgs_amd.encode_depth_png(strided, filter="none", segment_bytes=32), R.encode(R.depth_image(depth, (17, 33), (0, 0, 33, 17)), 0, 32, "bgr"))
    with pytest.raises(NotImplementedError, match="max_range"):
        mtgs_amd.encode_depth_png(dev(depth), max_range=700)
