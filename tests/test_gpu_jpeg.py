"""mtgs_amd.jpeg on the device (csrc/jpeg.hip): every file is compared BYTE FOR BYTE with tests/jpeg_refs.py, the NumPy encoder
that tests/test_jpeg_host.py pins to Pillow, and with Pillow's own bytes in tests/golden/jpeg_pillow.npz."""
import io

import numpy as np
import pytest
import torch

import mtgs_amd
from mtgs_amd import jpeg as J
from mtgs_amd import present as P
from tests import jpeg_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_file(got: bytes, want: bytes, what=""):
    if got != want:
        at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError(f"{what}: {len(got)} bytes against {len(want)}, first difference at byte {at} "
                             f"(header: {R.HEADER_BYTES}): {got[max(at - 4, 0):at + 8].hex()} against {want[max(at - 4, 0):at + 8].hex()}")


def float_image(kind, h, w):
    """float32 [h, w, 3] that both conversions treat differently: the uint8 image over 255, plus for noise values beside [0, 1],
    halves and a NaN"""
    x = R.image_of(kind, h, w).astype(np.float32) / np.float32(255)
    if kind == "noise":
        rng = np.random.default_rng(h * 77 + w)
        x = (x + rng.uniform(-0.2, 0.2, x.shape)).astype(np.float32)
        x.flat[0] = np.nan
        x.flat[x.size // 2] = np.float32(100.5 / 255)
    return x


# ---- the cases of the issue --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h, w", R.SIZES, ids=lambda v: str(v))
def test_uint8_files_equal_the_reference(h, w):
    for kind in R.KINDS:
        image = dev(R.image_of(kind, h, w))
        for q in R.QUALITIES:
            for s in R.SUBSAMPLINGS:
                same_file(mtgs_amd.encode_jpeg(image, q, s).tobytes(), R.encoded(kind, h, w, q, s), f"{kind} {h}x{w} q{q} {s}")


@pytest.mark.parametrize("h, w", R.SIZES, ids=lambda v: str(v))
def test_float32_files_equal_the_reference_under_both_conversions(h, w):
    differ = 0
    for kind in R.KINDS:
        x = float_image(kind, h, w)
        image = dev(x)
        as_u8 = {c: R.to_u8(x, c) for c in ("truncate", "round")}
        differ += int((as_u8["truncate"] != as_u8["round"]).any())
        for conversion, u8 in as_u8.items():
            for q in R.QUALITIES:
                for s in R.SUBSAMPLINGS:
                    got = mtgs_amd.encode_jpeg(image, q, s, conversion=conversion).tobytes()
                    same_file(got, R.encode(u8, q, s), f"{kind} {h}x{w} q{q} {s} {conversion}")
    assert differ, "no image told the two conversions apart"


def test_files_equal_pillows_bytes_in_the_fixture():
    cases, (default_image, default_bytes) = R.golden()
    assert len(cases) >= 100
    for (kind, h, w, q, s), (image, want) in cases.items():
        same_file(mtgs_amd.encode_jpeg(dev(image), q, s).tobytes(), want, f"fixture {kind} {h}x{w} q{q} {s}")
    same_file(mtgs_amd.encode_jpeg(dev(default_image)).tobytes(), default_bytes, "the default save: quality 75, 4:2:0")


# ---- across the scans' spines: more than 2048 blocks, more than 2048 chunks -------------------------------------------------------------
def test_more_blocks_than_one_scan_tile():
    h, w = 264, 200
    assert R.n_blocks(h, w, "4:4:4") == 2475 > 2048
    image = R.images("ramp", h, w)
    same_file(mtgs_amd.encode_jpeg(dev(image), 75, "4:4:4").tobytes(), R.encode(image, 75, "4:4:4"), "ramp 264x200")
    same_file(mtgs_amd.encode_jpeg(dev(image), 75, "4:2:0").tobytes(), R.encode(image, 75, "4:2:0"), "ramp 264x200 4:2:0")


def test_more_stuffing_chunks_than_one_scan_tile_and_many_stuffed_bytes():
    h, w = 264, 200
    image = R.images("noise", h, w, seed=5)
    want = R.encode(image, 100, "4:4:4")
    scan = want[R.HEADER_BYTES:-2]
    assert len(scan) > 2048 * 16                               # the stream itself, not only its bound, spans several tiles of chunks
    assert scan.count(b"\xff\x00") > 100                       # noise at quality 100: many stuffed bytes
    same_file(mtgs_amd.encode_jpeg(dev(image), 100, "4:4:4").tobytes(), want, "noise 264x200 q100")


def test_noise_at_quality_100_is_stuffed():
    image = R.image_of("noise", 64, 50)
    want = R.encoded("noise", 64, 50, 100, "4:2:0")
    assert want[R.HEADER_BYTES:-2].count(b"\xff\x00") > 0
    same_file(mtgs_amd.encode_jpeg(dev(image), 100, "4:2:0").tobytes(), want)


def test_a_smooth_ramp_at_quality_1_has_zrl_and_early_eob():
    h, w = 64, 50
    image = R.image_of("ramp", h, w)
    found = {}
    for s in R.SUBSAMPLINGS:
        stats = {}
        R.scan(image, 1, s, stats)
        found[s] = stats
        same_file(mtgs_amd.encode_jpeg(dev(image), 1, s).tobytes(), R.encoded("ramp", h, w, 1, s), f"ramp q1 {s}")
    assert all(st["eob"] == st["blocks"] for st in found.values())           # every block ends early
    # ZRL needs a lone coefficient after 16 zeros, which a smooth ramp at quality 1 does not have: noise at quality 1 does
    noise = R.images("noise", 40, 48, seed=3)
    stats = {}
    R.scan(noise, 25, "4:4:4", stats)
    assert stats["zrl"] > 0 and stats["eob"] > 0
    same_file(mtgs_amd.encode_jpeg(dev(noise), 25, "4:4:4").tobytes(), R.encode(noise, 25, "4:4:4"), "noise q25: ZRL")


# ---- behaviour -------------------------------------------------------------------------------------------------------------------
def test_a_view_with_strides_gives_the_same_bytes():
    h, w = 31, 37
    image = R.images("noise", h, w, seed=11)
    want = R.encode(image, 75, "4:2:0")
    big = torch.zeros((h + 3, 2 * w + 5, 4), dtype=torch.uint8, device=DEV)
    view = big[2:2 + h, 1:1 + 2 * w:2, 1:4]
    view.copy_(dev(image))
    assert not view.is_contiguous()
    same_file(mtgs_amd.encode_jpeg(view, 75, "4:2:0").tobytes(), want, "strided uint8")
    planes = dev(image.astype(np.float32) / np.float32(255)).permute(2, 0, 1).contiguous().permute(1, 2, 0)   # channels first in memory
    assert not planes.is_contiguous()
    same_file(mtgs_amd.encode_jpeg(planes, 75, "4:2:0", conversion="round").tobytes(), want, "channel-major float32")


def test_encoding_twice_gives_identical_bytes():
    image = dev(R.images("noise", 100, 131, seed=12))
    first = mtgs_amd.encode_jpeg(image, 95, "4:2:0").tobytes()
    for _ in range(3):
        assert mtgs_amd.encode_jpeg(image, 95, "4:2:0").tobytes() == first


@pytest.mark.parametrize("short", [1, 2, 3, 700])
def test_a_short_capacity_sets_overflow_and_stays_inside(short):
    image = R.image_of("noise", 40, 48)
    want = R.encoded("noise", 40, 48, 95, "4:2:0")
    capacity, guard = len(want) - short, 64
    buffer = torch.full((capacity + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    out = J.JpegStream(buffer[:capacity], torch.zeros(2, dtype=torch.int64, device=DEV))
    stream = mtgs_amd.encode_jpeg(dev(image), 95, "4:2:0", out=out)
    assert stream is out and int(stream.overflow) == 1 and int(stream.nbytes) == len(want)
    assert bytes(buffer[capacity:].cpu().numpy()) == b"\xa5" * guard                 # nothing behind the buffer
    assert bytes(buffer[:capacity].cpu().numpy()) == want[:capacity]                 # and what fits is the file's start
    with pytest.raises(RuntimeError, match="overflow"):
        stream.tobytes()
    exact = mtgs_amd.encode_jpeg(dev(image), 95, "4:2:0", capacity=len(want))         # exactly enough: no overflow
    assert int(exact.overflow) == 0 and exact.tobytes() == want


def test_capture_and_replay_follow_the_pixels():
    h, w = 40, 48
    first, second = R.images("noise", h, w, seed=21), R.images("ramp", h, w)
    image = dev(first)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):                      # warm-up on the capture stream: the header and the workspace exist
        out = mtgs_amd.encode_jpeg(image, 40)
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    eager = out.tobytes()
    graph = torch.cuda.CUDAGraph()
    allocations = lambda: torch.cuda.memory_stats()["allocation.all.allocated"]
    with torch.cuda.graph(graph, stream=stream):
        before = allocations()
        assert mtgs_amd.encode_jpeg(image, 40, out=out) is out
        assert allocations() == before                   # nothing was allocated for the file
    for pixels in (second, first):
        image.copy_(dev(pixels))
        out.data.zero_()
        out.meta.zero_()
        graph.replay()
        torch.cuda.synchronize()
        same_file(out.tobytes(), R.encode(pixels, 40, "4:2:0"), "replay")
    assert out.tobytes() == eager


def test_no_host_read_in_encode():
    image = dev(R.image_of("noise", 40, 48))
    mtgs_amd.encode_jpeg(image, 75)                      # the one upload of the header
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        stream = mtgs_amd.encode_jpeg(image, 75)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    same_file(stream.tobytes(), R.encoded("noise", 40, 48, 75, "4:2:0"))
    key = (40, 48, 75, "4:2:0", image.device)
    table = J._DEVICE_HEADERS[key]
    mtgs_amd.encode_jpeg(image, 75)
    assert J._DEVICE_HEADERS[key] is table               # uploaded once


def test_viewer_and_render_frames_as_jpeg():
    H, W = 30, 53
    rng = np.random.default_rng(31)
    outputs = {"rgb": dev(rng.uniform(0, 1, (H, W, 3)).astype(np.float32)), "depth": dev(rng.uniform(1, 50, (H, W, 1)).astype(np.float32)),
               "accumulation": dev(rng.uniform(0, 1, (H, W, 1)).astype(np.float32))}
    o = P.ColormapOptions("gray")
    aspect = (W + 14) / H
    frame = P.viewer_frame(outputs, "depth", o, "rgb", None, 0.4, aspect)
    assert isinstance(frame, torch.Tensor) and frame.dtype == torch.uint8            # without the keyword: the frame, as before
    got = P.viewer_frame(outputs, "depth", o, "rgb", None, 0.4, aspect, jpeg_quality=40)
    assert isinstance(got, J.JpegStream)
    assert got.tobytes() == mtgs_amd.encode_jpeg(frame, 40).tobytes() == R.encode(frame.cpu().numpy(), 40, "4:2:0")
    tool = P.render_frame(outputs, ["rgb", "depth"], 1.0, 50.0, o)
    got = P.render_frame(outputs, ["rgb", "depth"], 1.0, 50.0, o, jpeg_quality=75)
    assert got.tobytes() == mtgs_amd.encode_jpeg(tool, 75).tobytes() == R.encode(tool.cpu().numpy(), 75, "4:2:0")


def test_pillow_decodes_our_stream_as_the_references():
    Image = pytest.importorskip("PIL.Image", reason="Pillow is not installed")
    for kind, s in (("noise", "4:2:0"), ("ramp", "4:4:4")):
        image = R.image_of(kind, 31, 9)
        ours = mtgs_amd.encode_jpeg(dev(image), 75, s).tobytes()
        a, b = (np.asarray(Image.open(io.BytesIO(data)).convert("RGB")) for data in (ours, R.encoded(kind, 31, 9, 75, s)))
        assert a.shape == (31, 9, 3) and np.array_equal(a, b)
