"""mtgs_amd.undistort.redistort_image / redistort_map and mtgs_amd.evaldump on the device: bit for bit the NumPy restatement
(tests/redistort_refs.py).  No tolerance anywhere: the map is fp64 with one rounding per operation (add, multiply and divide are
correctly rounded on both sides), the float conversion is two correctly rounded fp32 operations, everything after that is integer
arithmetic.  Frames are compared for equality, the map as uint32 patterns, files as bytes.  No input has more than 20 000 pixels; every
reference is computed once per case."""
import io
from functools import lru_cache

import numpy as np
import pytest
import torch

from mtgs_amd import evaldump as E
from mtgs_amd import jpeg as J
from mtgs_amd import undistort as U
from tests import jpeg_refs
from tests import redistort_refs as R
from tests import undistort_refs

pytestmark = pytest.mark.gpu
TW, TH = U.TILE_W, U.TILE_H
ITERATIONS = (0, 1, 5, 20, 64)

# The lenses of tests/test_gpu_undistort.py.  "wide" bends a pincushion lens with tangential terms back through a new camera of 1.4
# times the focal length: the map runs off the image that is read on all four sides.  "barrel" is a nuPlan-like lens, with four
# coefficients in keep_focal_length and with k3 in mode "optimal" -- the camera pair invert_distortion builds.  "folded" has
# 1 + k1 r2 < 0 at the corners of the raw image.
WIDE = (0.3, 0.1, 0.02, -0.015, 0.02)
BARREL = (-0.356, 0.173, 0.001, -0.0005)
FOLDED = (-4.0, 0.0, 0.0, 0.0)
EXACT = (16.0, 8.0, 7.5, 5.5)             # powers of two after the half pixel is taken off: the maps without a lens are exact


def lens(h, w, zoom=1.4):
    """(K, new_K) in the dataset's convention for a raw image of h x w: the principal point off the centre, K' = zoom K"""
    f = 0.9 * max(h, w, 8)
    K = (f, 1.05 * f, 0.5 * w + 0.3, 0.5 * h - 0.2)
    return K, (zoom * K[0], zoom * K[1], K[2] + 0.4, K[3] - 0.3)


def shifted(dx, dy=0.0):
    return dict(K=EXACT, D=(0.0,) * 4, new_K=(EXACT[0], EXACT[1], EXACT[2] + dx, EXACT[3] + dy))


# name -> (the raw size that is WRITTEN, the size that is READ or None for the same, undistort_camera's arguments)
CASES = {}
for _h, _w in ((1, 1), (2, 2), (TH - 1, TW - 1), (TH, TW), (TH + 1, TW + 1), (2 * TH + 1, 2 * TW + 2), (37, 53)):
    _K, _newK = lens(_h, _w)
    CASES[f"wide-{_h}x{_w}"] = ((_h, _w), None, dict(K=_K, D=WIDE, new_K=_newK))
CASES["other-size"] = ((37, 53), (TH + 2, 2 * TW + 1), dict(K=lens(37, 53)[0], D=WIDE, new_K=lens(TH + 2, 2 * TW + 1)[1]))
CASES["smaller-read"] = ((TH + 1, TW + 1), (3, 41), dict(K=lens(TH + 1, TW + 1)[0], D=BARREL, new_K=lens(3, 41, 0.8)[1]))
CASES["barrel-37x53"] = ((37, 53), None, dict(K=lens(37, 53)[0], D=BARREL, mode="keep_focal_length"))
CASES["barrel-k3-37x53"] = ((37, 53), None, dict(K=lens(37, 53)[0], D=BARREL + (-0.052,), mode="keep_focal_length"))
CASES["optimal-37x53"] = ((37, 53), None, dict(K=lens(37, 53)[0], D=BARREL + (-0.052,), mode="optimal"))
CASES["folded"] = ((37, 53), None, dict(K=lens(37, 53)[0], D=FOLDED, mode="keep_focal_length"))
CASES["half"] = ((13, 17), None, shifted(0.5, 0.5))
CASES["tie-1/64"] = ((13, 17), None, shifted(1.0 / 64))
CASES["tie-3/64"] = ((13, 17), None, shifted(3.0 / 64, 3.0 / 64))
CASES["nan"] = ((13, 17), None, dict(K=(16.0, 8.0, 7.75, 5.75), D=(float("nan"), 0.0, 0.0, 0.0), mode="keep_focal_length"))
CASES["huge"] = ((13, 17), None, dict(K=(16.0, 8.0, 7.75, 5.75), D=(0.0, 0.0, 1e300, 1e300, 0.0), mode="keep_focal_length"))
LAYOUT_CASES = ("wide-37x53", "other-size", "optimal-37x53", f"wide-{TH + 1}x{TW + 1}")


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()             # a copy: the cached sources are read-only


def host(t):
    return t.cpu().numpy()


def same(got, want, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    a, b = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if a.dtype == np.float32:
        a, b = a.view(np.uint32), b.view(np.uint32)
    wrong = int((a != b).sum())
    assert wrong == 0, f"{what}: {wrong} of {want.size} elements differ"


@lru_cache(maxsize=None)
def camera(name):
    raw, read, kw = CASES[name]
    return U.undistort_camera(size=raw, out_size=read, **kw)


def map_arguments(cam):
    """(K, D, new_K) of the restatement: the scalars the camera uploaded, the half pixel already taken off"""
    p = cam.params.cpu().numpy()
    return tuple(p[:4]), tuple(p[8:13]), tuple(p[4:8])


@lru_cache(maxsize=None)
def sources(shape, seed=0):
    """the image that is read: uint8 and float32 (in and beyond [0, 1], on and just below k / 255, NaN), 3 channels"""
    h, w = shape
    rng = np.random.default_rng([seed, h, w])
    u8 = rng.integers(1, 256, (h, w, 3), dtype=np.uint8)
    f32 = rng.uniform(-0.1, 1.1, (h, w, 3)).astype(np.float32)
    k = (rng.integers(0, 256, (h, w, 3)) / np.float32(255)).astype(np.float32)
    pick = rng.integers(0, 8, (h, w, 3))
    f32 = np.where(pick == 0, k, np.where(pick == 1, np.nextafter(k, np.float32(-1)), np.where(pick == 2, np.float32(np.nan), f32))).astype(np.float32)
    for a in (u8, f32):
        a.setflags(write=False)
    return {"u8": u8, "f32": f32}


@lru_cache(maxsize=None)
def reference_map(name, iterations):
    cam = camera(name)
    K, D, new_K = map_arguments(cam)
    m = R.redistort_map(K, D, new_K, *cam.source_size, iterations)
    m.setflags(write=False)
    return m


@lru_cache(maxsize=None)
def reference(name, iterations, kind="u8", conversion="truncate", channels=3):
    src = sources(camera(name).size)[kind]
    return R.remap(src if channels == 3 else src[:, :, 1:2], reference_map(name, iterations), conversion)


# ---- the cases are what they claim to be (host arithmetic, stated here so that a changed lens cannot empty a test quietly) --------
def test_the_lenses_leave_the_image_fold_over_and_change_with_the_iterations():
    def outside(name, iterations=5):
        cam, m = camera(name), reference_map(name, iterations)
        ix, iy = undistort_refs.fixed(m[..., 0]) >> 5, undistort_refs.fixed(m[..., 1]) >> 5
        return (ix < -1) | (ix >= cam.size[1]) | (iy < -1) | (iy >= cam.size[0])
    for name in ("wide-37x53", f"wide-{2 * TH + 1}x{2 * TW + 2}", "other-size"):
        o = outside(name)
        assert o[0, 0] and o[0, -1] and o[-1, 0] and o[-1, -1] and 0.05 < o.mean() < 0.96, (name, o.mean())        # other-size reads 6 rows: 95 %
    # a barrel lens pushes the raw corners outwards: beyond the image in keep_focal_length, and mode "optimal" (alpha = 1) keeps them in
    assert outside("barrel-37x53")[0, 0] and not outside("barrel-37x53")[18, 26] and not outside("optimal-37x53").any()
    assert outside("nan").all() and outside("huge").all() and outside("huge", 1).all() and not outside("huge", 0).any()
    sizes = [(CASES[n][0], camera(n).size) for n in CASES]
    assert sum(raw != read for raw, read in sizes) >= 2
    # the iteration count moves the map of every lens with coefficients: 0, 1 and 5 differ, and the barrel lenses have not settled at
    # 5 in float32 either (by 64 a float32 map no longer moves)
    for name in ("wide-37x53", "barrel-37x53", "barrel-k3-37x53", "optimal-37x53", "folded"):
        maps = [reference_map(name, n) for n in ITERATIONS]
        assert not np.array_equal(maps[0], maps[1]) and not np.array_equal(maps[1], maps[2]), name
        assert name in ("wide-37x53", "folded") or not np.array_equal(maps[2], maps[3]), name
    assert not np.array_equal(reference_map("barrel-37x53", 5), reference_map("barrel-k3-37x53", 5))
    # the folded lens: the corners are the plain change of camera at every count, the centre is not
    plain, five = reference_map("folded", 0), reference_map("folded", 5)
    for i, j in ((0, 0), (0, -1), (-1, 0), (-1, -1)):
        assert np.array_equal(plain[i, j], five[i, j]) and np.array_equal(plain[i, j], reference_map("folded", 64)[i, j])
    assert 0.1 < (plain == five).all(-1).mean() < 0.9


# ---- the map and the frame ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iterations", ITERATIONS)
@pytest.mark.parametrize("name", CASES)
def test_the_map_and_the_frame_are_the_restatement_bit_for_bit(name, iterations, monkeypatch):
    cam, want_map = camera(name), reference_map(name, iterations)
    got_map = U.redistort_map(cam, iterations)
    assert got_map.shape == cam.source_size + (2,) and got_map.dtype == torch.float32
    m = host(got_map)
    if name in ("nan", "huge"):                  # NaN payloads are nobody's contract: the non-finite entries are in the same places
        assert np.array_equal(np.isnan(m), np.isnan(want_map)) and np.array_equal(m[~np.isnan(m)], want_map[~np.isnan(want_map)])
    else:
        same(m, want_map, "map")
    src = dev(sources(cam.size)["u8"])
    calls = []
    monkeypatch.setattr(U, "call", lambda fn, *a, _call=U.call: (calls.append(fn), _call(fn, *a))[1])
    out = U.redistort_image(src, cam, iterations)
    assert calls == ["mtgs_redistort_frame"]                                          # one launch
    assert out.dtype == torch.uint8 and out.shape == cam.source_size + (3,) and out.is_contiguous()
    want = reference(name, iterations)
    same(host(out), want, "frame, the map evaluated in the launch")
    # the same bytes from a given map; the iteration count then plays no part
    same(host(U.redistort_image(src, cam, iterations, map=got_map)), want, "frame from the map in memory")
    same(host(U.redistort_image(src, cam, 64 - iterations, map=dev(want_map))), want, "frame from the restatement's map")
    into = torch.full(cam.source_size + (3,), 77, dtype=torch.uint8, device="cuda")
    assert U.redistort_image(src, cam, iterations, out=into) is into
    same(host(into), want, "out=")
    if name in ("nan", "huge") and iterations:
        assert not want.any()


# ---- sources: dtype, channels, conversion, layout ------------------------------------------------------------------------------------
def launch(cam, base, is_float, strides, channels, iterations, conversion):
    """the record written by hand: torch refuses negative strides"""
    out = torch.full(cam.source_size + (channels,), 77, dtype=torch.uint8, device="cuda")
    U._launch_redistort(cam, base, is_float, strides, channels, out, iterations, conversion, None, torch.cuda.current_stream().cuda_stream)
    return out


@pytest.mark.parametrize("conversion", ["truncate", "round"])
@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("name", LAYOUT_CASES)
def test_every_source_format_and_layout_gives_the_same_bytes(name, channels, kind, conversion):
    cam, iterations = camera(name), 5
    want = reference(name, iterations, kind, conversion, channels)
    full = sources(cam.size)[kind]
    a = full if channels == 3 else full[:, :, 1:2]
    h, w = cam.size
    t = dev(a)
    same(host(U.redistort_image(t, cam, iterations, conversion)), want, "contiguous")
    # planes: CHW memory looked at as HWC
    chw = t.permute(2, 0, 1).contiguous().permute(1, 2, 0)
    assert channels == 1 or (chw.stride() == (w, 1, h * w) and not chw.is_contiguous())
    same(host(U.redistort_image(chw, cam, iterations, conversion)), want, "CHW viewed as HWC")
    if channels == 3:                            # the middle channel of an RGB frame read in place
        same(host(U.redistort_image(dev(full)[:, :, 1:2], cam, iterations, conversion)), reference(name, iterations, kind, conversion, 1),
             "a channel slice")
    # a base offset by ONE element: a misaligned byte image; a float image stays 4-byte aligned
    flat = torch.zeros(a.size + 1, dtype=t.dtype, device="cuda")
    flat[1:] = t.reshape(-1)
    off = flat[1:].view(h, w, channels)
    assert off.data_ptr() == flat.data_ptr() + t.element_size()
    same(host(U.redistort_image(off, cam, iterations, conversion)), want, "a base offset by one element")
    # flipped in both axes and in the channels: negative strides over the flipped allocation, the base at its last element
    flipped = torch.flip(t, dims=(0, 1, 2)).contiguous()
    base = flipped.data_ptr() + (flipped.numel() - 1) * flipped.element_size()
    got = launch(cam, base, kind == "f32", tuple(-s for s in flipped.stride()), channels, iterations, conversion)
    same(host(got), want, "negative strides")
    if kind == "f32":                            # the conversion, then the 8-bit rule: the same as converting first
        as_bytes = dev(jpeg_refs.to_u8(a, conversion))
        same(host(U.redistort_image(as_bytes, cam, iterations)), want, "the converted bytes as a uint8 source")


# ---- identities that need no recall, and the dump --------------------------------------------------------------------------------------
def test_under_the_identity_camera_the_file_is_the_file_of_the_frame():
    h, w = 24, 40
    cam = U.undistort_camera(EXACT, (0.0,) * 4, (h, w), new_K=EXACT)
    x = dev(sources((h, w))["f32"])
    for iterations in (0, 5):
        raw = U.redistort_image(x, cam, iterations)
        same(host(raw), jpeg_refs.to_u8(sources((h, w))["f32"], "truncate"), "the identity")
        assert J.encode_jpeg(raw).tobytes() == J.encode_jpeg(x).tobytes() == E.eval_dump(x, "nuplan", cam=cam, iterations=iterations)["rendered"].tobytes()
    assert J.encode_jpeg(U.redistort_image(x, cam, conversion="round")).tobytes() == J.encode_jpeg(x, conversion="round").tobytes()


@lru_cache(maxsize=None)
def dumped(name="optimal-37x53", iterations=5):
    """(the restatement's raw pixels, their file by the NumPy encoder that tests/test_jpeg_host.py pins to Pillow)"""
    pixels = reference(name, iterations, "f32", "truncate")
    return pixels, jpeg_refs.encode(pixels, 75, "4:2:0")


def test_the_nuplan_dump_is_the_file_of_the_restatements_pixels():
    name = "optimal-37x53"
    cam = camera(name)
    x = dev(sources(cam.size)["f32"])
    pixels, want = dumped()
    out = E.eval_dump(x, "nuplan", cam=cam)
    assert set(out) == {"rendered"} and out["rendered"].tobytes() == want
    assert E.eval_dump(x, "nuplan", cam=cam, map=U.redistort_map(cam))["rendered"].tobytes() == want
    assert E.eval_dump(x, "nuplan", cam=cam, iterations=20)["rendered"].tobytes() == jpeg_refs.encode(reference(name, 20, "f32"), 75, "4:2:0")
    assert E.eval_dump(x, "nuplan", cam=cam, quality=90, subsampling="4:4:4")["rendered"].tobytes() == jpeg_refs.encode(pixels, 90, "4:4:4")


def test_the_nuplan_dump_is_pillows_default_save():
    Image = pytest.importorskip("PIL.Image", reason="Pillow is not installed")
    cam = camera("optimal-37x53")
    pixels, _ = dumped()
    buf = io.BytesIO()
    Image.fromarray(pixels).save(buf, format="JPEG", quality=75)
    assert E.eval_dump(dev(sources(cam.size)["f32"]), "nuplan", cam=cam)["rendered"].tobytes() == buf.getvalue()


def test_the_sequential_dumps_are_the_encoder():
    s = sources((37, 53))
    x, gt = dev(s["f32"]), dev(sources((37, 53), seed=3)["f32"])
    want, want_gt = J.encode_jpeg(x, conversion="truncate").tobytes(), J.encode_jpeg(gt, conversion="truncate").tobytes()
    assert want == jpeg_refs.encode(jpeg_refs.to_u8(s["f32"], "truncate"), 75, "4:2:0") and want != want_gt
    out = E.eval_dump(x, "sequential")
    assert set(out) == {"rendered"} and out["rendered"].tobytes() == want
    out = E.eval_dump(x, "sequential_with_gt", gt_image=gt)
    assert set(out) == {"rendered", "gt_processed"} and out["rendered"].tobytes() == want and out["gt_processed"].tobytes() == want_gt
    assert E.eval_dump(dev(s["u8"]), "sequential", quality=40)["rendered"].tobytes() == J.encode_jpeg(dev(s["u8"]), 40).tobytes()


# ---- one graph -----------------------------------------------------------------------------------------------------------------------
def test_a_captured_redistortion_follows_its_camera_and_repeats_every_bit():
    names = ("wide-37x53", "optimal-37x53")
    cams = [camera(n) for n in names]
    frames = [dev(sources((37, 53), seed)["f32"]) for seed in (0, 5)]
    static = frames[0].clone()
    cam = U.undistort_camera(size=(37, 53), **CASES[names[0]][2])            # its scalars are uploaded here, before the capture
    run = lambda: U.redistort_image(static, cam, 20)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        run()
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = run()
    seen = {}
    for which, lens_at in ((1, 0), (0, 1), (0, 0), (0, 1)):
        static.copy_(frames[which])
        cam.params.copy_(cams[lens_at].params)                                 # the camera lives on the device: a replay follows it
        out.fill_(77)
        graph.replay()
        torch.cuda.synchronize()
        K, D, new_K = map_arguments(cams[lens_at])
        want = R.redistort_image(sources((37, 53), (0, 5)[which])["f32"], K, D, new_K, (37, 53), 20)
        same(host(out), want, f"replay of frame {which} through lens {names[lens_at]}")
        assert seen.setdefault((which, lens_at), host(out).tobytes()) == host(out).tobytes()           # two replays: every bit again
    assert len(set(seen.values())) == 3
