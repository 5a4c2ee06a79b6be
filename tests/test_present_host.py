"""Presenting frames (mtgs_amd/present.py, csrc/present.hip, include/mtgs_present.h) without a GPU: the header as a group of its
own, the layout arithmetic against hand-worked cases, the two references of tests/present_refs.py against each other on the CPU,
what the Python layer refuses before it touches a device, and the host-side checks of the C entry points."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from mtgs_amd import present as P
from tests import present_refs as R

NAMES = ["mtgs_present_compose", "mtgs_present_depth_resize", "mtgs_present_stats", "mtgs_present_workspace_bytes"]


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_the_header_is_declared_bound_and_exported(hip_lib):
    """include/mtgs_present.h is a group of its own (tests/test_abi.py checks every group against its header, its reviewed record
    tests/golden/abi_signatures_present.txt and the library): its entry points, its panel record and its constants."""
    from mtgs_amd import _abi, _lib
    abi = _abi.header_abi("mtgs_present.h")
    assert sorted(_lib.GROUPS["mtgs_present.h"]) == NAMES
    # the panel record the Python layer fills is the header's struct, of the size the library reports
    ws, pb = C.c_size_t(0), C.c_size_t(0)
    assert hip_lib.mtgs_present_workspace_bytes(C.byref(ws), C.byref(pb)) == 0
    assert pb.value == P._PANEL.itemsize == 96 and P._PANEL == abi.structs["mtgs_present_panel"]
    assert ws.value == P._WS_BYTES == 8 * 256 * 2 * 4
    assert P.MAX_PANELS == abi.constants["MTGS_PRESENT_MAX_PANELS"] == 8
    assert [abi.constants["MTGS_PRESENT_" + k] for k in ("RGB", "FLOAT", "DEPTH", "BOOL")] == [0, 1, 2, 3]


# ---- layout arithmetic -------------------------------------------------------------------------------------------------------------
def test_split_index_by_hand():
    assert P.split_index(0.0, 100) == 0
    assert P.split_index(1.0, 100) == 99            # 100 %: the last column still shows the divider
    assert P.split_index(0.5, 100) == 50 and P.split_index(0.5, 53) == 26 and P.split_index(0.999, 53) == 52
    for pct in (0.0, 0.5, 1.0):
        assert P.split_index(pct, 1) == 0             # a width of 1


def test_pad_sizes_by_hand():
    assert P.pad_sizes(100, 100, None) == (0, 0)
    assert P.pad_sizes(100, 100, 1.0) == (0, 0)
    # width: (aspect * H - W) // 2 -> 100 x 100 to aspect 1.10 gives 5.0 -> nothing; 1.12 gives 6 on each side
    assert P.pad_sizes(100, 100, 1.10) == (0, 0)
    assert P.pad_sizes(100, 100, 1.12) == (0, 6)
    assert P.pad_sizes(100, 100, 2.0) == (0, 50)
    # height: (W / aspect - H) // 2 -> 100 wide, 40 high, aspect 2 gives (50 - 40) // 2 = 5 -> nothing; 38 high gives 6
    assert P.pad_sizes(40, 100, 2.0) == (0, 0)
    assert P.pad_sizes(38, 100, 2.0) == (6, 0)
    assert P.pad_sizes(30, 53, 1.0) == (11, 0)        # (53 - 30) // 2


def test_depth_size_by_hand():
    # 30 x 53 = 1590 pixels: below both budgets, never enlarged
    for state in ("low_move", "low_static", "high"):
        assert P.depth_size(30, 53, state) == (30, 53)
    # 128 x 128 is the low budget exactly
    assert P.depth_size(128, 128, "low_move") == (128, 128) and P.depth_size(128, 128, "high") == (128, 128)
    # 1080 x 1920: the scale is the ratio of the pixel counts, applied to each side (the reference's arithmetic)
    low, high = 128 * 128 / (1080 * 1920), 512 * 512 / (1080 * 1920)
    assert P.depth_size(1080, 1920, "low_move") == P.depth_size(1080, 1920, "low_static") == (int(1080 * low), int(1920 * low)) == (8, 15)
    assert P.depth_size(1080, 1920, "high") == (int(1080 * high), int(1920 * high)) == (136, 242)
    assert P.depth_size(0, 0, "high") == (0, 0)
    with pytest.raises(ValueError, match="state"):
        P.depth_size(10, 10, "medium")
    assert P.concat_columns([5, 3, 9]) == [0, 5, 8]


# ---- the two references against each other, on the CPU -------------------------------------------------------------------------------
def _rand(shape, seed, lo=0.02, hi=0.98):
    return np.random.default_rng(seed).uniform(lo, hi, size=shape).astype(np.float32)


@pytest.mark.parametrize("name, invert, acc", [("turbo", False, False), ("viridis", True, True), ("gray", False, True), ("magma", True, False)])
def test_restatement_equals_transcription_without_a_scalar_division(name, invert, acc):
    """near = 0, far = 1 (the divisor is then 1 + 1e-10, whose fp32 reciprocal is 1: no rounding that depends on how the division is
    carried out), colormap_min / max that are exact in fp32: both references give the same bytes."""
    H, W = 30, 53
    depth, a = _rand((H, W, 1), 1), _rand((H, W, 1), 2, 0.0, 1.0)
    lut = None if name == "gray" else R.tables()[name]
    for cmin, cmax in ((0.0, 1.0), (0.25, 0.75)):
        p = R.panel("depth", depth, lut=lut, cmin=cmin, cmax=cmax, invert=invert, acc=a if acc else None, near=0.0, far=1.0)
        want = R.ns_apply_depth_colormap(torch.from_numpy(depth), torch.from_numpy(a) if acc else None, 0.0, 1.0,
                                         R.NSColormapOptions(name, False, cmin, cmax, invert)).numpy()
        got, _ = R.frame_np([p], [(0, 0, H, W, 0)], H, W, fmt="float")
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        got8, _ = R.frame_np([p], [(0, 0, H, W, 0)], H, W, fmt="truncate")
        assert np.array_equal(got8, (torch.from_numpy(want) * 255).type(torch.uint8).numpy())


def test_viewer_and_render_layouts_of_both_references_agree():
    H, W = 17, 65
    rgb, depth, a = _rand((H, W, 3), 3, 0.0, 1.0), _rand((H, W, 1), 4), _rand((H, W, 1), 5, 0.0, 1.0)
    outputs = {"rgb": torch.from_numpy(rgb), "depth": torch.from_numpy(depth), "accumulation": torch.from_numpy(a)}
    lut = R.tables()["turbo"]
    for pct, aspect in ((0.5, None), (0.0, 1.0), (1.0, 8.0)):
        k = P.split_index(pct, W)
        ph, pw = P.pad_sizes(H, W, aspect)
        want = R.viewer_frame_torch(outputs, "rgb", R.NSColormapOptions(), "depth", R.NSColormapOptions(), pct, aspect)
        panels = [R.panel("rgb", rgb), R.panel("float", depth, lut=lut)]
        got, _ = R.frame_np(panels, [(ph, pw, H, k, 0), (ph, pw + k, H, W - k, k)], H + 2 * ph, W + 2 * pw, pw + k, "truncate")
        assert got.shape == want.shape and np.array_equal(got, want), (pct, aspect)
        assert tuple(got[ph, pw + k]) == (33, 40, 48)
    want_f, want_8 = R.render_frame_torch(outputs, ["rgb", "depth"], 0.0, 1.0, R.NSColormapOptions())
    panels = [R.panel("rgb", rgb), R.panel("depth", depth, lut=lut, acc=a, near=0.0, far=1.0)]
    places = [(0, 0, H, W, 0), (0, W, H, W, 0)]
    assert np.array_equal(R.frame_np(panels, places, H, 2 * W, fmt="float")[0], want_f)
    assert np.array_equal(R.frame_np(panels, places, H, 2 * W, fmt="round")[0], want_8)


def test_gray_boolean_nan_and_the_depth_resize_of_both_references():
    H, W = 7, 9
    v = _rand((H, W, 1), 6)
    v[3, 4, 0] = np.nan
    want = R.ns_apply_colormap(torch.from_numpy(v), R.NSColormapOptions("gray")).numpy()
    got = R.panel_np(R.panel("float", v))
    assert np.array_equal(got, want) and got[3, 4].tolist() == [0.0, 0.0, 0.0] and got.shape == (H, W, 3)
    want = R.ns_apply_colormap(torch.from_numpy(v), R.NSColormapOptions("turbo", invert=True)).numpy()
    got = R.panel_np(R.panel("float", v, lut=R.tables()["turbo"], invert=True))
    assert np.array_equal(got, want) and np.array_equal(got[3, 4], R.tables()["turbo"][0])     # 1 - NaN is NaN, then 0
    # a NaN in a source whose extrema are taken: every pixel NaN -> 0 -> entry 0
    got = R.panel_np(R.panel("depth", v, lut=R.tables()["turbo"]))
    assert (got == R.tables()["turbo"][0]).all()
    want = R.ns_apply_depth_colormap(torch.from_numpy(v), colormap_options=R.NSColormapOptions("turbo")).numpy()
    assert np.array_equal(got, want)
    mask = np.random.default_rng(7).random((H, W, 1)) < 0.5
    want = R.ns_apply_colormap(torch.from_numpy(mask)).numpy()
    got = R.panel_np(R.panel("bool", mask))
    assert np.array_equal(got, want) and set(np.unique(got)) == {0.0, 1.0}
    # quantisation: clamped, NaN -> 0, 1.0 -> 255 in both modes, 0.5 -> 127 truncated and 128 rounded
    x = np.array([[[-0.5, np.nan, 1.5], [1.0, 0.5, 0.999]]], dtype=np.float32)
    assert R.quantise_np(x, "truncate").tolist() == [[[0, 0, 255], [255, 127, 254]]]
    assert R.quantise_np(x, "round").tolist() == [[[0, 0, 255], [255, 128, 255]]]
    # the depth resize: NumPy against torch on the CPU, within the bound of the GPU test
    d = _rand((30, 53), 8, 0.5, 80.0)
    for oh, ow in ((30, 53), (11, 20), (1, 1)):
        got, lo, hi = R.depth_resize_np(d, oh, ow, 2.5)
        want = torch.nn.functional.interpolate(torch.from_numpy(d)[None, None], size=(oh, ow), mode="bilinear")[0, 0].numpy() * np.float32(2.5)
        bound = 2.5 * (2.0 ** -22 * 53 * (hi - lo) + 8 * 2.0 ** -24 * np.maximum(np.abs(hi), np.abs(lo))) + 2.0 ** -24 * np.abs(want)
        assert (np.abs(got.astype(np.float64) - want) <= bound).all()


# ---- what the Python layer refuses, before anything is launched -------------------------------------------------------------------------
def test_python_checks_name_the_argument():
    with pytest.raises(NotImplementedError, match=r"image has 4 channels.*PCA colormap"):
        P.colorize(torch.zeros(4, 5, 4))
    with pytest.raises(NotImplementedError, match="no colormap for 2 channel"):
        P.colorize(torch.zeros(4, 5, 2))
    with pytest.raises(ValueError, match=r"image must be a \[H, W, C\] tensor"):
        P.colorize(torch.zeros(4, 5))
    with pytest.raises(TypeError, match="3-channel image must be float32"):
        P.colorize(torch.zeros(4, 5, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="image must be contiguous"):
        P.colorize(torch.zeros(4, 10, 1)[:, ::2])
    rgb = torch.zeros(4, 5, 3)
    assert P.colorize(rgb) is rgb                                  # the reference returns the tensor itself
    with pytest.raises(TypeError, match=r"depth must be float32 \[H, W, 1\]"):
        P.colorize_depth(torch.zeros(4, 5, 3))
    with pytest.raises(ValueError, match="accumulation must be contiguous float32"):
        P.colorize_depth(torch.zeros(4, 5, 1), torch.zeros(4, 6, 1))
    outputs = {"rgb": torch.zeros(4, 5, 3), "depth": torch.zeros(4, 5, 1), "accumulation": torch.zeros(4, 5, 1), "tall": torch.zeros(6, 5, 3)}
    with pytest.raises(KeyError, match="output_render 'nothing'"):
        P.viewer_frame(outputs, "nothing")
    with pytest.raises(ValueError, match="split_output_render 'tall' is 6 x 5"):
        P.viewer_frame(outputs, "rgb", split_output_render="tall")
    with pytest.raises(ValueError, match=r"outputs\['tall'\] has 6 rows"):
        P.render_frame(outputs, ["rgb", "tall"])
    with pytest.raises(ValueError, match="9 panels: a frame holds at most 8"):
        P.render_frame(outputs, ["rgb"] * 9)
    with pytest.raises(KeyError, match="could not find 'normals'"):
        P.render_frame(outputs, ["rgb", "normals"])
    with pytest.raises(ValueError, match=r"out must be contiguous torch.uint8 \[4, 10, 3\]"):
        P.render_frame(outputs, ["rgb", "depth"], out=torch.zeros(4, 5, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"a table must be \[256, 3\]"):
        P.register_colormap("short", np.zeros((10, 3)))
    with pytest.raises(ValueError, match=r"tensor must be contiguous float32 \[256, 3\]"):
        P.colormap_table(torch.zeros(256, 4), "cpu")
    with pytest.raises(ValueError, match=r"depth must be float32 \[H, W, 1\]"):
        P.viewer_depth(torch.zeros(4, 5), "high")
    # past every check: only the device is missing
    with pytest.raises(RuntimeError, match="HIP device"):
        P.render_frame(outputs, ["rgb", "depth"])
    with pytest.raises(RuntimeError, match="HIP device"):
        P.viewer_depth(torch.zeros(4, 5, 1), "high")
    o = P.ColormapOptions()
    assert (o.colormap, o.normalize, o.colormap_min, o.colormap_max, o.invert) == ("default", False, 0.0, 1.0, False)


def test_named_tables_are_the_golden_ones():
    """matplotlib's listed colormaps, where it is installed, are the tables of tests/golden/colormap_luts.npz; "default" is turbo"""
    golden = R.tables()
    assert sorted(golden) == ["cividis", "inferno", "magma", "plasma", "turbo", "viridis"]
    for name, table in golden.items():
        P._TABLES.pop(name, None)
        assert np.array_equal(P._host_table(name), table) and table.dtype == np.float32 and table.shape == (256, 3)
    a, b = P.colormap_table("default", "cpu"), P.colormap_table("turbo", "cpu")
    assert a is b and P.colormap_table("gray", "cpu") is None
    with pytest.raises(ValueError, match="no listed colormap"):
        P.colormap_table("no_such_map", "cpu")


# ---- the C entry points' host checks ---------------------------------------------------------------------------------------------------
def test_host_side_argument_checks(hip_lib):
    """Every refusal happens before a launch and names the argument (the pointers are never followed: no device is needed)."""
    err = lambda: hip_lib.mtgs_rast_last_error().decode()
    buf = (C.c_int64 * 64)()
    a = C.addressof(buf)

    def table(n=1, **fields):
        t = np.zeros(n, dtype=P._PANEL)
        t["src"], t["kind"], t["src_h"], t["src_w"], t["h"], t["w"] = a, 1, 4, 6, 4, 6
        t["near_plane"], t["far_plane"], t["colormap_max"] = 0.0, 1.0, 1.0
        for k, v in fields.items():
            t[k][-1] = v
        return t

    color = (C.c_float * 3)(*P.SPLIT_COLOR)

    def compose(t, n=None, out_h=4, out_w=6, split=-1, col=color, fmt=0, out=a, ws=a, ws_bytes=1 << 14):
        return hip_lib.mtgs_present_compose(len(t) if n is None else n, t.ctypes.data_as(C.c_void_p), out_h, out_w, split, col, fmt, out, ws,
                                            ws_bytes, None)

    assert compose(table(), n=0) == 1 and "n_panels outside [1, 8] (0)" in err()
    assert compose(table(9)) == 1 and "n_panels outside [1, 8] (9)" in err()
    assert hip_lib.mtgs_present_compose(1, None, 4, 6, -1, color, 0, a, a, 1 << 14, None) == 1 and "null pointer: panels" in err()
    assert compose(table(), out_h=-1) == 1 and "out_h, out_w" in err()
    assert compose(table(), out_h=1 << 16, out_w=1 << 15) == 1 and "out_h * out_w < 2^31" in err()
    assert compose(table(), fmt=3) == 1 and "format outside [0, 2] (3)" in err()
    assert compose(table(), split=6) == 1 and "split_column outside [-1, out_w) (6)" in err()
    assert compose(table(), split=2, col=None) == 1 and "null pointer: split_color" in err()
    assert compose(table(), out=None) == 1 and "null pointer: out" in err()
    assert compose(table(), fmt=2, out=a + 2) == 1 and "float32 out must be 4-byte aligned" in err()
    assert compose(table(2, kind=4)) == 1 and "panels[1].kind outside [0, 3] (4)" in err()
    assert compose(table(2, src=0)) == 1 and "null pointer: panels[1].src" in err()
    assert compose(table(src=a + 1)) == 1 and "panels[0].src must be 4-byte aligned" in err()
    assert compose(table(lut=a + 2)) == 1 and "panels[0].accumulation and .lut must be 4-byte aligned" in err()
    assert compose(table(src_h=0)) == 1 and "src_h, src_w must be >= 1" in err()
    assert compose(table(w=-1)) == 1 and "panels[0]: negative rectangle" in err()
    assert compose(table(h=5)) == 1 and "rectangle reads outside its source (h 5 of 4 rows" in err()
    assert compose(table(src_x0=1)) == 1 and "columns [1, 7) of 6" in err()
    assert compose(table(x0=1)) == 1 and "rectangle outside the 4 x 6 frame" in err()
    assert compose(table(y0=1)) == 1 and "rectangle outside the 4 x 6 frame" in err()
    # a panel that takes its extrema from the data needs the workspace
    assert compose(table(normalize=1), ws=None) == 1 and "null pointer: ws" in err()
    assert compose(table(kind=2, near_plane=math.nan), ws_bytes=100) == 3 and "workspace 100 < 16384 bytes" in err()
    assert compose(table(kind=2, far_plane=math.nan), ws=a + 4) == 1 and "workspace must be 8-byte aligned" in err()
    assert compose(table(), out_h=0, out_w=0, out=None) == 1               # the rectangle no longer fits
    assert compose(table(h=0, w=0), out_h=0, out_w=0, out=None, ws=None) == 0     # an empty frame: a no-op

    stats = lambda t, ws=a, ws_bytes=1 << 14: hip_lib.mtgs_present_stats(len(t), t.ctypes.data_as(C.c_void_p), ws, ws_bytes, None)
    assert stats(table(), ws=None) == 0                                      # nothing to take from the data: nothing launched
    assert stats(table(kind=0, normalize=1), ws=None) == 0                  # normalize means nothing for an RGB panel
    assert stats(table(normalize=1), ws=None) == 1 and "null pointer: ws" in err()
    assert stats(table(normalize=1), ws_bytes=16383) == 3 and "workspace 16383 < 16384" in err()
    assert stats(table(9)) == 1 and "n_panels outside [1, 8] (9)" in err()

    resize = lambda ih=4, iw=6, src=a, oh=2, ow=3, dst=a: hip_lib.mtgs_present_depth_resize(ih, iw, src, oh, ow, 1.0, dst, None)
    assert resize(src=None) == 1 and "null pointer: src" in err()
    assert resize(dst=None) == 1 and "null pointer: dst" in err()
    assert resize(ih=-1) == 1 and "in_h, in_w" in err()
    assert resize(oh=1 << 16, ow=1 << 15) == 1 and "out_h * out_w < 2^31" in err()
    assert resize(ih=0) == 1 and "an empty source" in err()
    assert resize(oh=0, src=None, dst=None) == 0                             # nothing to write
