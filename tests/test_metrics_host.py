"""Image metrics (mtgs_amd/metrics.py, csrc/metrics.hip) without a GPU: the C entry points are declared, bound and exported,
refuse bad arguments on the host by name, take P = 0 as a no-op, and the Python layer refuses CPU tensors and images that do
not have three channels."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

METRICS = ("mtgs_metrics_workspace_bytes", "mtgs_color_correct", "mtgs_image_metrics")
EPS = 0.5 / 255


def test_metrics_symbols_declared_bound_and_exported(hip_lib):
    from mtgs_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", (Path(__file__).resolve().parents[1] / "include" / "mtgs_rast.h").read_text(), flags=re.S)
    syms = set(re.findall(r"\b(mtgs_[a-z0-9_]+)\s*\(", text))
    for name in METRICS:
        assert name in syms, name
        assert name in _lib.EXPORTS, name
        assert hasattr(hip_lib, name), name
    abi, hot = (int(re.search(r"#define %s (\d+)" % macro, text).group(1)) for macro in ("MTGS_RAST_ABI_VERSION", "MTGS_RAST_HOT_ABI_VERSION"))
    assert hip_lib.mtgs_rast_version() == abi and hip_lib.mtgs_rast_hot_version() == hot
    import mtgs_amd
    assert mtgs_amd.color_correct is mtgs_amd.metrics.color_correct
    assert mtgs_amd.image_metrics is mtgs_amd.metrics.image_metrics


def _ws(lib, P, iters):
    n = C.c_size_t(0)
    assert lib.mtgs_metrics_workspace_bytes(P, iters, C.byref(n)) == 0
    return n.value


def test_metrics_host_validation_names_the_bad_argument(hip_lib):
    big = 1 << 30
    assert hip_lib.mtgs_color_correct(10, 5, EPS, None, 1, None, 1, 1, big, None) == 1
    assert b"img" in hip_lib.mtgs_rast_last_error()
    assert hip_lib.mtgs_color_correct(10, 5, EPS, 1, None, None, 1, 1, big, None) == 1
    assert b"ref" in hip_lib.mtgs_rast_last_error()
    assert hip_lib.mtgs_color_correct(10, 5, EPS, 1, 1, None, None, 1, big, None) == 1
    assert b"out" in hip_lib.mtgs_rast_last_error()
    assert hip_lib.mtgs_color_correct(10, 5, EPS, 1, 1, None, 1, None, big, None) == 1
    assert b"ws" in hip_lib.mtgs_rast_last_error()
    assert hip_lib.mtgs_color_correct(10, -1, EPS, 1, 1, None, 1, 1, big, None) == 1
    assert b"num_iters" in hip_lib.mtgs_rast_last_error()
    assert hip_lib.mtgs_color_correct(10, 5, EPS, 1, 1, None, 1, 1, _ws(hip_lib, 10, 5) - 8, None) == 3
    assert b"workspace" in hip_lib.mtgs_rast_last_error()
    assert hip_lib.mtgs_image_metrics(10, 5, EPS, None, 1, None, None, None, 1, 1, big, None) == 1
    assert b"pred" in hip_lib.mtgs_rast_last_error()
    assert hip_lib.mtgs_image_metrics(10, 5, EPS, 1, None, None, None, None, 1, 1, big, None) == 1
    assert b"gt" in hip_lib.mtgs_rast_last_error()
    assert hip_lib.mtgs_image_metrics(10, 5, EPS, 1, 1, None, None, None, None, 1, big, None) == 1
    assert b"metrics" in hip_lib.mtgs_rast_last_error()
    assert hip_lib.mtgs_image_metrics(10, 5, EPS, 1, 1, None, 1, None, 1, 1, big, None) == 1
    assert b"lidar_depth" in hip_lib.mtgs_rast_last_error()
    assert hip_lib.mtgs_image_metrics(10, -2, EPS, 1, 1, None, None, None, 1, 1, big, None) == 1
    assert b"num_iters" in hip_lib.mtgs_rast_last_error()
    assert hip_lib.mtgs_metrics_workspace_bytes(10, 5, None) == 1
    assert hip_lib.mtgs_metrics_workspace_bytes(10, -1, C.byref(C.c_size_t(0))) == 1


def test_metrics_zero_pixels_is_a_noop(hip_lib):
    # no pointer is touched and nothing is launched (no device on this machine)
    assert hip_lib.mtgs_color_correct(0, 5, EPS, None, None, None, None, None, 0, None) == 0
    assert hip_lib.mtgs_image_metrics(0, 5, EPS, None, None, None, None, None, None, None, 0, None) == 0
    # the workspace grows with the iterations (one warp per fit) and is positive for any P
    assert 0 < _ws(hip_lib, 0, 0) < _ws(hip_lib, 0, 5) <= _ws(hip_lib, 1 << 21, 5)


def test_metrics_python_refuses_cpu_tensors_and_other_channel_counts():
    from mtgs_amd import color_correct, image_metrics
    img = torch.rand(8, 8, 3)
    with pytest.raises(RuntimeError, match="HIP device"):
        color_correct(img, img)
    with pytest.raises(RuntimeError, match="HIP device"):
        image_metrics(img, img)
    # the channel count is checked first and named
    four = torch.rand(8, 8, 4)
    with pytest.raises(NotImplementedError, match="4 channels"):
        color_correct(four, four)
    with pytest.raises(NotImplementedError, match="1 channels"):
        image_metrics(four[..., :1], four[..., :1])
    with pytest.raises(ValueError, match="num_iters"):
        color_correct(img, img, num_iters=-1)
