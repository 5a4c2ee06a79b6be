"""Geometric loss terms (mtgs_amd/loss.py: normals_from_depth, depth_normal_loss, scale_regularizers; csrc/geomloss.hip)
without a GPU: the C entry points are declared, bound and exported, the ABI versions are unchanged, bad arguments are refused
on the host by name, and the Python layer refuses CPU tensors."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

GEOM = ("mtgs_depth_normals", "mtgs_depth_normal_loss_workspace_floats", "mtgs_depth_normal_loss_fwd",
        "mtgs_depth_normal_loss_bwd", "mtgs_scale_reg_workspace_floats", "mtgs_scale_reg_fwd", "mtgs_scale_reg_bwd")


def _err(lib):
    return lib.mtgs_rast_last_error()


def test_geom_loss_symbols_declared_bound_and_exported(hip_lib):
    from mtgs_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", (Path(__file__).resolve().parents[1] / "include" / "mtgs_rast.h").read_text(), flags=re.S)
    syms = set(re.findall(r"\b(mtgs_[a-z0-9_]+)\s*\(", text))
    for name in GEOM:
        assert name in syms, name
        assert name in _lib.EXPORTS, name
        assert hasattr(hip_lib, name), name
    abi, hot = (int(re.search(r"#define %s (\d+)" % macro, text).group(1)) for macro in ("MTGS_RAST_ABI_VERSION", "MTGS_RAST_HOT_ABI_VERSION"))
    assert hip_lib.mtgs_rast_version() == abi and hip_lib.mtgs_rast_hot_version() == hot
    assert _lib.ABI_VERSION == abi and _lib.HOT_ABI_VERSION == hot


def test_depth_normals_validation_names_the_bad_argument(hip_lib):
    assert hip_lib.mtgs_depth_normals(0, 4, 1, 1, 1, None) == 1 and b"width" in _err(hip_lib)
    assert hip_lib.mtgs_depth_normals(4, -1, 1, 1, 1, None) == 1 and b"height" in _err(hip_lib)
    assert hip_lib.mtgs_depth_normals(4, 4, None, 1, 1, None) == 1 and b"depth is NULL" in _err(hip_lib)
    assert hip_lib.mtgs_depth_normals(4, 4, 1, None, 1, None) == 1 and b"K is NULL" in _err(hip_lib)
    assert hip_lib.mtgs_depth_normals(4, 4, 1, 1, None, None) == 1 and b"out is NULL" in _err(hip_lib)


def test_depth_normal_loss_validation_names_the_bad_argument(hip_lib):
    fwd, bwd = hip_lib.mtgs_depth_normal_loss_fwd, hip_lib.mtgs_depth_normal_loss_bwd
    assert fwd(0, 4, 1, 1, 1, None, 0.1, 50.0, 1, 1, 1, None) == 1 and b"width" in _err(hip_lib)
    assert fwd(4, 0, 1, 1, 1, None, 0.1, 50.0, 1, 1, 1, None) == 1 and b"height" in _err(hip_lib)
    assert fwd(4, 4, None, 1, 1, None, 0.1, 50.0, 1, 1, 1, None) == 1 and b"pred is NULL" in _err(hip_lib)
    assert fwd(4, 4, 1, None, 1, None, 0.1, 50.0, 1, 1, 1, None) == 1 and b"depth is NULL" in _err(hip_lib)
    assert fwd(4, 4, 1, 1, None, None, 0.1, 50.0, 1, 1, 1, None) == 1 and b"K is NULL" in _err(hip_lib)
    assert fwd(4, 4, 1, 1, 1, None, 0.1, 50.0, 1, None, 1, None) == 1 and b"partials is NULL" in _err(hip_lib)
    assert fwd(4, 4, 1, 1, 1, None, 0.1, 50.0, 1, 1, None, None) == 1 and b"out is NULL" in _err(hip_lib)
    assert b"mtgs_depth_normal_loss_fwd" in _err(hip_lib)
    assert bwd(4, 4, None, 1, 1, None, 0.1, 50.0, 1, 1, 1, 1, None) == 1 and b"pred is NULL" in _err(hip_lib)
    assert b"mtgs_depth_normal_loss_bwd" in _err(hip_lib)
    assert bwd(4, 4, 1, 1, 1, None, 0.1, 50.0, 1, None, 1, 1, None) == 1 and b"v_out is NULL" in _err(hip_lib)
    assert bwd(4, 4, 1, 1, 1, None, 0.1, 50.0, 1, 1, None, 1, None) == 1 and b"out is NULL" in _err(hip_lib)
    assert bwd(4, 4, 1, 1, 1, None, 0.1, 50.0, 1, 1, 1, None, None) == 1 and b"v_pred is NULL" in _err(hip_lib)


def test_scale_reg_validation_names_the_bad_argument(hip_lib):
    fwd, bwd = hip_lib.mtgs_scale_reg_fwd, hip_lib.mtgs_scale_reg_bwd
    assert fwd(-1, 1, 1, 10.0, 1, 1, None) == 1 and b"n must be" in _err(hip_lib)
    assert fwd(8, None, 1, 10.0, 1, 1, None) == 1 and b"scales is NULL" in _err(hip_lib)
    assert fwd(8, 1, 1, float("inf"), 1, 1, None) == 1 and b"max_ratio" in _err(hip_lib)
    assert fwd(8, 1, 1, float("nan"), 1, 1, None) == 1 and b"max_ratio" in _err(hip_lib)
    assert fwd(8, 1, 1, 10.0, None, 1, None) == 1 and b"partials is NULL" in _err(hip_lib)
    assert fwd(8, 1, 1, 10.0, 1, None, None) == 1 and b"out is NULL" in _err(hip_lib)
    assert bwd(-1, 1, 1, 10.0, 1, 1, None) == 1 and b"n must be" in _err(hip_lib)
    assert bwd(8, None, 1, 10.0, 1, 1, None) == 1 and b"scales is NULL" in _err(hip_lib)
    assert bwd(8, 1, 1, 10.0, None, 1, None) == 1 and b"v_out is NULL" in _err(hip_lib)
    assert bwd(8, 1, 1, 10.0, 1, None, None) == 1 and b"v_scales is NULL" in _err(hip_lib)
    # no rows: the backward has nothing to write (nothing is launched: no device on this machine)
    assert bwd(0, None, 1, 10.0, None, None, None) == 0


def test_geom_loss_workspace_sizes(hip_lib):
    n = C.c_size_t(0)
    assert hip_lib.mtgs_depth_normal_loss_workspace_floats(960, 540, C.byref(n)) == 0
    assert n.value == -(-960 * 540 // 256) * 4          # four partial sums per 256-pixel block
    assert hip_lib.mtgs_depth_normal_loss_workspace_floats(0, 540, C.byref(n)) == 1 and b"width and height" in _err(hip_lib)
    assert hip_lib.mtgs_depth_normal_loss_workspace_floats(960, 540, None) == 1
    assert hip_lib.mtgs_scale_reg_workspace_floats(1 << 21, C.byref(n)) == 0 and n.value == (1 << 21) // 256 * 2
    assert hip_lib.mtgs_scale_reg_workspace_floats(0, C.byref(n)) == 0 and n.value == 2      # never an empty workspace
    assert hip_lib.mtgs_scale_reg_workspace_floats(-5, C.byref(n)) == 1 and b"n must be" in _err(hip_lib)


def test_geom_loss_python_refuses_cpu_tensors_and_bad_shapes():
    from mtgs_amd.loss import depth_normal_loss, normals_from_depth, scale_regularizers
    depth = torch.rand(6, 8, 1) * 10
    K = torch.eye(3)
    pred = torch.rand(6, 8, 3, requires_grad=True)
    with pytest.raises(RuntimeError, match="HIP device"):
        normals_from_depth(depth, K)
    with pytest.raises(RuntimeError, match="HIP device"):
        depth_normal_loss(pred, depth, K)
    with pytest.raises(RuntimeError, match="HIP device"):
        scale_regularizers(torch.rand(10, 3, requires_grad=True))
    with pytest.raises(NotImplementedError, match="gt_depth"):
        depth_normal_loss(pred, depth.clone().requires_grad_(True), K)
    with pytest.raises(AssertionError):
        depth_normal_loss(torch.rand(6, 8, 4), depth, K)        # three channels
    with pytest.raises(AssertionError):
        depth_normal_loss(pred, torch.rand(8, 6, 1), K)          # depth of another size
    with pytest.raises(AssertionError):
        normals_from_depth(depth, torch.eye(4))                   # K is 3x3
    with pytest.raises(AssertionError):
        scale_regularizers(torch.rand(10, 2))
