"""The pseudo-depth loss entry points (csrc/depthloss.hip; mtgs_amd.loss.pseudo_depth_loss) without a GPU: declared, bound and
exported, the ABI versions unchanged (an additive block), bad arguments refused on the host by name, the workspace sized by
the launch cap."""
import ctypes as C
import re
from pathlib import Path

DEPTH = ("mtgs_depth_loss_workspace_floats", "mtgs_depth_loss_fwd", "mtgs_depth_loss_bwd")
HEADER = Path(__file__).resolve().parents[1] / "include" / "mtgs_rast.h"


def _err(lib):
    return lib.mtgs_rast_last_error()


def test_depth_loss_symbols_declared_bound_and_exported(hip_lib):
    from mtgs_amd import _lib, loss
    text = HEADER.read_text()
    syms = set(re.findall(r"\b(mtgs_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    for name in DEPTH:
        assert name in syms, name
        assert name in _lib.EXPORTS, name
        assert hasattr(hip_lib, name), name
    assert hip_lib.mtgs_rast_version() == _lib.ABI_VERSION and hip_lib.mtgs_rast_hot_version() == _lib.HOT_ABI_VERSION
    # the kind numbers and the record length of the Python layer are the header's
    macros = dict(re.findall(r"#define MTGS_DEPTH_LOSS_([A-Z0-9_]+) (\d+)", text))
    names = {"mse": "MSE", "L1": "L1", "InverseL1": "INVERSE_L1", "LogL1": "LOG_L1", "HuberL1": "HUBER_L1",
             "EdgeAwareLogL1": "EDGE_AWARE_LOG_L1"}
    assert {k: int(macros[v]) for k, v in names.items()} == loss._DEPTH_LOSS_KINDS
    assert int(macros["RECORD_FLOATS"]) == loss._DEPTH_LOSS_RECORD


def test_depth_loss_validation_names_the_bad_argument(hip_lib):
    fwd, bwd = hip_lib.mtgs_depth_loss_fwd, hip_lib.mtgs_depth_loss_bwd
    assert fwd(6, 4, 4, 1, 1, None, 1, 0.1, 50.0, 0.2, 1, 1, None) == 1 and b"kind" in _err(hip_lib)
    assert fwd(-1, 4, 4, 1, 1, None, 1, 0.1, 50.0, 0.2, 1, 1, None) == 1 and b"kind" in _err(hip_lib)
    assert fwd(1, 0, 4, 1, 1, None, None, 0.1, 50.0, 0.2, 1, 1, None) == 1 and b"width" in _err(hip_lib)
    assert fwd(1, 4, 0, 1, 1, None, None, 0.1, 50.0, 0.2, 1, 1, None) == 1 and b"height" in _err(hip_lib)
    assert fwd(1, 4, 4, None, 1, None, None, 0.1, 50.0, 0.2, 1, 1, None) == 1 and b"pred is NULL" in _err(hip_lib)
    assert fwd(1, 4, 4, 1, None, None, None, 0.1, 50.0, 0.2, 1, 1, None) == 1 and b"gt is NULL" in _err(hip_lib)
    assert fwd(5, 4, 4, 1, 1, None, None, 0.1, 50.0, 0.2, 1, 1, None) == 1 and b"rgb is NULL" in _err(hip_lib)
    assert fwd(1, 4, 4, 1, 1, None, None, float("nan"), 50.0, 0.2, 1, 1, None) == 1 and b"lo and hi" in _err(hip_lib)
    assert fwd(4, 4, 4, 1, 1, None, None, 0.1, 50.0, 0.0, 1, 1, None) == 1 and b"huber_thresh" in _err(hip_lib)
    assert fwd(4, 4, 4, 1, 1, None, None, 0.1, 50.0, float("inf"), 1, 1, None) == 1 and b"huber_thresh" in _err(hip_lib)
    assert fwd(1, 4, 4, 1, 1, None, None, 0.1, 50.0, 0.2, None, 1, None) == 1 and b"partials is NULL" in _err(hip_lib)
    assert fwd(1, 4, 4, 1, 1, None, None, 0.1, 50.0, 0.2, 1, None, None) == 1 and b"out is NULL" in _err(hip_lib)
    assert b"mtgs_depth_loss_fwd" in _err(hip_lib)
    assert bwd(9, 4, 4, 1, 1, None, None, 0.1, 50.0, 0.2, 1, 1, 1, None) == 1 and b"kind" in _err(hip_lib)
    assert bwd(1, 4, 4, None, 1, None, None, 0.1, 50.0, 0.2, 1, 1, 1, None) == 1 and b"pred is NULL" in _err(hip_lib)
    assert b"mtgs_depth_loss_bwd" in _err(hip_lib)
    assert bwd(5, 4, 4, 1, 1, None, None, 0.1, 50.0, 0.2, 1, 1, 1, None) == 1 and b"rgb is NULL" in _err(hip_lib)
    assert bwd(1, 4, 4, 1, 1, None, None, 0.1, 50.0, 0.2, None, 1, 1, None) == 1 and b"v_out is NULL" in _err(hip_lib)
    assert bwd(1, 4, 4, 1, 1, None, None, 0.1, 50.0, 0.2, 1, None, 1, None) == 1 and b"out is NULL" in _err(hip_lib)
    assert bwd(1, 4, 4, 1, 1, None, None, 0.1, 50.0, 0.2, 1, 1, None, None) == 1 and b"v_pred is NULL" in _err(hip_lib)


def test_depth_loss_workspace_is_capped(hip_lib):
    n = C.c_size_t(0)
    assert hip_lib.mtgs_depth_loss_workspace_floats(16, 16, C.byref(n)) == 0 and n.value == 5          # one 256-pixel block
    assert hip_lib.mtgs_depth_loss_workspace_floats(257, 1, C.byref(n)) == 0 and n.value == 2 * 5
    assert hip_lib.mtgs_depth_loss_workspace_floats(512, 512, C.byref(n)) == 0 and n.value == 1024 * 5   # exactly the cap
    assert hip_lib.mtgs_depth_loss_workspace_floats(1920, 1080, C.byref(n)) == 0 and n.value == 1024 * 5  # the passes stride
    assert hip_lib.mtgs_depth_loss_workspace_floats(0, 540, C.byref(n)) == 1 and b"width and height" in _err(hip_lib)
    assert hip_lib.mtgs_depth_loss_workspace_floats(960, 540, None) == 1
