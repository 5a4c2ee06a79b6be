"""WildGaussians appearance colours (mtgs_amd/appearance.py, csrc/wild.hip) without a GPU: the C entry points are declared,
bound and exported, refuse bad arguments on the host by name, take n = 0 as a no-op, and the Python layer refuses CPU tensors
and MLPs of another shape."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

WILD = ("mtgs_wild_workspace_bytes", "mtgs_wild_fwd", "mtgs_wild_bwd", "mtgs_wild_reduce")
W = (27, 32, 128, 6)     # the widths the kernels take


def _mlp(h1=128, h2=128, d_in=59, d_out=6):
    return torch.nn.Sequential(torch.nn.Linear(d_in, h1), torch.nn.ReLU(), torch.nn.Linear(h1, h2), torch.nn.ReLU(),
                               torch.nn.Linear(h2, d_out))


def _fwd(lib, n, dc=None, rest=None, w=(1, 1, 1, 1, 1, 1), out=1, widths=W):
    return lib.mtgs_wild_fwd(n, None, None, None, dc, 3, rest, 45, None, *w, *widths, out, 3, None)


def _bwd(lib, n, grad=1, ws=1 << 30, widths=W):
    return lib.mtgs_wild_bwd(n, None, None, grad, 3, 1, 3, 1, 45, None, 1, 1, 1, 1, 1, 1, *widths, 1, 1, 45, 1, ws, None)


def test_wild_symbols_declared_bound_and_exported(hip_lib):
    from mtgs_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", (Path(__file__).resolve().parents[1] / "include" / "mtgs_rast.h").read_text(), flags=re.S)
    syms = set(re.findall(r"\b(mtgs_[a-z0-9_]+)\s*\(", text))
    for name in WILD:
        assert name in syms, name
        assert name in _lib.EXPORTS, name
        assert hasattr(hip_lib, name), name
    abi, hot = (int(re.search(r"#define %s (\d+)" % macro, text).group(1)) for macro in ("MTGS_RAST_ABI_VERSION", "MTGS_RAST_HOT_ABI_VERSION"))
    assert hip_lib.mtgs_rast_version() == abi and hip_lib.mtgs_rast_hot_version() == hot


def test_wild_host_validation_names_the_null_pointer(hip_lib):
    assert _fwd(hip_lib, 10, dc=None, rest=1) == 1
    assert b"features_dc" in hip_lib.mtgs_rast_last_error()
    assert _fwd(hip_lib, 10, dc=1, rest=None) == 1
    assert b"features_rest" in hip_lib.mtgs_rast_last_error()
    assert _fwd(hip_lib, 10, dc=1, rest=1, w=(1, 1, None, 1, 1, 1)) == 1
    assert b"w2" in hip_lib.mtgs_rast_last_error()
    assert _fwd(hip_lib, 10, dc=1, rest=1, out=None) == 1
    assert b"out" in hip_lib.mtgs_rast_last_error()
    # vis_ids without the device count
    assert hip_lib.mtgs_wild_fwd(10, 1, None, None, 1, 3, 1, 45, None, 1, 1, 1, 1, 1, 1, *W, 1, 16, None) == 1
    assert b"totals" in hip_lib.mtgs_rast_last_error()
    assert _bwd(hip_lib, 10, grad=None) == 1
    assert b"grad" in hip_lib.mtgs_rast_last_error()
    assert hip_lib.mtgs_wild_bwd(10, None, None, 1, 3, 1, 3, 1, 45, None, 1, 1, 1, 1, 1, 1, *W, 1, 1, 45, None, 1 << 30, None) == 1
    assert b"partials" in hip_lib.mtgs_rast_last_error()
    assert _bwd(hip_lib, 10, ws=16) == 3          # workspace too small
    assert hip_lib.mtgs_wild_reduce(10, None, None, 1, *W, 1, 1, 1, 1, 1, 1, None, None) == 1
    assert b"partials" in hip_lib.mtgs_rast_last_error()
    assert hip_lib.mtgs_wild_workspace_bytes(10, None) == 1


@pytest.mark.parametrize("widths", [(27, 32, 64, 6), (27, 16, 128, 6), (24, 32, 128, 6), (27, 32, 128, 3)])
def test_wild_other_widths_unsupported(hip_lib, widths):
    assert _fwd(hip_lib, 10, dc=1, rest=1, widths=widths) == 4
    assert b"27+32 -> 128 -> 128 -> 6" in hip_lib.mtgs_rast_last_error()
    assert _bwd(hip_lib, 10, widths=widths) == 4
    assert hip_lib.mtgs_wild_reduce(10, 1, None, 1, *widths, 1, 1, 1, 1, 1, 1, None, None) == 4


def test_wild_empty_is_a_no_op(hip_lib):
    n = C.c_size_t(7)
    assert hip_lib.mtgs_wild_workspace_bytes(0, C.byref(n)) == 0 and n.value == 0
    assert hip_lib.mtgs_wild_workspace_bytes(1000, C.byref(n)) == 0 and n.value > 0
    assert _fwd(hip_lib, 0, dc=None, rest=None, w=(None,) * 6, out=None) == 0
    assert hip_lib.mtgs_wild_bwd(0, None, None, None, 3, None, 3, None, 45, None, *(None,) * 6, *W, None, None, 45, None, 0, None) == 0
    assert hip_lib.mtgs_wild_reduce(0, None, None, None, *W, *(None,) * 7, None) == 0


def _inputs(N=5, dev="cpu"):
    g = torch.Generator().manual_seed(0)
    return (torch.randn(N, 3, generator=g).to(dev), torch.randn(N, 15, 3, generator=g).to(dev), torch.randn(32, generator=g).to(dev))


def test_wild_colors_refuses_cpu_tensors():
    from mtgs_amd import wild_color_source, wild_colors
    dc, rest, e = _inputs()
    with pytest.raises(RuntimeError, match="HIP device"):
        wild_colors(dc, rest, e, _mlp())
    with pytest.raises(RuntimeError, match="HIP device"):
        wild_color_source(dc, rest, None, _mlp())


@pytest.mark.parametrize("mlp, shape", [(_mlp(h1=64), "(64, 59)"), (_mlp(h2=96), "(128, 128)"), (_mlp(d_in=60), "(128, 60)"),
                                        (_mlp(d_out=3), "(3, 128)")])
def test_wild_colors_refuses_other_mlp_shapes(mlp, shape):
    from mtgs_amd import wild_colors
    dc, rest, e = _inputs()
    with pytest.raises(NotImplementedError, match=shape.replace("(", r"\(").replace(")", r"\)")):
        wild_colors(dc, rest, e, mlp)


def test_wild_colors_refuses_other_layouts():
    from mtgs_amd import wild_colors
    dc, rest, e = _inputs()
    with pytest.raises(NotImplementedError, match="Sequential"):
        wild_colors(dc, rest, e, torch.nn.Sequential(torch.nn.Linear(59, 128), torch.nn.Linear(128, 6)))
    with pytest.raises(NotImplementedError, match=r"embedding of shape \(16,\)"):
        wild_colors(dc, rest, e[:16], _mlp())
    with pytest.raises(NotImplementedError, match=r"features_rest of shape \(5, 4, 3\)"):
        wild_colors(dc, rest[:, :4], e, _mlp())
    with pytest.raises(NotImplementedError, match="six tensors"):
        wild_colors(dc, rest, e, [torch.zeros(128, 59)])


def test_wild_exported_from_the_package():
    import mtgs_amd
    from mtgs_amd import appearance
    assert "wild_colors" in mtgs_amd.__all__ and "wild_color_source" in mtgs_amd.__all__
    assert mtgs_amd.wild_colors is appearance.wild_colors and "appearance" in mtgs_amd.__doc__
