"""ctypes binding of libmtgs_rast.so (include/mtgs_rast.h).

The product path has NO fallback: if the HIP library is missing or a call fails, an exception is
raised.  Nothing here (or anywhere under mtgs_amd/) touches oracle/.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import torch

from . import _abi

_PKG = Path(__file__).resolve().parent
LIB_PATH = _PKG / "libmtgs_rast.so"


def use_library(path) -> None:
    """Development only (scripts/kbench.py --lib, A/B builds of scripts/build_variant.py): load another build of the
    library instead of the in-tree one.  Must be called before the first load(); nothing in the product reads the
    environment for this."""
    global LIB_PATH
    if _lib is not None:
        raise RuntimeError("use_library() after the library was loaded")
    LIB_PATH = Path(path)

# include/mtgs_rast.h and the headers it includes are the description of the ABI: argument and result types of every entry point are
# read from their prototypes.  One group per header, the main header's own declarations first
_PROTOTYPES = {_abi.HEADER.name: _abi.prototypes()}
for _name in _abi.included_headers():
    _PROTOTYPES[_name] = _abi.header_abi(_name).prototypes
GROUPS = {header: list(group) for header, group in _PROTOTYPES.items()}       # header name -> its entry points
EXPORTS = GROUPS[_abi.HEADER.name]
ABI_VERSION = _abi.constant("MTGS_RAST_ABI_VERSION")
HOT_ABI_VERSION = _abi.constant("MTGS_RAST_HOT_ABI_VERSION")      # hot-path subset: what profiles/rNN_pmc_step.json is keyed on

_lib = None


def load() -> C.CDLL:
    """Loads the library (does not initialise the GPU).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -m mtgs_amd.build` (needs hipcc). "
            "mtgs_amd has no CPU or PyTorch fallback for the rasterizer.")
    lib = C.CDLL(str(LIB_PATH))
    for group in _PROTOTYPES.values():
        for name, (restype, argtypes) in group.items():
            fn = getattr(lib, name)
            fn.argtypes = argtypes
            fn.restype = restype
    v = lib.mtgs_rast_version()
    if v != ABI_VERSION:
        raise RuntimeError(f"libmtgs_rast.so ABI version {v} != expected {ABI_VERSION}; rebuild")
    if lib.mtgs_rast_hot_version() != HOT_ABI_VERSION:
        raise RuntimeError(f"libmtgs_rast.so hot-path ABI version {lib.mtgs_rast_hot_version()} != expected {HOT_ABI_VERSION}; rebuild")
    _lib = lib
    return lib


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def host_i64(values):
    """HOST int64 array argument (None -> NULL)."""
    return None if values is None else (C.c_int64 * len(values))(*values)


def stream_of(t: torch.Tensor):
    return torch.cuda.current_stream(t.device).cuda_stream


_timed: dict = {}  # entry-point name -> list of (start_event, end_event); filled when enabled


def time_calls(names=()) -> None:
    """Bracket every call of the named entry points with HIP events on the current stream (the
    stream the kernels are launched on).  `time_calls(())` disables.  Used by bench.py only."""
    _timed.clear()
    for n in names:
        _timed[n] = []


def timed_ms() -> dict:
    """name -> list of elapsed milliseconds (call torch.cuda.synchronize() first)."""
    return {n: [s.elapsed_time(e) for s, e in evs] for n, evs in _timed.items()}


def call(name: str, *args) -> None:
    evs = _timed.get(name) if _timed else None
    if evs is not None:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
    rc = getattr(load(), name)(*args)
    if evs is not None:
        e.record()
        evs.append((s, e))
    if rc != 0:
        msg = load().mtgs_rast_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{name} failed (code {rc}): {msg}")


def size_query(name: str, *dims) -> int:
    """What the size query `name` (a *_bytes / *_floats entry point) reports for `dims`."""
    n = C.c_size_t(0)
    call(name, *dims, C.byref(n))
    return n.value


def workspace(name: str, *dims, device, dtype, pad: int = 0) -> torch.Tensor:
    """The scratch tensor whose element count the size query `name` reports for `dims`: dtype torch.float32 for the
    *_workspace_floats entry points, torch.uint8 for the *_workspace_bytes ones.  `pad` more elements for a caller that
    aligns the pointer itself."""
    return torch.empty(size_query(name, *dims) + pad, dtype=dtype, device=device)


_scratch: dict = {}     # (device, stream) + key -> uint8 tensor


def scratch(key: tuple, nbytes, device, stream) -> torch.Tensor:
    """The cached uint8 scratch tensor of one operator on one stream: allocated on the first call with (device, stream) + key and
    returned again after that, so that a repeated call allocates nothing and two streams never share a buffer.  `nbytes` is a
    number or a callable that returns it (a size query, made on a miss only)."""
    key = (device, stream) + key
    ws = _scratch.get(key)
    if ws is None:
        ws = _scratch[key] = torch.empty(nbytes() if callable(nbytes) else nbytes, dtype=torch.uint8, device=device)
    return ws


def require_gpu(*tensors) -> None:
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                "mtgs_amd: tensors must live on the HIP device (torch device 'cuda'); got "
                f"{t.device}. There is no CPU fallback in the product path.")
