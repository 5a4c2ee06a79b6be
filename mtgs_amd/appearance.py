"""WildGaussians appearance colours (MTGS config/WildGaussians.py, use_wild_gaussians=True) on the HIP device.

MTGS colours every Gaussian with a small appearance network (mtgs_scene_graph.py:308-318 builds it, :623-632 evaluates it):

    rgb    = clamp(features_dc * C0 + 0.5, 0, 1)
    x      = [rgb | features_rest.view(N, -1)[:, :24] | e]          e = camera embedding [32], or zeros
    y      = 0.01 * L3(relu(L2(relu(L1(x)))))                      L1: 59 -> 128, L2: 128 -> 128, L3: 128 -> 6
    colour = rgb * (1 + y[:, 3:6]) + y[:, :3]

Two forms, both csrc/wild.hip (exact-f32 MFMA, weight gradients reduced in a fixed order: bitwise reproducible):

    wild_colors(features_dc, features_rest, embedding, mlp) -> [N, 3]        an autograd op over all N
    wild_color_source(features_dc, features_rest, embedding, mlp)           rasterization(colors=None | [N, DX], color_source=src):
                                                                             the colours of the VISIBLE Gaussians only, straight
                                                                             into their packed records (touch_first: only those the
                                                                             frame composites from); gradients reach every input
                                                                             through loss.backward(), dense.

`mlp` is the reference-shaped nn.Sequential(Linear(59, 128), ReLU, Linear(128, 128), ReLU, Linear(128, 6)) or its six tensors
(w1, b1, w2, b2, w3, b3).  `embedding` is [32], [1, 32] or None.  There is no CPU path.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from . import wrapper
from ._lib import ptr, require_gpu, stream_of, workspace
from .nodes import ColorSourceDefaults

N_FEAT, N_EMBED, N_HIDDEN, N_OUT = 27, 32, 128, 6
_SHAPES = (("w1", (N_HIDDEN, N_FEAT + N_EMBED)), ("b1", (N_HIDDEN,)), ("w2", (N_HIDDEN, N_HIDDEN)), ("b2", (N_HIDDEN,)),
           ("w3", (N_OUT, N_HIDDEN)), ("b3", (N_OUT,)))

__all__ = ["wild_colors", "wild_color_source", "WildColorSource"]


def _mlp_tensors(mlp):
    """The six weight / bias tensors of the appearance MLP, shapes checked (NotImplementedError names what differs)."""
    if isinstance(mlp, torch.nn.Sequential):
        kinds = [type(m).__name__ for m in mlp]
        if kinds != ["Linear", "ReLU", "Linear", "ReLU", "Linear"]:
            raise NotImplementedError(f"wild_colors: the MLP must be Sequential(Linear, ReLU, Linear, ReLU, Linear), got {kinds}")
        lin = [mlp[0], mlp[2], mlp[4]]
        if any(m.bias is None for m in lin):
            raise NotImplementedError("wild_colors: Linear layers without bias")
        ts = (lin[0].weight, lin[0].bias, lin[1].weight, lin[1].bias, lin[2].weight, lin[2].bias)
    else:
        ts = tuple(mlp)
        if len(ts) != 6:
            raise NotImplementedError(f"wild_colors: mlp must be an nn.Sequential or six tensors (w1, b1, w2, b2, w3, b3), got {len(ts)}")
    for (name, shape), t in zip(_SHAPES, ts):
        if tuple(t.shape) != shape:
            raise NotImplementedError(f"wild_colors: {name} has shape {tuple(t.shape)}; only the 59 -> 128 -> 128 -> 6 MLP of "
                                      f"WildGaussians.py is implemented ({name} {shape})")
        if t.dtype != torch.float32:
            raise NotImplementedError(f"wild_colors: {name} is {t.dtype}; fp32 only")
    return ts


def _check(features_dc: Tensor, features_rest: Tensor, embedding: Optional[Tensor]):
    N = features_dc.shape[0]
    if not (features_dc.shape in ((N, 3), (N, 1, 3))):
        raise NotImplementedError(f"wild_colors: features_dc of shape {tuple(features_dc.shape)} (expected [N, 3] or [N, 1, 3])")
    if not (features_rest.dim() == 3 and features_rest.shape[0] == N and features_rest.shape[2] == 3 and features_rest.shape[1] >= 8):
        raise NotImplementedError(f"wild_colors: features_rest of shape {tuple(features_rest.shape)} (expected [N, R, 3], R >= 8)")
    if embedding is not None and tuple(embedding.shape) not in ((N_EMBED,), (1, N_EMBED)):
        raise NotImplementedError(f"wild_colors: embedding of shape {tuple(embedding.shape)} (expected [32], [1, 32] or None)")
    for name, t in (("features_dc", features_dc), ("features_rest", features_rest), ("embedding", embedding)):
        if t is not None and t.dtype != torch.float32:
            raise NotImplementedError(f"wild_colors: {name} is {t.dtype}; fp32 only")


def _prepared(dc, rest, emb, ws):
    """Row-contiguous forms the kernels read (views where possible) -- detached: the autograd nodes own the gradients."""
    N = dc.shape[0]
    dc2 = dc.detach().reshape(N, 3)
    if dc2.stride(1) != 1 or N == 0:
        dc2 = dc2.contiguous()
    rest2 = rest.detach().reshape(N, rest.shape[1] * rest.shape[2])
    if rest2.stride(1) != 1 or N == 0:
        rest2 = rest2.contiguous()
    e = None if emb is None else emb.detach().reshape(N_EMBED).contiguous()
    return (dc2, rest2, e) + tuple(w.detach().contiguous() for w in ws)


def _widths():
    return (N_FEAT, N_EMBED, N_HIDDEN, N_OUT)


def _forward(prep, cap, vis_ids, totals, flags, out, out_stride, st):
    dc2, rest2, e, w1, b1, w2, b2, w3, b3 = prep
    wrapper.call("mtgs_wild_fwd", cap, ptr(vis_ids), ptr(totals), ptr(flags), ptr(dc2), dc2.stride(0), ptr(rest2), rest2.stride(0),
                 ptr(e), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(w3), ptr(b3), *_widths(), out if isinstance(out, int) else ptr(out),
                 out_stride, st)


def _backward(prep, shapes, need, cap, vis_ids, totals, grad_ptr, grad_stride, st):
    """Gradients of the nine inputs (dc, rest, embedding, w1, b1, w2, b2, w3, b3) from d L / d colour of the row set; None where
    `need` is False.  Dense row set (vis_ids None): every row of d features is written; a row set: zeros elsewhere."""
    dc2, rest2, e, w1, b1, w2, b2, w3, b3 = prep
    N, dev = dc2.shape[0], dc2.device
    R3 = rest2.shape[1]
    alloc = torch.empty if vis_ids is None else torch.zeros
    d_dc = alloc((N, 3), dtype=torch.float32, device=dev)
    d_rest = alloc((N, R3), dtype=torch.float32, device=dev)
    wz = torch.empty if cap > 0 else torch.zeros      # (written by mtgs_wild_reduce; no rows: zero)
    dw = [wz(s, dtype=torch.float32, device=dev) for _, s in _SHAPES]
    d_e = wz(N_EMBED, dtype=torch.float32, device=dev) if (e is not None and need[2]) else None
    if cap > 0:
        part = workspace("mtgs_wild_workspace_bytes", cap, device=dev, dtype=torch.uint8)
        wrapper.call("mtgs_wild_bwd", cap, ptr(vis_ids), ptr(totals), grad_ptr, grad_stride, ptr(dc2), dc2.stride(0), ptr(rest2),
                     rest2.stride(0), ptr(e), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(w3), ptr(b3), *_widths(), ptr(d_dc),
                     ptr(d_rest), R3, ptr(part), part.numel(), st)
        wrapper.call("mtgs_wild_reduce", cap, ptr(part), ptr(e), ptr(w1), *_widths(), *(ptr(t) for t in dw), ptr(d_e), st)
    grads = [d_dc.view(shapes[0]), d_rest.view(shapes[1]), None if d_e is None else d_e.view(shapes[2])] + dw
    return tuple(g if n else None for g, n in zip(grads, need))


class _WildColors(torch.autograd.Function):
    """The dense op: one forward (mtgs_wild_fwd) and one backward chain (mtgs_wild_bwd + mtgs_wild_reduce) over all N rows."""

    @staticmethod
    def forward(ctx, dc, rest, emb, w1, b1, w2, b2, w3, b3):
        prep = _prepared(dc, rest, emb, (w1, b1, w2, b2, w3, b3))
        N = dc.shape[0]
        out = torch.empty((N, 3), dtype=torch.float32, device=dc.device)
        if N > 0:
            _forward(prep, N, None, None, None, out, 3, stream_of(out))
        ctx.save_for_backward(*prep)      # (detached views: an in-place change of an input before the backward is caught)
        ctx.shapes = (dc.shape, rest.shape, None if emb is None else emb.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        prep = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        N = prep[0].shape[0]
        return _backward(prep, ctx.shapes, ctx.needs_input_grad, N, None, None, ptr(g), 3, stream_of(g))


def wild_colors(features_dc: Tensor, features_rest: Tensor, embedding: Optional[Tensor], mlp) -> Tensor:
    """Appearance colours [N, 3] of every Gaussian (see the module docstring); differentiable in all nine inputs."""
    ws = _mlp_tensors(mlp)
    _check(features_dc, features_rest, embedding)
    require_gpu(features_dc, features_rest, embedding, *ws)
    return _WildColors.apply(features_dc, features_rest, embedding, *ws)


class WildColorSource(ColorSourceDefaults):
    """Colour source for rasterization(color_source=...): channels 0..2 of the blended colours are the appearance colours of the
    VISIBLE Gaussians, evaluated by the rasterization between its front end and its binning (csrc/wild.hip, visible-row form),
    and its backward turns the colour-gradient rows of the compositing backward into dense gradients of the nine inputs, which
    are inputs of the rasterization's autograd node (`wild_inputs`).  camera_normals = camera_to_world [3, 4]: MTGS's three
    camera-space normal channels follow (as for nodes.ColorSource).  touch_first: only the Gaussians the frame composites from
    are evaluated (exact: colours do not change the compositing decisions).  One camera, no backgrounds, no data-parallel
    exchange: the rasterization refuses the others by name."""

    wild = True

    def __init__(self, features_dc, features_rest, embedding, ws, camera_normals=None, touch_first=False):
        self.wild_inputs = (features_dc, features_rest, embedding) + tuple(ws)
        self.camera_normals = camera_normals
        self.touch_first = bool(touch_first)
        self.row_flags = None
        self._prep = None

    def colour_rows(self, vis_ids, totals, cap_vis, recs, row_flags, stream):
        """Forward (called by the rasterization): colours of the visible rows into channels 0..2 of their records."""
        dc, rest, emb, *ws = self.wild_inputs
        self._prep = _prepared(dc, rest, emb, ws)
        self.row_flags = row_flags
        if cap_vis > 0:
            _forward(self._prep, cap_vis, vis_ids, totals, row_flags, recs.data_ptr() + 4 * 8, recs.stride(0), stream)

    def backward_rows(self, need, vis_ids, totals, n_rows, G, RS, stream):
        """Backward (called by the rasterization): gradients of the nine `wild_inputs` from the colour columns 8..10 of the
        compaction rows G [n_rows, RS] (row r = Gaussian vis_ids[r], count on the device in totals)."""
        dc, rest, emb, *_ = self.wild_inputs
        prep = self._prep if self._prep is not None else _prepared(dc, rest, emb, self.wild_inputs[3:])
        shapes = (dc.shape, rest.shape, None if emb is None else emb.shape)
        return _backward(prep, shapes, need, n_rows, vis_ids, totals, G.data_ptr() + 4 * 8, RS, stream)


def wild_color_source(features_dc: Tensor, features_rest: Tensor, embedding: Optional[Tensor], mlp,
                      camera_normals: Optional[Tensor] = None, touch_first: bool = False) -> WildColorSource:
    """A WildColorSource for rasterization(colors=None | [N, DX], color_source=src) (see the class)."""
    ws = _mlp_tensors(mlp)
    _check(features_dc, features_rest, embedding)
    require_gpu(features_dc, features_rest, embedding, camera_normals, *ws)
    return WildColorSource(features_dc, features_rest, embedding, ws, camera_normals, touch_first)
