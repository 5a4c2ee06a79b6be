"""Densification statistics of MTGS Gaussian nodes in one launch per node.

`update_statistics` does what MTGSSceneModel.update_submodel_statistics followed by
VanillaGaussianSplattingModel.after_train do per step and node
(/root/reference/mtgs/scene_model/mtgs_scene_graph.py:1157-1183,
 /root/reference/mtgs/scene_model/gaussian_model/vanilla_gaussian_splatting.py:448-474).  Under view-parallel data
parallelism every rank must take identical refine decisions: `mtgs_amd.dist.all_reduce_stats` sum-/max-reduces the
three arrays before `refinement_after` reads them.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from ._abi import struct_dtype
from ._lib import call, ptr, require_gpu, stream_of


@torch.no_grad()
def update_statistics(xys_grad_norm: Tensor, vis_counts: Tensor, max_2Dsize: Tensor, radii: Tensor, xys_grad: Tensor,
                      width: int, height: int, start: int = 0) -> None:
    """In place, for the node whose n = xys_grad_norm.numel() Gaussians are rows [start, start + n) of the collected
    arrays: radii[(1,) N] int32 (info["radii"]), xys_grad[(1,) N, 2] (info["means2d"].absgrad or .grad).
    Visible (radii > 0):  xys_grad_norm += |xys_grad * (width, height) * 0.5|,  vis_counts += 1,
    max_2Dsize = max(max_2Dsize, radii)."""
    require_gpu(xys_grad_norm, vis_counts, max_2Dsize, radii, xys_grad)
    n = xys_grad_norm.numel()
    assert vis_counts.numel() == n and max_2Dsize.numel() == n
    for t in (xys_grad_norm, vis_counts, max_2Dsize):
        assert t.dtype == torch.float32 and t.is_contiguous(), "statistics must be contiguous float32"
    radii = radii.reshape(-1)
    grads = xys_grad.reshape(-1, 2)
    assert radii.numel() == grads.shape[0] and start >= 0 and start + n <= radii.numel(), (radii.shape, grads.shape, start, n)
    r = radii[start:start + n].contiguous()
    if r.dtype != torch.int32:
        r = r.to(torch.int32)
    g = grads[start:start + n].to(torch.float32).contiguous()
    call("mtgs_densify_stats", n, ptr(r), ptr(g), int(width), int(height), ptr(xys_grad_norm), ptr(vis_counts),
         ptr(max_2Dsize), stream_of(xys_grad_norm))


_STATS_DESC = struct_dtype("mtgs_stats_desc")      # include/mtgs_rast.h


@torch.no_grad()
def update_statistics_all(stats: Sequence[Tuple[Tensor, Tensor, Tensor]], radii: Tensor, xys_grad: Tensor, width: int,
                          height: int, starts: Optional[Sequence[int]] = None) -> None:
    """`update_statistics` for every node of the scene graph in ONE launch: stats[i] = (xys_grad_norm, vis_counts,
    max_2Dsize) of node i, whose Gaussians are rows [starts[i], starts[i] + n_i) of the collected arrays (default: the nodes
    follow each other in order, as get_gaussians concatenates them)."""
    from ._lib import load
    if not stats:
        return
    flat = [t for s in stats for t in s]
    require_gpu(radii, xys_grad, *flat)
    for t in flat:
        assert t.dtype == torch.float32 and t.is_contiguous(), "statistics must be contiguous float32"
    n = np.asarray([s[0].numel() for s in stats], dtype=np.int64)
    for s_, k in zip(stats, n):
        assert s_[1].numel() == k and s_[2].numel() == k
    st = np.cumsum(n) - n if starts is None else np.asarray(starts, dtype=np.int64)
    r = radii.reshape(-1)
    r = r if r.dtype == torch.int32 else r.to(torch.int32)
    r = r.contiguous()
    g = xys_grad.reshape(-1, 2).to(torch.float32).contiguous()
    assert r.numel() == g.shape[0] and (st >= 0).all() and int((st + n).max()) <= r.numel(), (r.shape, g.shape)
    if load().mtgs_stats_desc_bytes() != _STATS_DESC.itemsize:
        raise RuntimeError("mtgs_stats_desc layout mismatch between libmtgs_rast.so and mtgs_amd.densify")
    tab = np.zeros(len(stats), dtype=_STATS_DESC)
    nblk = (n + 255) // 256
    tab["n"], tab["start"], tab["first_block"] = n, st, np.cumsum(nblk) - nblk
    for j, k in enumerate(("xys_grad_norm", "vis_counts", "max_2dsize")):
        tab[k] = [s_[j].data_ptr() for s_ in stats]
    from .nodes import upload_table
    tab_dev = upload_table(tab, r.device)
    call("mtgs_densify_stats_batch", len(stats), ptr(tab_dev), int(nblk.sum()), ptr(r), ptr(g), int(width), int(height),
         stream_of(r))


@torch.no_grad()
def update_statistics_rows(stats: Sequence[Tuple[Tensor, Tensor, Tensor]], radii: Tensor, grad_rows: Tensor, vis_ids: Tensor,
                           width: int, height: int, starts: Optional[Sequence[int]] = None, absgrad: bool = True,
                           n_vis: Optional[int] = None, n_vis_dev: Optional[Tensor] = None) -> None:
    """`update_statistics_all` from the COMPACT gradient rows of the one-node rasterization instead of a dense
    means2d gradient: grad_rows[n_vis, 16] (columns 0-1 the 2-D gradient, 2-3 its absolute-value sum) and vis_ids[n_vis]
    (flat index of each row's Gaussian), as the data-parallel exchange keeps them after the backward
    (mtgs_amd.dist.SparseGradExchange.grad_rows / .vis_ids) -- in that mode no dense gradient exists.  Same update,
    visible Gaussians only (mtgs_scene_graph.py:1157-1183, vanilla_gaussian_splatting.py:448-474).  n_vis_dev (device int64,
    mtgs_front_fwd's packed totals): the row count on the device (graph mode: the buffers are capacity-sized)."""
    from ._lib import load
    if not stats:
        return
    flat = [t for s_ in stats for t in s_]
    require_gpu(radii, grad_rows, vis_ids, *flat)
    for t in flat:
        assert t.dtype == torch.float32 and t.is_contiguous(), "statistics must be contiguous float32"
    n = np.asarray([s_[0].numel() for s_ in stats], dtype=np.int64)
    st = np.cumsum(n) - n if starts is None else np.asarray(starts, dtype=np.int64)
    assert (np.diff(st) >= 0).all(), "nodes in the order of the collected arrays"
    r = radii.reshape(-1)
    r = (r if r.dtype == torch.int32 else r.to(torch.int32)).contiguous()
    assert grad_rows.dim() == 2 and grad_rows.shape[1] >= 4 and grad_rows.dtype == torch.float32 and grad_rows.is_contiguous()
    assert vis_ids.dtype == torch.int32 and vis_ids.is_contiguous()
    nv = int(vis_ids.numel() if n_vis is None else n_vis)
    assert nv <= vis_ids.numel() and nv <= grad_rows.shape[0] and int((st + n).max()) <= r.numel()
    if load().mtgs_stats_desc_bytes() != _STATS_DESC.itemsize:
        raise RuntimeError("mtgs_stats_desc layout mismatch between libmtgs_rast.so and mtgs_amd.densify")
    tab = np.zeros(len(stats), dtype=_STATS_DESC)
    tab["n"], tab["start"] = n, st
    for j, k in enumerate(("xys_grad_norm", "vis_counts", "max_2dsize")):
        tab[k] = [s_[j].data_ptr() for s_ in stats]
    from .nodes import upload_table
    tab_dev = upload_table(tab, r.device)
    call("mtgs_densify_stats_rows", nv, ptr(vis_ids), ptr(grad_rows), int(grad_rows.shape[1]), 2 if absgrad else 0, ptr(r),
         len(stats), ptr(tab_dev), int(width), int(height), ptr(n_vis_dev), stream_of(r))


# ------------------------------------------------------------------------------------------------ refinement on device
import ctypes as _C
from dataclasses import dataclass
from typing import Dict


@dataclass
class RefineConfig:
    """The control fields of GaussianSplattingControlConfig that refinement_after reads
    (vanilla_gaussian_splatting.py:29-66; values of the shipped config/MTGS.py:59-71 with iteration_factor 1)."""
    refine_every: int = 100
    stop_split_at: int = 15000
    reset_alpha_every: int = 30
    continue_cull_post_densification: bool = False
    cull_alpha_thresh: float = 0.005
    cull_scale_thresh: float = 0.5
    densify_size_thresh: float = 0.2
    densify_grad_thresh: float = 0.001
    n_split_samples: int = 2
    clone_sample_means: bool = True
    stop_screen_size_at: int = 15000
    cull_screen_size: float = 150.0
    split_screen_size: float = 100.0
    densify_from_iter: int = 500       # refine_scene's gate (step <= densify_from_iter: untouched); refine_gaussians ignores it


@torch.no_grad()
def refine_gaussians(params: Dict[str, Tensor], stats: Tuple[Tensor, Tensor, Tensor], cfg: RefineConfig, step: int, seed: int,
                     moments: Optional[Dict[str, Tuple[Tensor, Tensor]]] = None, extras: Optional[Dict[str, Tensor]] = None,
                     before_rows=None):
    """VanillaGaussianSplattingModel.refinement_after (densification branch, step < stop_split_at) for one node, on the
    device: split / duplicate / cull, every per-Gaussian tensor of `params` (means[N,3], scales[N,3] log, quats[N,4] wxyz,
    opacities[N,1] logit, + any other [N, ...] tensors: features_dc / features_rest / features_adapters ...) compacted and
    appended in the reference's order, the Adam moments `moments[name] = (exp_avg, exp_avg_sq)` following their rows
    (zeros for new Gaussians, dup_in_optim / remove_from_optim).  stats = (xys_grad_norm, vis_counts, max_2Dsize).

    Rank-deterministic: the split / clone samples come from a counter-based generator keyed by (seed, step, Gaussian index,
    sample) -- with all-reduced statistics (mtgs_amd.dist.all_reduce_stats) every rank of a data-parallel job produces
    bit-identical tensors, so N stays identical without a broadcast (the reference draws torch.randn per rank, :642, :687).
    ONE host synchronisation: the new N (tensor sizes).  Returns (new_params, new_moments | None, info) with
    info = {n_before, n_after, n_old_kept (old Gaussians kept), n_children (split children), n_dups, n_split (split parents; a device scalar),
    src_index, kind}.
    extras {name: [N, ...] tensor of a 4-byte dtype}: moved like a parameter (a child / duplicate takes its parent's row) and
    returned in info["extras"] -- the row-lazy optimizer's `last` stamps.  before_rows(parents bool [N]): called after the
    decisions are known and before any row is copied, with the Gaussians that get children or a duplicate -- a caller whose rows are
    lazy brings THOSE rows up to date there (FusedAdam.catch_up_rows) instead of flushing every row.
    The four GEOMETRY tensors (means, scales, quats, opacities) must be CURRENT when this function is called: the split / cull
    decisions and the children's positions are computed from them before the hook runs, so the hook is only good for tensors that
    are copied afterwards (colours, extras).  A caller whose geometry rows are lazy flushes them first."""
    from ._lib import call, ptr, stream_of
    means, scales, quats, opac = (params[k] for k in ("means", "scales", "quats", "opacities"))
    require_gpu(means, scales, quats, opac, *stats)
    N, dev = means.shape[0], means.device
    assert means.shape == (N, 3) and scales.shape == (N, 3) and quats.shape == (N, 4) and opac.numel() == N
    for t in params.values():
        assert t.dtype == torch.float32 and t.shape[0] == N, "every parameter is float32 with one row per Gaussian"
    gn, vc, m2 = (t.reshape(-1).to(torch.float32).contiguous() for t in stats)
    assert gn.numel() == N and vc.numel() == N and m2.numel() == N
    S = int(cfg.n_split_samples)
    th = (_C.c_float * 6)(cfg.densify_grad_thresh, cfg.densify_size_thresh, cfg.split_screen_size, cfg.cull_alpha_thresh,
                          cfg.cull_scale_thresh, cfg.cull_screen_size)
    cull_big = step > cfg.refine_every * cfg.reset_alpha_every
    opt = (_C.c_int * 5)(S, int(step < cfg.stop_screen_size_at), int(cull_big), int(cull_big and step < cfg.stop_screen_size_at),
                         int(cfg.clone_sample_means))
    st = stream_of(means)
    c = {k: params[k].detach().contiguous() for k in params}
    counts = torch.empty((2 + S, max(N, 1)), dtype=torch.int32, device=dev)
    flags = torch.empty(max(N, 1), dtype=torch.uint8, device=dev)
    call("mtgs_refine_classify", N, ptr(c["means"]), ptr(c["scales"]), ptr(c["quats"]), ptr(c["opacities"]), ptr(gn), ptr(vc), ptr(m2),
         th, opt, _C.c_uint64(seed & (2 ** 64 - 1)), int(step), ptr(counts), ptr(flags), st)
    counts = counts[:, :N]
    incl = torch.cumsum(counts, dim=1, dtype=torch.int64)
    pos = (incl - counts).contiguous()
    totals = incl[:, -1] if N > 0 else torch.zeros(2 + S, dtype=torch.int64, device=dev)
    bases = (torch.cumsum(totals, 0) - totals).contiguous()
    tot_h = totals.tolist()                      # the one host synchronisation: the new tensor sizes
    n_out = int(sum(tot_h))
    src_index = torch.empty(max(n_out, 1), dtype=torch.int32, device=dev)
    kind = torch.empty(max(n_out, 1), dtype=torch.uint8, device=dev)
    new = {"means": torch.empty((n_out, 3), dtype=torch.float32, device=dev),
           "scales": torch.empty((n_out, 3), dtype=torch.float32, device=dev)}
    call("mtgs_refine_apply", N, n_out, ptr(flags), ptr(pos), ptr(bases), ptr(c["means"]), ptr(c["scales"]), ptr(c["quats"]), th, opt,
         _C.c_uint64(seed & (2 ** 64 - 1)), int(step), ptr(src_index), ptr(kind), ptr(new["means"]), ptr(new["scales"]), st)

    if before_rows is not None and N > 0:
        assert 1 <= S <= 4, S                      # (MAX_SAMPS of csrc/refine.hip; flag byte: bit 0 old row kept, bits 1..S children, bit 1+S duplicate, bit 7 split parent)
        before_rows((flags[:N] & (((1 << (S + 1)) - 1) << 1)) != 0)      # (bits 1 .. 1 + S: a child or the duplicate is kept)

    def rows(src, zero_new):
        w = src.numel() // max(N, 1)
        dst = torch.empty((n_out,) + tuple(src.shape[1:]), dtype=torch.float32, device=dev)
        call("mtgs_refine_rows", n_out, w, ptr(src.contiguous()), ptr(src_index), ptr(kind), int(zero_new), ptr(dst), st)
        return dst

    for k, t in c.items():
        if k not in new:
            new[k] = rows(t, False)
    new_moments = None
    if moments is not None:
        new_moments = {k: (rows(a.detach(), True), rows(b.detach(), True)) for k, (a, b) in moments.items()}
    moved = {}
    for k, t in (extras or {}).items():
        assert t.shape[0] == N and t.element_size() == 4, "extras: [N, ...] tensors of a 4-byte dtype"
        moved[k] = rows(t.contiguous().view(torch.float32), False).view(t.dtype)      # (a bit-for-bit row copy)
    # (n_split stays a DEVICE scalar: children can be culled one by one, so the number of split parents does not follow from
    #  the totals, and a second host synchronisation is not worth a log line -- int(info["n_split"]) reads it when wanted)
    info = {"n_before": N, "n_after": n_out, "n_old_kept": tot_h[0], "n_children": sum(tot_h[1:1 + S]), "n_dups": tot_h[1 + S],
            "n_split": (flags[:N] >> 7).sum() if N else torch.zeros((), dtype=torch.int64, device=dev),
            "src_index": src_index[:n_out], "kind": kind[:n_out], "extras": moved}
    return new, new_moments, info


@torch.no_grad()
def reset_opacities(opacities: Tensor, cfg: RefineConfig, moments: Optional[Tuple[Tensor, Tensor]] = None) -> None:
    """The opacity reset of refinement_after (:555-572): clamp the logits at logit(2 cull_alpha_thresh), zero their moments."""
    v = 2.0 * cfg.cull_alpha_thresh
    opacities.clamp_(max=float(np.log(v / (1.0 - v))))
    if moments is not None:
        moments[0].zero_()
        moments[1].zero_()


# ------------------------------------------------------------------------------------- refinement of a whole scene graph
from typing import List

from ._abi import header_abi as _header_abi

_SCENE_ABI = _header_abi("mtgs_refine_scene.h")          # include/mtgs_refine_scene.h
_REFINE_NODE = _SCENE_ABI.structs["mtgs_refine_node"]
_REFINE_MOVE = _SCENE_ABI.structs["mtgs_refine_move"]
_DENSIFY, _CULL_ONLY = _SCENE_ABI.constants["MTGS_REFINE_DENSIFY"], _SCENE_ABI.constants["MTGS_REFINE_CULL_ONLY"]
_COPY, _ZERO_NEW, _CLAMP_MAX, _ZERO_ALL = (_SCENE_ABI.constants["MTGS_REFINE_" + k] for k in ("COPY", "ZERO_NEW", "CLAMP_MAX", "ZERO_ALL"))
_MOVE_DWORDS = _SCENE_ABI.constants["MTGS_REFINE_MOVE_DWORDS"]     # dwords of a move one workgroup of mtgs_refine_scene_rows works on
_GEOMETRY = ("means", "scales", "quats", "opacities")


@dataclass
class NodeRefine:
    """One node of the scene graph as refine_scene sees it.  params / stats / cfg / seed / moments / extras: the arguments of
    refine_gaussians (MTGS overlays the control config per node, mtgs_scene_graph.py:194-205, hence a cfg per node).
    stats None: the node never collected statistics (rigid_node.py:356-366, deformable_node.py:288-298).
    cull_rule = (far radius, far factor): beyond |mean| > radius the world-size limit is factor x cull_scale_thresh.
    (100, 40) is VanillaGaussianSplattingModel.cull_gaussians (:599-600); the sky node takes
    (skybox_radius / 10, skybox_scale_factor) (skybox_gaussian_splatting.py:147-148).  frozen: the node's `frozen` flag (:478)."""
    params: Dict[str, Tensor]
    stats: Optional[Tuple[Tensor, Tensor, Tensor]]
    cfg: RefineConfig
    seed: int
    moments: Optional[Dict[str, Tuple[Tensor, Tensor]]] = None
    extras: Optional[Dict[str, Tensor]] = None
    cull_rule: Tuple[float, float] = (100.0, 40.0)
    frozen: bool = False


def refine_phase(node: NodeRefine, step: int) -> int:
    """What refinement_after does with this node at `step` (vanilla_gaussian_splatting.py:476-550): 0 untouched,
    MTGS_REFINE_DENSIFY or MTGS_REFINE_CULL_ONLY.  No tensor is read."""
    cfg = node.cfg
    if node.frozen or step <= cfg.densify_from_iter or node.params["means"].shape[0] == 0:       # :478-484
        return 0
    if step < cfg.stop_split_at:                                                                  # :486
        return 0 if node.stats is None else _DENSIFY       # (the rigid / deformable skip; a vanilla node asserts at :491)
    return _CULL_ONLY if cfg.continue_cull_post_densification else 0                              # :546-550


def _c(t: Tensor) -> Tensor:
    return t if t.is_contiguous() else t.contiguous()


@torch.no_grad()
def refine_scene(nodes: Sequence[NodeRefine], step: int, before_rows=None) -> List[Optional[Tuple[dict, Optional[dict], dict]]]:
    """refinement_after (vanilla_gaussian_splatting.py:476-577) for EVERY node of a scene graph in one pass: one classify launch,
    one prefix sum, ONE blocking host read (the per-node, per-column survivor totals, which fix the new sizes), one index and one
    geometry launch and one table-driven launch that moves every remaining tensor of every node -- whatever the number of nodes.

    Per node, as the reference gates it:
      untouched (result None, no tensor read or written): frozen, step <= cfg.densify_from_iter, N == 0; in the densify phase
        with stats None -- the "never seen, skip" rule of the rigid and deformable nodes; a VANILLA node in that state asserts in
        the reference (:491), here it is skipped like the others; and past stop_split_at without
        continue_cull_post_densification.
      densify (step < stop_split_at): exactly refine_gaussians(params, stats, cfg, step, seed, ...) -- the samples are keyed by
        (node seed, step, node-local Gaussian index, slot), so the result is bit-identical to that call whatever the node's
        neighbours are -- with the cull rule node.cull_rule in place of the constants 100 / 40, and, when
        step % (reset_alpha_every * refine_every) == refine_every, followed in the same pass by reset_opacities (:555-573):
        the new opacities clamped at logit(2 cull_alpha_thresh), their moments zero.
      cull-only (step >= stop_split_at and continue_cull_post_densification): cull_gaussians() alone (:546-547); rows only leave,
        the moments follow, stats may be None unless the screen-size rule is still on (step < stop_screen_size_at), which reads
        max_2Dsize: ValueError, as the reference asserts (:607).

    Returns one entry per node: None, or (new_params, new_moments | None, info) with refine_gaussians' info keys (n_split is a
    host int here: it comes with the one host read).  The new tensors are VIEWS of one buffer per tensor name (and row shape):
    a hundred nodes do not cost a hundred allocations per tensor.  before_rows(masks): called once, after all decisions and
    before any row moves, masks[i] = bool [N_i] of the Gaussians of node i that get children or a duplicate (None for an untouched
    node); as in refine_gaussians the four geometry tensors must be current before the call.  extras move like parameters.
    Isotropic nodes (scales[N, 1], no quats) are not supported: NotImplementedError."""
    from ._lib import call, ptr, stream_of
    from .nodes import upload_table
    results: List[Optional[tuple]] = [None] * len(nodes)
    act = []                                               # (index into nodes, phase)
    for j, nd in enumerate(nodes):                         # what is not supported, before anything else
        scales = nd.params["scales"]
        if "quats" not in nd.params or scales.dim() != 2 or scales.shape[1] != 3:
            raise NotImplementedError(f"refine_scene: node {j} is isotropic (scales {tuple(scales.shape)}, "
                                      f"{'no ' if 'quats' not in nd.params else ''}quats): only scale_dim == 3 nodes are supported")
    for j, nd in enumerate(nodes):
        p = nd.params
        means, scales = p["means"], p["scales"]
        N = means.shape[0]
        require_gpu(*p.values(), *(nd.stats or ()), *(nd.extras or {}).values(), *(t for ab in (nd.moments or {}).values() for t in ab))
        if means.shape != (N, 3) or scales.shape != (N, 3) or p["quats"].shape != (N, 4) or p["opacities"].numel() != N:
            raise ValueError(f"refine_scene: node {j}: means[N,3], scales[N,3], quats[N,4], opacities[N(,1)] expected")
        for k, t in p.items():
            if t.dtype != torch.float32 or t.shape[0] != N:
                raise ValueError(f"refine_scene: node {j}: parameter {k!r} must be float32 with one row per Gaussian")
        for k, (a, b) in (nd.moments or {}).items():
            if k not in p or a.shape != p[k].shape or b.shape != p[k].shape or a.dtype != torch.float32 or b.dtype != torch.float32:
                raise ValueError(f"refine_scene: node {j}: moments of {k!r} must be two float32 tensors of the parameter's shape")
        for k, t in (nd.extras or {}).items():
            if t.shape[0] != N or t.element_size() != 4:
                raise ValueError(f"refine_scene: node {j}: extra {k!r} must be an [N, ...] tensor of a 4-byte dtype")
        if not 1 <= int(nd.cfg.n_split_samples) <= 4:
            raise ValueError(f"refine_scene: node {j}: n_split_samples={nd.cfg.n_split_samples} (1..4)")
        ph = refine_phase(nd, step)
        if ph:
            act.append((j, ph))
    if not act:
        return results
    A = len(act)
    dev = nodes[act[0][0]].params["means"].device
    st = stream_of(nodes[act[0][0]].params["means"])
    nb, mb = _C.c_size_t(0), _C.c_size_t(0)
    call("mtgs_refine_scene_table_bytes", _C.byref(nb), _C.byref(mb))
    if (nb.value, mb.value) != (_REFINE_NODE.itemsize, _REFINE_MOVE.itemsize):
        raise RuntimeError("mtgs_refine_node / mtgs_refine_move layout mismatch between libmtgs_rast.so and mtgs_amd.densify")

    # ---- the node table: sizes, pointers, thresholds, options, rule, phase ---------------------------------------------------
    tab = np.zeros(A, dtype=_REFINE_NODE)
    keep_alive = []                                        # converted inputs (non-contiguous / non-float32 statistics): rare
    geo = {k: [] for k in _GEOMETRY}
    stat_ptrs = ([], [], [])
    n, resets = np.zeros(A, dtype=np.int64), [False] * A
    for i, (j, ph) in enumerate(act):
        nd, cfg = nodes[j], nodes[j].cfg
        n[i] = nd.params["means"].shape[0]
        for k in _GEOMETRY:
            t = _c(nd.params[k])
            keep_alive.append(t)
            geo[k].append(t.data_ptr())
        cull_big = step > cfg.refine_every * cfg.reset_alpha_every
        opt = (int(cfg.n_split_samples), int(step < cfg.stop_screen_size_at), int(cull_big),
               int(cull_big and step < cfg.stop_screen_size_at), int(cfg.clone_sample_means))
        if nd.stats is None:
            if opt[3]:
                raise ValueError(f"refine_scene: node {j}: the screen-size cull rule is on at step {step} "
                                 f"(< stop_screen_size_at = {cfg.stop_screen_size_at}) and reads max_2Dsize: stats must not be None")
            for q in stat_ptrs:
                q.append(0)
        else:
            for q, t in zip(stat_ptrs, nd.stats):
                if t.numel() != n[i]:
                    raise ValueError(f"refine_scene: node {j}: statistics must have one element per Gaussian")
                if t.dtype != torch.float32 or not t.is_contiguous():
                    t = t.to(torch.float32).contiguous()
                    keep_alive.append(t)
                q.append(t.data_ptr())
        tab["thresholds"][i] = (cfg.densify_grad_thresh, cfg.densify_size_thresh, cfg.split_screen_size, cfg.cull_alpha_thresh,
                                cfg.cull_scale_thresh, cfg.cull_screen_size)
        tab["options"][i] = opt
        tab["far_radius"][i], tab["far_factor"][i] = nd.cull_rule
        tab["seed"][i] = nd.seed & (2 ** 64 - 1)
        tab["phase"][i] = ph
        resets[i] = ph == _DENSIFY and step % (cfg.reset_alpha_every * cfg.refine_every) == cfg.refine_every     # :555
    nblk = (n + 255) // 256
    n_total, total_blocks = int(n.sum()), int(nblk.sum())
    if n_total >= 2 ** 31:
        raise ValueError(f"refine_scene: {n_total} Gaussians in the scene (limit 2^31 - 1)")
    tab["n"], tab["start"], tab["first_block"] = n, np.cumsum(n) - n, np.cumsum(nblk) - nblk
    for k in _GEOMETRY:
        tab[k] = geo[k]
    for k, q in zip(("xys_grad_norm", "vis_counts", "max_2dsize"), stat_ptrs):
        tab[k] = q
    ncol = 2 + int(tab["options"][:, 0].max())

    # ---- decisions, prefix sums, the one host read ---------------------------------------------------------------------------
    counts = torch.empty((ncol + 1, n_total), dtype=torch.int32, device=dev)
    flags = torch.empty(n_total, dtype=torch.uint8, device=dev)
    parents = torch.empty(n_total, dtype=torch.uint8, device=dev) if before_rows is not None else None
    ends = upload_table(np.cumsum(n) - 1, dev).view(torch.int64)
    call("mtgs_refine_scene_classify", A, ptr(upload_table(tab, dev)), total_blocks, n_total, ncol, int(step), ptr(counts), ptr(flags),
         ptr(parents), st)
    incl = torch.cumsum(counts, dim=1, dtype=torch.int64)
    bound = incl.index_select(1, ends).cpu().numpy()       # [ncol + 1, A]: THE host synchronisation
    before = np.concatenate([np.zeros((ncol + 1, 1), dtype=np.int64), bound[:, :-1]], axis=1)
    tot = bound - before                                   # survivors per column and node; last row: split parents
    n_out = tot[:ncol].sum(axis=0)
    oblk = (n_out + 255) // 256
    out_start = np.cumsum(n_out) - n_out
    n_out_total, out_blocks = int(n_out.sum()), int(oblk.sum())
    if n_out_total >= 2 ** 31:
        raise ValueError(f"refine_scene: {n_out_total} Gaussians after the refinement (limit 2^31 - 1)")
    tab["n_out"], tab["out_start"], tab["out_first_block"] = n_out, out_start, np.cumsum(oblk) - oblk
    tab["scan_base"][:, :ncol] = before[:ncol].T
    tab["col_base"][:, :ncol] = (np.cumsum(tot[:ncol], axis=0) - tot[:ncol]).T
    src_index = torch.empty(n_out_total, dtype=torch.int32, device=dev)
    kind = torch.empty(n_out_total, dtype=torch.uint8, device=dev)
    out_means = torch.empty((n_out_total, 3), dtype=torch.float32, device=dev)
    out_scales = torch.empty((n_out_total, 3), dtype=torch.float32, device=dev)
    call("mtgs_refine_scene_apply", A, ptr(upload_table(tab, dev)), total_blocks, out_blocks, n_total, n_out_total, ncol, int(step),
         ptr(flags), ptr(incl), ptr(src_index), ptr(kind), ptr(out_means), ptr(out_scales), st)

    if before_rows is not None:
        masks: List[Optional[Tensor]] = [None] * len(nodes)
        for (j, _), m in zip(act, parents.view(torch.bool).split(n.tolist())):
            masks[j] = m
        before_rows(masks)

    # ---- every remaining tensor: one buffer per (tensor, row shape), one move per (node, tensor) ----------------------------------
    rows = n_out.tolist()
    groups: Dict[tuple, list] = {}                         # (what, name, row shape, dtype) -> [(active node, source, op, clamp)]
    for i, (j, ph) in enumerate(act):
        nd, cfg = nodes[j], nodes[j].cfg
        v = 2.0 * cfg.cull_alpha_thresh
        clamp = float(np.log(v / (1.0 - v)))
        for k, t in nd.params.items():
            if k in ("means", "scales"):
                continue
            op = _CLAMP_MAX if (k == "opacities" and resets[i]) else _COPY
            groups.setdefault(("p", k, tuple(t.shape[1:]), t.dtype), []).append((i, t, op, clamp))
        for k, ab in (nd.moments or {}).items():
            op = _ZERO_ALL if (k == "opacities" and resets[i]) else _ZERO_NEW
            for h, t in enumerate(ab):
                groups.setdefault(("m%d" % h, k, tuple(t.shape[1:]), t.dtype), []).append((i, t, op, 0.0))
        for k, t in (nd.extras or {}).items():
            groups.setdefault(("x", k, tuple(t.shape[1:]), t.dtype), []).append((i, t, _COPY, 0.0))
    moved: Dict[tuple, Tensor] = {}                        # (what, name, active node) -> the node's view
    mv_cols = ([], [], [], [], [], [], [], [])             # n_rows, out_start, n_src, src, dst, width, op, clamp_max
    for (what, name, shape, dtype), members in groups.items():
        w = int(np.prod(shape, dtype=np.int64)) if shape else 1
        if not 1 <= w <= 32768:
            raise ValueError(f"refine_scene: {name!r}: rows of {w} elements (1..32768)")
        sizes = [rows[i] for i, *_ in members]
        buf = torch.empty((sum(sizes),) + shape, dtype=dtype, device=dev)
        base, off = buf.data_ptr(), 0
        for (i, t, op, clamp), view, r in zip(members, buf.split(sizes), sizes):
            moved[(what, name, i)] = view
            if r:
                t = _c(t)
                keep_alive.append(t)
                for col, val in zip(mv_cols, (r, int(out_start[i]), int(n[i]), t.data_ptr(), base + off * w * 4, w, op, clamp)):
                    col.append(val)
            off += r
    M = len(mv_cols[0])
    if M:
        mv = np.zeros(M, dtype=_REFINE_MOVE)
        for key, col in zip(("n_rows", "out_start", "n_src", "src", "dst", "width", "op", "clamp_max"), mv_cols):
            mv[key] = col
        blocks = (mv["n_rows"] * mv["width"] + 3 + _MOVE_DWORDS - 1) // _MOVE_DWORDS
        mv["first_block"] = np.cumsum(blocks) - blocks
        call("mtgs_refine_scene_rows", M, ptr(upload_table(mv, dev)), int(blocks.sum()), ptr(src_index), ptr(kind), st)

    # ---- the nodes' results: views ------------------------------------------------------------------------------------------------
    means_v, scales_v = out_means.split(rows), out_scales.split(rows)
    src_v, kind_v = src_index.split(rows), kind.split(rows)
    for i, (j, ph) in enumerate(act):
        nd = nodes[j]
        S = int(nd.cfg.n_split_samples)
        new = {k: (means_v[i] if k == "means" else scales_v[i] if k == "scales" else moved[("p", k, i)]) for k in nd.params}
        new_m = None if nd.moments is None else {k: (moved[("m0", k, i)], moved[("m1", k, i)]) for k in nd.moments}
        t = tot[:, i].tolist()
        info = {"n_before": int(n[i]), "n_after": rows[i], "n_old_kept": t[0], "n_children": sum(t[1:1 + S]), "n_dups": t[1 + S],
                "n_split": t[ncol], "src_index": src_v[i], "kind": kind_v[i],
                "extras": {k: moved[("x", k, i)] for k in (nd.extras or {})}}
        results[j] = (new, new_m, info)
    return results
