"""Densification of MTGS Gaussian nodes on the device: the statistics in one launch per node or
per scene, and refinement_after through ONE implementation -- `refine_scene` for every node of a scene graph in one pass,
`refine_gaussians` for one node as the one-entry case of the same node table (csrc/refine.hip, include/mtgs_refine_scene.h).

`update_statistics` does what MTGSSceneModel.update_submodel_statistics followed by
VanillaGaussianSplattingModel.after_train do per step and node
(/root/reference/mtgs/scene_model/mtgs_scene_graph.py:1157-1183,
 /root/reference/mtgs/scene_model/gaussian_model/vanilla_gaussian_splatting.py:448-474).  Under view-parallel data
parallelism every rank must take identical refine decisions: `mtgs_amd.dist.all_reduce_stats` sum-/max-reduces the
three arrays before `refinement_after` reads them.
"""
from __future__ import annotations

import ctypes as _C
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from ._abi import header_abi as _header_abi, struct_dtype
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


def _stats_table(stats, n: np.ndarray, st: np.ndarray, dev, first_block: Optional[np.ndarray] = None) -> Tensor:
    """The device table of mtgs_stats_desc for the nodes' statistics: n / start / the three pointers (+ first_block)."""
    from ._lib import load
    from .nodes import upload_table
    if load().mtgs_stats_desc_bytes() != _STATS_DESC.itemsize:
        raise RuntimeError("mtgs_stats_desc layout mismatch between libmtgs_rast.so and mtgs_amd.densify")
    tab = np.zeros(len(stats), dtype=_STATS_DESC)
    tab["n"], tab["start"] = n, st
    if first_block is not None:
        tab["first_block"] = first_block
    for j, k in enumerate(("xys_grad_norm", "vis_counts", "max_2dsize")):
        tab[k] = [s_[j].data_ptr() for s_ in stats]
    return upload_table(tab, dev)


@torch.no_grad()
def update_statistics_all(stats: Sequence[Tuple[Tensor, Tensor, Tensor]], radii: Tensor, xys_grad: Tensor, width: int,
                          height: int, starts: Optional[Sequence[int]] = None) -> None:
    """`update_statistics` for every node of the scene graph in ONE launch: stats[i] = (xys_grad_norm, vis_counts,
    max_2Dsize) of node i, whose Gaussians are rows [starts[i], starts[i] + n_i) of the collected arrays (default: the nodes
    follow each other in order, as get_gaussians concatenates them)."""
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
    nblk = (n + 255) // 256
    tab_dev = _stats_table(stats, n, st, r.device, first_block=np.cumsum(nblk) - nblk)
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
    tab_dev = _stats_table(stats, n, st, r.device)
    call("mtgs_densify_stats_rows", nv, ptr(vis_ids), ptr(grad_rows), int(grad_rows.shape[1]), 2 if absgrad else 0, ptr(r),
         len(stats), ptr(tab_dev), int(width), int(height), ptr(n_vis_dev), stream_of(r))


# ------------------------------------------------------------------------------------------------ refinement on device
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
def reset_opacities(opacities: Tensor, cfg: RefineConfig, moments: Optional[Tuple[Tensor, Tensor]] = None) -> None:
    """The opacity reset of refinement_after (:555-572): clamp the logits at logit(2 cull_alpha_thresh), zero their moments."""
    v = 2.0 * cfg.cull_alpha_thresh
    opacities.clamp_(max=float(np.log(v / (1.0 - v))))
    if moments is not None:
        moments[0].zero_()
        moments[1].zero_()


# ------------------------------------------------------------------------------------- refinement of a whole scene graph
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
def _refine_nodes(nodes: Sequence[NodeRefine], plan: Sequence[Tuple[int, bool]], step: int, before_rows, who: str) -> List[Optional[tuple]]:
    """The one implementation behind refine_scene and refine_gaussians: plan[j] = (phase, reset) of nodes[j] -- phase 0 untouched,
    MTGS_REFINE_DENSIFY or MTGS_REFINE_CULL_ONLY (an empty node is untouched whatever its phase); reset: the opacity reset inside
    the row move -- and everything from the node table to the result views.  Every node's arguments are checked, whatever its phase, before the first launch.  `who` names
    the caller in the messages."""
    from .nodes import upload_table
    results: List[Optional[tuple]] = [None] * len(nodes)
    for j, nd in enumerate(nodes):                         # what is not supported, before anything else
        scales = nd.params["scales"]
        if "quats" not in nd.params or scales.dim() != 2 or scales.shape[1] != 3:
            raise NotImplementedError(f"{who}: node {j} is isotropic (scales {tuple(scales.shape)}, "
                                      f"{'no ' if 'quats' not in nd.params else ''}quats): only scale_dim == 3 nodes are supported")
    for j, nd in enumerate(nodes):
        p = nd.params
        means, scales = p["means"], p["scales"]
        N = means.shape[0]
        require_gpu(*p.values(), *(nd.stats or ()), *(nd.extras or {}).values(), *(t for ab in (nd.moments or {}).values() for t in ab))
        if means.shape != (N, 3) or scales.shape != (N, 3) or p["quats"].shape != (N, 4) or p["opacities"].numel() != N:
            raise ValueError(f"{who}: node {j}: means[N,3], scales[N,3], quats[N,4], opacities[N(,1)] expected")
        for k, t in p.items():
            if t.dtype != torch.float32 or t.shape[0] != N:
                raise ValueError(f"{who}: node {j}: parameter {k!r} must be float32 with one row per Gaussian")
        for k, (a, b) in (nd.moments or {}).items():
            if k not in p or a.shape != p[k].shape or b.shape != p[k].shape or a.dtype != torch.float32 or b.dtype != torch.float32:
                raise ValueError(f"{who}: node {j}: moments of {k!r} must be two float32 tensors of the parameter's shape")
        for k, t in (nd.extras or {}).items():
            if t.shape[0] != N or t.element_size() != 4:
                raise ValueError(f"{who}: node {j}: extra {k!r} must be an [N, ...] tensor of a 4-byte dtype")
        if not 1 <= int(nd.cfg.n_split_samples) <= 4:
            raise ValueError(f"{who}: node {j}: n_split_samples={nd.cfg.n_split_samples} (1..4)")
    act = [(j, ph) for j, (ph, _) in enumerate(plan) if ph and nodes[j].params["means"].shape[0]]      # (index into nodes, phase)
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
    n, resets = np.zeros(A, dtype=np.int64), [plan[j][1] for j, _ in act]
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
            if ph == _DENSIFY:
                raise ValueError(f"{who}: node {j}: the densify phase reads the statistics: stats must not be None")
            if opt[3]:
                raise ValueError(f"{who}: node {j}: the screen-size cull rule is on at step {step} "
                                 f"(< stop_screen_size_at = {cfg.stop_screen_size_at}) and reads max_2Dsize: stats must not be None")
            for q in stat_ptrs:
                q.append(0)
        else:
            for q, t in zip(stat_ptrs, nd.stats):
                if t.numel() != n[i]:
                    raise ValueError(f"{who}: node {j}: statistics must have one element per Gaussian")
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
    nblk = (n + 255) // 256
    n_total, total_blocks = int(n.sum()), int(nblk.sum())
    if n_total >= 2 ** 31:
        raise ValueError(f"{who}: {n_total} Gaussians in the scene (limit 2^31 - 1)")
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
        raise ValueError(f"{who}: {n_out_total} Gaussians after the refinement (limit 2^31 - 1)")
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
        clamp = float(np.log(v / (1.0 - v))) if resets[i] else 0.0       # (read by MTGS_REFINE_CLAMP_MAX only)
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
        w = math.prod(shape)
        if not 1 <= w <= 32768:
            raise ValueError(f"{who}: {name!r}: rows of {w} elements (1..32768)")
        sizes = [rows[i] for i, *_ in members]
        buf = torch.empty((sum(sizes),) + shape, dtype=dtype, device=dev)
        base, off = buf.data_ptr(), 0
        for (i, t, op, clamp), view, r in zip(members, buf.split_with_sizes(sizes), sizes):
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
    means_v, scales_v = out_means.split_with_sizes(rows), out_scales.split_with_sizes(rows)
    src_v, kind_v = src_index.split_with_sizes(rows), kind.split_with_sizes(rows)
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
      densify (step < stop_split_at): exactly refine_gaussians(params, stats, cfg, step, seed, ...), which is this pass with a
        table of one node -- the samples are keyed by (node seed, step, node-local Gaussian index, slot), so the result is
        bit-identical to that call whatever the node's neighbours are -- with the cull rule node.cull_rule in place of the constants 100 / 40, and, when
        step % (reset_alpha_every * refine_every) == refine_every, followed in the same pass by reset_opacities (:555-573):
        the new opacities clamped at logit(2 cull_alpha_thresh), their moments zero.
      cull-only (step >= stop_split_at and continue_cull_post_densification): cull_gaussians() alone (:546-547); rows only leave,
        the moments follow, stats may be None unless the screen-size rule is still on (step < stop_screen_size_at), which reads
        max_2Dsize: ValueError, as the reference asserts (:607).

    Returns one entry per node: None, or (new_params, new_moments | None, info) with refine_gaussians' info keys.  The new tensors
    are VIEWS of one buffer per tensor name (and row shape): a hundred nodes do not cost a hundred allocations per tensor.  before_rows(masks): called once, after all decisions and
    before any row moves, masks[i] = bool [N_i] of the Gaussians of node i that get children or a duplicate (None for an untouched
    node); as in refine_gaussians the four geometry tensors must be current before the call.  extras move like parameters.
    Isotropic nodes (scales[N, 1], no quats) are not supported: NotImplementedError."""
    plan = []
    for nd in nodes:
        ph, cfg = refine_phase(nd, step), nd.cfg
        plan.append((ph, ph == _DENSIFY and step % (cfg.reset_alpha_every * cfg.refine_every) == cfg.refine_every))     # :555
    return _refine_nodes(nodes, plan, step, before_rows, "refine_scene")


@torch.no_grad()
def refine_gaussians(params: Dict[str, Tensor], stats: Tuple[Tensor, Tensor, Tensor], cfg: RefineConfig, step: int, seed: int,
                     moments: Optional[Dict[str, Tuple[Tensor, Tensor]]] = None, extras: Optional[Dict[str, Tensor]] = None,
                     before_rows=None):
    """VanillaGaussianSplattingModel.refinement_after (densification branch, step < stop_split_at) for one node, on the
    device: split / duplicate / cull, every per-Gaussian tensor of `params` (means[N,3], scales[N,3] log, quats[N,4] wxyz,
    opacities[N,1] logit, + any other [N, ...] tensors: features_dc / features_rest / features_adapters ...) compacted and
    appended in the reference's order, the Adam moments `moments[name] = (exp_avg, exp_avg_sq)` following their rows
    (zeros for new Gaussians, dup_in_optim / remove_from_optim).  stats = (xys_grad_norm, vis_counts, max_2Dsize).

    The one-entry case of refine_scene's node table -- the same launches, the same bits -- with the gates taken out: the phase is
    densify whatever densify_from_iter and stop_split_at say, the cull rule is (100, 40), and the opacities are never reset
    (reset_opacities is the caller's).

    Rank-deterministic: the split / clone samples come from a counter-based generator keyed by (seed, step, Gaussian index,
    sample) -- with all-reduced statistics (mtgs_amd.dist.all_reduce_stats) every rank of a data-parallel job produces
    bit-identical tensors, so N stays identical without a broadcast (the reference draws torch.randn per rank, :642, :687).
    ONE host synchronisation: the survivor totals (tensor sizes).  Returns (new_params, new_moments | None, info) with
    info = {n_before, n_after, n_old_kept (old Gaussians kept), n_children (split children), n_dups, n_split (split parents),
    src_index, kind, extras}; every count is a host int (they come with the one host read).  N == 0: the empty result, without
    a launch or a host read.  n_split_samples outside 1..4: RuntimeError, before any launch.
    extras {name: [N, ...] tensor of a 4-byte dtype}: moved like a parameter (a child / duplicate takes its parent's row) and
    returned in info["extras"] -- the row-lazy optimizer's `last` stamps.  before_rows(parents bool [N]): called (N > 0) after the
    decisions are known and before any row is copied, with the Gaussians that get children or a duplicate -- a caller whose rows are
    lazy brings THOSE rows up to date there (FusedAdam.catch_up_rows) instead of flushing every row.
    The four GEOMETRY tensors (means, scales, quats, opacities) must be CURRENT when this function is called: the split / cull
    decisions and the children's positions are computed from them before the hook runs, so the hook is only good for tensors that
    are copied afterwards (colours, extras).  A caller whose geometry rows are lazy flushes them first."""
    if not 1 <= int(cfg.n_split_samples) <= 4:
        raise RuntimeError(f"refine_gaussians: n_split_samples={cfg.n_split_samples} outside 1..4")
    node = NodeRefine(params, stats, cfg, seed, moments=moments, extras=extras)
    hook = None if before_rows is None else (lambda masks: before_rows(masks[0]))
    res = _refine_nodes([node], [(_DENSIFY, False)], step, hook, "refine_gaussians")[0]
    if res is not None:
        return res
    empty = lambda t: t.new_empty((0,) + tuple(t.shape[1:]))
    info = {"n_before": 0, "n_after": 0, "n_old_kept": 0, "n_children": 0, "n_dups": 0, "n_split": 0,
            "src_index": params["means"].new_empty(0, dtype=torch.int32), "kind": params["means"].new_empty(0, dtype=torch.uint8),
            "extras": {k: empty(t) for k, t in (extras or {}).items()}}
    return ({k: empty(t) for k, t in params.items()},
            None if moments is None else {k: (empty(a), empty(b)) for k, (a, b) in moments.items()}, info)
