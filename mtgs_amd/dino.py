"""The DINOv2 similarity metric on the device (include/mtgs_dino.h, csrc/dino.hip): what mtgs/utils/dinov2.py's
DINOv2Similarity.similarity computes under the key dinov2_sim in mtgs_scene_graph.py's get_metrics_dict and
get_image_metrics_and_images -- without its three host round trips and its .item().

    w = DinoWeights.from_state_dict(torch.hub.load("facebookresearch/dinov2", "dinov2_vitb14").state_dict(), device="cuda")   # once
    s = dino_similarity(pred, gt, mask, weights=w)                   # 0-dim fp32 device tensor; float(s) is the caller's choice
    image_metrics(pred, gt, mask, dino_weights=w)["dinov2_sim"]      # the same number under MTGS's key

Forward only, no host read (graph-capturable), no atomics (bitwise reproducible), about 7 launches per block.  Pillow's two-pass
integer BILINEAR resample, the centre crop and the mask's NEAREST resize run on the device from coefficient tables that this module
builds on the host in double, once per (H, W, S), and keeps on the device (as present.py keeps a colour table).

[RECALL] Three things are recalled, not checked -- neither torchvision nor the DINOv2 hub code was available to run: torchvision's
to_pil_image / Resize / CenterCrop / ToTensor / Normalize (the output size, the crop offsets, the byte conversion), the hub model's
forward_features (include/mtgs_dino.h states it, tests/dino_refs.py restates it in fp64), and the hub state-dict key names that
from_state_dict reads.  Pillow's resampling is restated and compared with Pillow bit for bit (tests/test_dino_host.py).
The clamp of the image to [0, 1] before the byte conversion is ours: the reference's mul(255).byte() wraps outside that range.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from ._abi import header_abi
from ._inputs import as_f32, image_pair, mask_u8
from ._lib import call, ptr, require_gpu, scratch, size_query, stream_of

_ABI = header_abi("mtgs_dino.h")
_CONFIG = _ABI.structs["mtgs_dino_config"]
PATCH = _ABI.constants["MTGS_DINO_PATCH"]
HEAD_DIM = _ABI.constants["MTGS_DINO_HEAD_DIM"]
MAX_DIM = _ABI.constants["MTGS_DINO_MAX_DIM"]
EPILOGUES = {"bias": _ABI.constants["MTGS_DINO_EPI_BIAS"], "gelu": _ABI.constants["MTGS_DINO_EPI_BIAS_GELU"],
             "scale_residual": _ABI.constants["MTGS_DINO_EPI_SCALE_RESIDUAL"], "patch_embed": _ABI.constants["MTGS_DINO_EPI_PATCH_EMBED"]}
PRECISION_BITS = 22                # Pillow's 8-bit resampling: coefficients are int(w * 2^22 + 0.5)


@dataclass(frozen=True)
class DinoConfig:
    """The network's shape.  The hub's dinov2_vitb14 is the default: 768 / 12 / 12 / 14 / 518."""
    dim: int = 768
    heads: int = 12
    depth: int = 12
    patch: int = PATCH
    image: int = 518
    mlp_ratio: int = 4
    ln_eps: float = 1e-6

    def __post_init__(self):
        if self.patch != PATCH:
            raise NotImplementedError(f"patch = {self.patch}: only {PATCH} is implemented")
        if self.mlp_ratio != 4:
            raise NotImplementedError(f"mlp_ratio = {self.mlp_ratio}: only 4 is implemented")
        if self.dim <= 0 or self.heads <= 0 or self.depth <= 0 or self.dim != self.heads * HEAD_DIM:
            raise NotImplementedError(f"dim / heads = {self.dim} / {self.heads}: the head dimension must be {HEAD_DIM}")
        if self.dim > MAX_DIM:
            raise NotImplementedError(f"dim = {self.dim} exceeds {MAX_DIM}")
        if self.image <= 0 or self.image % self.patch != 0:
            raise ValueError(f"image = {self.image} must be a positive multiple of the patch {self.patch}")

    @property
    def grid(self) -> int:
        return self.image // self.patch

    @property
    def patches(self) -> int:
        return self.grid * self.grid

    @property
    def tokens(self) -> int:
        return 1 + self.patches

    def struct(self) -> np.ndarray:
        """HOST mtgs_dino_config"""
        c = np.zeros((), dtype=_CONFIG)
        for k in ("dim", "heads", "depth", "patch", "image", "mlp_ratio", "ln_eps"):
            c[k] = getattr(self, k)
        return c


def _cfg_ptr(c: np.ndarray):
    return c.ctypes.data


# ---- weights ---------------------------------------------------------------------------------------------------------------------
# (key, kind) in the order of the flat array; kind: "vec" as it is, "lin" = torch's [out, in] packed to [in][out], "conv" = the patch
# embedding's [dim, 3, 14, 14] packed to [588][dim]
_HEAD_KEYS = (("patch_embed.proj.weight", "conv"), ("patch_embed.proj.bias", "vec"), ("cls_token", "vec"), ("pos_embed", "vec"))
_BLOCK_KEYS = (("norm1.weight", "vec"), ("norm1.bias", "vec"), ("attn.qkv.weight", "lin"), ("attn.qkv.bias", "vec"), ("attn.proj.weight", "lin"),
               ("attn.proj.bias", "vec"), ("ls1.gamma", "vec"), ("norm2.weight", "vec"), ("norm2.bias", "vec"), ("mlp.fc1.weight", "lin"),
               ("mlp.fc1.bias", "vec"), ("mlp.fc2.weight", "lin"), ("mlp.fc2.bias", "vec"), ("ls2.gamma", "vec"))
_TAIL_KEYS = (("norm.weight", "vec"), ("norm.bias", "vec"))
IGNORED_KEYS = ("mask_token",)


def _layout(cfg: DinoConfig):
    """[(key, kind, torch shape)] in the order of the flat array"""
    d, h = cfg.dim, cfg.mlp_ratio * cfg.dim
    shapes = {"patch_embed.proj.weight": (d, 3, PATCH, PATCH), "patch_embed.proj.bias": (d,), "cls_token": (1, 1, d), "pos_embed": (1, cfg.tokens, d),
              "norm1.weight": (d,), "norm1.bias": (d,), "attn.qkv.weight": (3 * d, d), "attn.qkv.bias": (3 * d,), "attn.proj.weight": (d, d),
              "attn.proj.bias": (d,), "ls1.gamma": (d,), "norm2.weight": (d,), "norm2.bias": (d,), "mlp.fc1.weight": (h, d), "mlp.fc1.bias": (h,),
              "mlp.fc2.weight": (d, h), "mlp.fc2.bias": (d,), "ls2.gamma": (d,), "norm.weight": (d,), "norm.bias": (d,)}
    out = [(k, kind, shapes[k]) for k, kind in _HEAD_KEYS]
    for i in range(cfg.depth):
        out += [(f"blocks.{i}.{k}", kind, shapes[k]) for k, kind in _BLOCK_KEYS]
    return out + [(k, kind, shapes[k]) for k, kind in _TAIL_KEYS]


def _pack(t: Tensor, kind: str) -> Tensor:
    t = t.detach().to(torch.float32)
    if kind == "lin":
        return t.t().contiguous().reshape(-1)
    if kind == "conv":
        return t.reshape(t.shape[0], -1).t().contiguous().reshape(-1)
    return t.contiguous().reshape(-1)


def _unpack(flat: Tensor, kind: str, shape) -> Tensor:
    if kind == "lin":
        return flat.reshape(shape[1], shape[0]).t().contiguous()
    if kind == "conv":
        return flat.reshape(shape[1] * shape[2] * shape[3], shape[0]).t().contiguous().reshape(shape)
    return flat.reshape(shape).clone()


class DinoWeights:
    """One weight set, repacked once: `flat` is the array mtgs_dino_features / mtgs_dino_similarity read (include/mtgs_dino.h)."""

    def __init__(self, config: DinoConfig, flat: Tensor):
        self.config, self.flat = config, flat

    @property
    def device(self):
        return self.flat.device

    def to(self, device) -> "DinoWeights":
        return DinoWeights(self.config, self.flat.to(device))

    @staticmethod
    def infer_config(sd: Dict[str, Tensor]) -> DinoConfig:
        """The configuration a hub state dict implies, by shapes; names what this implementation refuses."""
        if "register_tokens" in sd:
            raise NotImplementedError("register_tokens: the register-token variants (dinov2_vit*_reg) are not implemented")
        swiglu = [k for k in sd if ".mlp.w12." in k or ".mlp.w3." in k]
        if swiglu:
            raise NotImplementedError(f"{swiglu[0]}: SwiGLU MLPs (mlp.w12 / mlp.w3, as in dinov2_vitg14) are not implemented")
        for k in ("patch_embed.proj.weight", "pos_embed", "cls_token", "blocks.0.attn.qkv.weight", "norm.weight"):
            if k not in sd:
                raise KeyError(f"{k}: not in the state dict (keys are expected under the hub model's names, e.g. blocks.0.attn.qkv.weight)")
        w = sd["patch_embed.proj.weight"]
        if w.dim() != 4 or w.shape[1] != 3 or tuple(w.shape[2:]) != (PATCH, PATCH):
            raise NotImplementedError(f"patch_embed.proj.weight {tuple(w.shape)}: only a {PATCH} x {PATCH} embedding of 3 channels is implemented")
        dim = w.shape[0]
        if dim % HEAD_DIM != 0:
            raise NotImplementedError(f"dim = {dim} is not a multiple of the head dimension {HEAD_DIM}")
        depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks.") and k.split(".")[1].isdigit())
        tokens = sd["pos_embed"].shape[-2]
        grid = int(round((tokens - 1) ** 0.5))
        if sd["pos_embed"].dim() != 3 or grid < 1 or grid * grid != tokens - 1:
            raise ValueError(f"pos_embed {tuple(sd['pos_embed'].shape)}: its length is not 1 + G^2")
        hidden = sd["blocks.0.mlp.fc1.weight"].shape[0] if "blocks.0.mlp.fc1.weight" in sd else 4 * dim
        if hidden != 4 * dim:
            raise NotImplementedError(f"blocks.0.mlp.fc1.weight has {hidden} rows: mlp_ratio = {hidden / dim:g}, only 4 is implemented")
        return DinoConfig(dim=dim, heads=dim // HEAD_DIM, depth=depth, image=grid * PATCH)

    @classmethod
    def from_state_dict(cls, sd: Dict[str, Tensor], device=None, config: Optional[DinoConfig] = None) -> "DinoWeights":
        """[RECALL] sd under the hub model's key names (module docstring).  The configuration is inferred from the shapes unless
        given; `config.image` other than the pos_embed's grid is refused, because pos_embed is added WITHOUT interpolation."""
        inferred = cls.infer_config(sd)
        cfg = inferred if config is None else config
        if "pos_embed" in sd and sd["pos_embed"].shape[-2] != cfg.tokens:
            raise NotImplementedError(f"pos_embed has {sd['pos_embed'].shape[-2]} tokens, the configuration 1 + {cfg.grid}^2 = {cfg.tokens}: "
                                      "interpolated position embeddings are not implemented")
        if (cfg.dim, cfg.depth) != (inferred.dim, inferred.depth):
            raise ValueError(f"the state dict is {inferred.dim} wide and {inferred.depth} deep, the configuration {cfg.dim} and {cfg.depth}")
        parts = []
        for key, kind, shape in _layout(cfg):
            if key not in sd:
                raise KeyError(f"{key}: not in the state dict")
            if tuple(sd[key].shape) != tuple(shape):
                raise ValueError(f"{key}: shape {tuple(sd[key].shape)}, expected {tuple(shape)}")
            parts.append(_pack(sd[key], kind))
        known = {k for k, _, _ in _layout(cfg)} | set(IGNORED_KEYS)
        unknown = sorted(k for k in sd if k not in known)
        if unknown:
            raise NotImplementedError(f"{unknown[0]}: a parameter this implementation does not know ({len(unknown)} such keys)")
        flat = torch.cat([p.to(parts[0].device) for p in parts]).contiguous()
        return cls(cfg, flat if device is None else flat.to(device))

    def to_state_dict(self) -> Dict[str, Tensor]:
        """The inverse of from_state_dict (without mask_token), on `flat`'s device."""
        out, o = {}, 0
        for key, kind, shape in _layout(self.config):
            n = int(np.prod(shape))
            out[key] = _unpack(self.flat[o:o + n], kind, shape)
            o += n
        assert o == self.flat.numel()
        return out

    def tensor(self, key: str) -> Tensor:
        """The packed form of one parameter, as a view of `flat` ([K, N] for a linear layer)."""
        o = 0
        for k, kind, shape in _layout(self.config):
            n = int(np.prod(shape))
            if k == key:
                v = self.flat[o:o + n]
                if kind == "lin":
                    return v.view(shape[1], shape[0])
                if kind == "conv":
                    return v.view(3 * PATCH * PATCH, shape[0])
                return v.view(shape[-2], shape[-1]) if key == "pos_embed" else v
            o += n
        raise KeyError(key)


# ---- the resampling tables (HOST, double) -------------------------------------------------------------------------------------------
def resized_size(H: int, W: int, S: int) -> Tuple[int, int]:
    """[RECALL] torchvision's Resize(S): the short side becomes S, the long one int(S * long / short)"""
    if H <= W:
        return (S, int(S * W / H)) if H != S else (H, W)
    return (int(S * H / W), S) if W != S else (H, W)


def crop_offset(size: int, S: int) -> int:
    """[RECALL] torchvision's CenterCrop: int(round((size - S) / 2.0)), Python's round (half to even)"""
    return int(round((size - S) / 2.0))


def bilinear_weights(in_size: int, out_size: int, first: int, count: int):
    """Pillow's precompute_coeffs for the BILINEAR filter, outputs first .. first + count - 1: (bounds [count, 2] int32 =
    (xmin, taps), weights [count, ksize] float64), the normalised double weights its 32-bit ("F") resampling multiplies by."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ss = 1.0 / fs
    ksize = int(np.ceil(support)) * 2 + 1
    bounds = np.zeros((count, 2), np.int32)
    weights = np.zeros((count, ksize), np.float64)
    for j in range(count):
        center = (first + j + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = np.maximum(0.0, 1.0 - np.abs((np.arange(xmax) + xmin - center + 0.5) * ss))
        ww = 0.0                               # Pillow adds them one by one in this order (numpy's sum is pairwise beyond 8 taps)
        for v in w:
            ww += v
        if ww != 0.0:
            w = w / ww
        bounds[j] = (xmin, xmax)
        weights[j, :xmax] = w
    taps = max(1, int(bounds[:, 1].max()))
    return bounds, np.ascontiguousarray(weights[:, :taps])


def bilinear_coefficients(in_size: int, out_size: int, first: int, count: int):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for the BILINEAR filter, outputs first .. first + count - 1:
    (bounds [count, 2] int32 = (xmin, taps), coefficients [count, ksize] int32)."""
    bounds, weights = bilinear_weights(in_size, out_size, first, count)
    coef = np.zeros(weights.shape, np.int32)
    for j in range(count):                     # int(0.5 + w * 2^22): the weights are >= 0, so the truncation is a floor
        coef[j, :bounds[j, 1]] = [int(0.5 + v * (1 << PRECISION_BITS)) for v in weights[j, :bounds[j, 1]]]
    return bounds, coef


def nearest_sources(in_size: int, out_size: int, first: int, count: int) -> np.ndarray:
    """Pillow's NEAREST resize: int(xo), xo = 0.5 * in / out advanced by REPEATED ADDITION of in / out in double"""
    step = in_size / out_size
    xo = step * 0.5
    out = np.zeros(count, np.int32)
    for j in range(first + count):
        if j >= first:
            out[j - first] = min(int(xo), in_size - 1)
        xo += step
    return out


def resample_tables(H: int, W: int, S: int):
    """(tables int32 [S * (6 + hk + vk)], hk, vk) of include/mtgs_dino.h for an H x W image and an S x S window"""
    oh, ow = resized_size(H, W, S)
    top, left = crop_offset(oh, S), crop_offset(ow, S)
    hb, hc = bilinear_coefficients(W, ow, left, S)
    vb, vc = bilinear_coefficients(H, oh, top, S)
    mx, my = nearest_sources(W, ow, left, S), nearest_sources(H, oh, top, S)
    flat = np.concatenate([a.reshape(-1) for a in (hb, hc, vb, vc, mx, my)]).astype(np.int32)
    return flat, hc.shape[1], vc.shape[1]


_tables: dict = {}          # (H, W, S, device) -> (int32 device tensor, hk, vk)


def _device_tables(H: int, W: int, S: int, device):
    key = (H, W, S, device)
    t = _tables.get(key)
    if t is None:
        if H < 1 or W < 1:
            raise ValueError(f"a {H} x {W} image")
        flat, hk, vk = resample_tables(H, W, S)
        dev = torch.empty(flat.size, dtype=torch.int32, device=device)
        dev.copy_(torch.from_numpy(flat))           # a blocking copy: the tables are complete before anything is captured
        t = _tables[key] = (dev, hk, vk)
    return t


def workspace_bytes(cfg: DinoConfig) -> int:
    c = cfg.struct()                                # alive until the call returns
    return size_query("mtgs_dino_workspace_bytes", _cfg_ptr(c))


def _scratch(cfg: DinoConfig, device, stream) -> Tensor:
    return scratch(("dino", cfg), lambda: workspace_bytes(cfg), device, stream)


# ---- the operators -----------------------------------------------------------------------------------------------------------------
def _images(pred: Tensor, gt: Tensor, mask: Optional[Tensor]):
    pred_c, gt_c, mask_c = image_pair(pred, gt, mask, metric="dinov2_sim")
    if pred_c.numel() == 0:
        raise ValueError(f"pred must have at least one pixel, got {tuple(pred.shape)}")
    return pred_c, gt_c, mask_c


def _check_weights(weights: "DinoWeights", device) -> None:
    if not isinstance(weights, DinoWeights):
        raise TypeError(f"weights must be a DinoWeights, got {type(weights).__name__}")
    if weights.device != device:
        raise RuntimeError(f"weights are on {weights.device}, the images on {device}: move them once with weights.to(device)")


def dino_preprocess(pred: Tensor, gt: Tensor, size: int = 518, return_bytes: bool = False):
    """Step 1 alone: the patch matrix [2 * G^2, 588] (and, if asked, the resized and cropped bytes [2, S, S, 3])."""
    pred_c, gt_c, _ = _images(pred, gt, None)
    if size <= 0 or size % PATCH != 0:
        raise ValueError(f"size = {size} must be a positive multiple of the patch {PATCH}")
    H, W = pred_c.shape[:2]
    tables, hk, vk = _device_tables(H, W, size, pred_c.device)
    G = size // PATCH
    patches = torch.empty(2 * G * G, 3 * PATCH * PATCH, dtype=torch.float32, device=pred_c.device)
    out_bytes = torch.empty(2, size, size, 3, dtype=torch.uint8, device=pred_c.device) if return_bytes else None
    call("mtgs_dino_preprocess", H, W, size, ptr(pred_c), ptr(gt_c), ptr(tables), hk, vk, ptr(out_bytes), ptr(patches), stream_of(pred_c))
    return (patches, out_bytes) if return_bytes else patches


def dino_patch_weights(mask: Optional[Tensor], H: int, W: int, size: int = 518, device=None) -> Tensor:
    """Step 2 alone: [G^2 + 1] = the patch weights and their sum.  mask [H, W] or [H, W, 1] bool / uint8, or None (all visible)."""
    if size <= 0 or size % PATCH != 0:
        raise ValueError(f"size = {size} must be a positive multiple of the patch {PATCH}")
    if mask is not None and mask.numel() != H * W:
        raise ValueError(f"mask must have H * W = {H * W} elements, got {tuple(mask.shape)}")
    require_gpu(mask)
    device = mask.device if mask is not None else torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise RuntimeError(f"mtgs_amd: tensors must live on the HIP device (torch device 'cuda'); got {device}")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    tables, hk, vk = _device_tables(H, W, size, device)
    G = size // PATCH
    out = torch.empty(G * G + 1, dtype=torch.float32, device=device)
    call("mtgs_dino_patch_weights", H, W, size, ptr(mask_u8(mask, H, W)), ptr(tables), hk, vk, ptr(out), torch.cuda.current_stream(device).cuda_stream)
    return out


def dino_linear(a: Tensor, w: Tensor, bias: Tensor, epilogue: str = "bias", *, gamma: Optional[Tensor] = None, residual: Optional[Tensor] = None,
                pos: Optional[Tensor] = None, cls: Optional[Tensor] = None) -> Tensor:
    """mtgs_dino_linear alone: a [M, K] x packed w [K, N].  epilogue "bias" | "gelu" | "scale_residual" (gamma [N], residual [M, N]:
    returns residual + gamma * (a w + bias), in a copy) | "patch_embed" (pos [T, N], cls [N], M = 2 (T - 1): returns [2 T, N])."""
    if epilogue not in EPILOGUES:
        raise ValueError(f"epilogue must be one of {sorted(EPILOGUES)}, got {epilogue!r}")
    if a.dim() != 2 or w.dim() != 2 or a.shape[1] != w.shape[0]:
        raise ValueError(f"a {tuple(a.shape)} and w {tuple(w.shape)} must be [M, K] and [K, N]")
    M, K = a.shape
    N = w.shape[1]
    if N % 64 != 0:
        raise NotImplementedError(f"N = {N} is not a multiple of 64")
    if K % 4 != 0:
        raise NotImplementedError(f"K = {K} is not a multiple of 4")
    if bias.numel() != N:
        raise ValueError(f"bias has {bias.numel()} elements for N = {N}")
    require_gpu(a, w, bias, gamma, residual, pos, cls)
    a = as_f32(a)                                  # no copy of an fp32 contiguous array, whatever its alignment
    w_c, bias_c = as_f32(w), as_f32(bias)
    tokens, gamma_c, pos_c, cls_c = 0, None, None, None
    if epilogue == "scale_residual":
        if gamma is None or residual is None or gamma.numel() != N or tuple(residual.shape) != (M, N):
            raise ValueError("scale_residual takes gamma [N] and residual [M, N]")
        gamma_c = as_f32(gamma)
        out = residual.to(torch.float32).clone(memory_format=torch.contiguous_format)
    elif epilogue == "patch_embed":
        if pos is None or cls is None or pos.dim() != 2 or pos.shape[1] != N or cls.numel() != N or M != 2 * (pos.shape[0] - 1):
            raise ValueError("patch_embed takes pos [T, N], cls [N] and M = 2 (T - 1) rows")
        tokens, pos_c, cls_c = pos.shape[0], as_f32(pos), as_f32(cls)
        out = torch.empty(2 * tokens, N, dtype=torch.float32, device=a.device)
    else:
        out = torch.empty(M, N, dtype=torch.float32, device=a.device)
    call("mtgs_dino_linear", M, K, N, ptr(a), ptr(w_c), ptr(bias_c), EPILOGUES[epilogue], ptr(gamma_c), ptr(pos_c), ptr(cls_c), tokens, ptr(out),
         stream_of(a))
    return out


def dino_layernorm(x: Tensor, weight: Tensor, bias: Tensor, eps: float = 1e-6) -> Tensor:
    """mtgs_dino_layernorm alone on the rows of x [M, D]"""
    if x.dim() != 2:
        raise ValueError(f"x must be [M, D], got {tuple(x.shape)}")
    M, D = x.shape
    if D % 64 != 0 or D > MAX_DIM:
        raise NotImplementedError(f"D = {D} must be a multiple of 64, at most {MAX_DIM}")
    if weight.numel() != D or bias.numel() != D:
        raise ValueError(f"weight and bias must have D = {D} elements")
    require_gpu(x, weight, bias)
    x_c = as_f32(x)
    out = torch.empty_like(x_c)
    call("mtgs_dino_layernorm", M, D, float(eps), ptr(x_c), ptr(as_f32(weight)), ptr(as_f32(bias)), ptr(out), stream_of(x_c))
    return out


def dino_attention(qkv: Tensor, heads: int) -> Tensor:
    """mtgs_dino_attention alone: qkv [n, T, 3 * heads * 64] (per row q | k | v) -> [n, T, heads * 64]"""
    if qkv.dim() != 3 or qkv.shape[2] != 3 * heads * HEAD_DIM:
        raise ValueError(f"qkv must be [n, T, 3 * {heads} * {HEAD_DIM}], got {tuple(qkv.shape)}")
    require_gpu(qkv)
    q = as_f32(qkv)
    n, T, _ = q.shape
    out = torch.empty(n, T, heads * HEAD_DIM, dtype=torch.float32, device=q.device)
    call("mtgs_dino_attention", n, T, heads, ptr(q), ptr(out), stream_of(q))
    return out


def dino_tail(features: Tensor, patch_weights: Tensor) -> Tensor:
    """Step 4 alone: features [2, G^2, D], patch_weights [G^2 + 1] (the weights and their sum) -> the 0-dim result"""
    if features.dim() != 3 or features.shape[0] != 2 or patch_weights.numel() != features.shape[1] + 1:
        raise ValueError(f"features {tuple(features.shape)} must be [2, G^2, D] and patch_weights {tuple(patch_weights.shape)} [G^2 + 1]")
    if features.shape[2] > MAX_DIM:
        raise NotImplementedError(f"D = {features.shape[2]} exceeds {MAX_DIM}")
    require_gpu(features, patch_weights)
    f, w = as_f32(features), as_f32(patch_weights)
    G2, D = f.shape[1], f.shape[2]
    scratch = torch.empty(G2, dtype=torch.float32, device=f.device)
    out = torch.empty((), dtype=torch.float32, device=f.device)
    call("mtgs_dino_tail", G2, D, ptr(f), ptr(f[1]), ptr(w), ptr(scratch), ptr(out), stream_of(f))
    return out


def dino_features(pred: Tensor, gt: Tensor, *, weights: DinoWeights) -> Tensor:
    """Steps 1 and 3: forward_features(...)["x_norm_patchtokens"] of both images, [2, G^2, dim]"""
    pred_c, gt_c, _ = _images(pred, gt, None)
    _check_weights(weights, pred_c.device)
    cfg = weights.config
    H, W = pred_c.shape[:2]
    tables, hk, vk = _device_tables(H, W, cfg.image, pred_c.device)
    stream = stream_of(pred_c)
    ws = _scratch(cfg, pred_c.device, stream)
    out = torch.empty(2, cfg.patches, cfg.dim, dtype=torch.float32, device=pred_c.device)
    c = cfg.struct()                                # alive until the call returns
    call("mtgs_dino_features", _cfg_ptr(c), H, W, ptr(pred_c), ptr(gt_c), ptr(tables), hk, vk, ptr(weights.flat), ptr(out), ptr(ws),
         ws.numel(), stream)
    return out


def dino_similarity(pred: Tensor, gt: Tensor, mask: Optional[Tensor] = None, *, weights: DinoWeights) -> Tensor:
    """DINOv2Similarity.similarity(pred, gt, mask) of [H, W, 3] images in [0, 1] (clamped to it) and a mask [H, W, 1] or [H, W]
    bool or uint8 (non-zero = visible; None = all visible): the patch-weighted mean cosine similarity of the two images' patch
    features, exactly 0 when no pixel is visible.  Returns a 0-dim fp32 tensor on the images' device.  The tables are kept per
    (H, W, image size, device), the workspace per (device, stream, configuration)."""
    pred_c, gt_c, mask_c = _images(pred, gt, mask)
    _check_weights(weights, pred_c.device)
    cfg = weights.config
    H, W = pred_c.shape[:2]
    tables, hk, vk = _device_tables(H, W, cfg.image, pred_c.device)
    stream = stream_of(pred_c)
    ws = _scratch(cfg, pred_c.device, stream)
    out = torch.empty((), dtype=torch.float32, device=pred_c.device)
    c = cfg.struct()                                # alive until the call returns
    call("mtgs_dino_similarity", _cfg_ptr(c), H, W, ptr(pred_c), ptr(gt_c), ptr(mask_c), ptr(tables), hk, vk, ptr(weights.flat),
         ptr(out), ptr(ws), ws.numel(), stream)
    return out


__all__ = ["DinoConfig", "DinoWeights", "dino_preprocess", "dino_patch_weights", "dino_linear", "dino_layernorm", "dino_attention", "dino_features",
           "dino_tail", "dino_similarity", "resample_tables", "resized_size", "crop_offset", "bilinear_weights", "bilinear_coefficients", "nearest_sources", "PATCH",
           "HEAD_DIM", "MAX_DIM", "EPILOGUES"]
