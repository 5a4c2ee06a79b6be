"""The two references of mtgs_amd.present (tests/test_present_host.py, tests/test_gpu_present.py).

(a) the specification of include/mtgs_present.h in executable form: NumPy, fp32, ONE rounded operation per line, with the
    layouts, the padding and both quantisations (`panel_np`, `frame_np`, `depth_resize_np`);
(b) a transcription in torch of what it restates, device-agnostic: nerfstudio's colormaps.py (`ns_*`, recalled from version 1.1.5,
    which is not part of the reference tree) and the frame code of the viewer and of the render tool (`viewer_frame_torch`,
    `viewer_depth_torch`, `render_frame_torch`), host reads and the per-call table upload included.

A panel, for (a): a dict with kind ("rgb" | "float" | "depth" | "bool"), src (NumPy [H, W, C]), and for the mapped kinds lut
([256, 3] float32 or None for gray), normalize, cmin, cmax, invert; for depth also acc ([H, W, 1] or None), near, far (None = from
the data)."""
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

f32 = np.float32
GOLDEN = Path(__file__).resolve().parent / "golden" / "colormap_luts.npz"
SPLIT_COLOR = (0.133, 0.157, 0.192)


def tables():
    """{name: [256, 3] float32} of tests/golden/colormap_luts.npz"""
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


# ---- (a) the NumPy restatement ---------------------------------------------------------------------------------------------------
def clip01(v):
    """v < 0 -> 0, v > 1 -> 1, NaN kept"""
    return np.where(v < f32(0), f32(0), np.where(v > f32(1), f32(1), v)).astype(f32)


def extrema(a):
    """(min, max) as torch.min / torch.max: NaN if any element is"""
    return f32(np.min(a)), f32(np.max(a))


def panel(kind, src, lut=None, normalize=False, cmin=0.0, cmax=1.0, invert=False, acc=None, near=None, far=None):
    return dict(kind=kind, src=src, lut=lut, normalize=normalize, cmin=cmin, cmax=cmax, invert=invert, acc=acc, near=near, far=far)


def panel_np(p, shift=0, want_t=False):
    """float32 [H, W, 3] of the whole source of panel p.  `shift` moves every table index by that much (kept inside the table):
    what a neighbouring index would have shown.  want_t: also t = v * 255 [H, W] (None for the unmapped kinds)."""
    src = p["src"]
    with np.errstate(all="ignore"):
        if p["kind"] == "rgb":
            out, t = src.astype(f32), None
        elif p["kind"] == "bool":
            out, t = np.repeat((src != 0).astype(f32), 3, axis=-1), None
        else:
            v = src[..., 0].astype(f32)
            if p["kind"] == "depth":
                mn, mx = extrema(v)
                near = float(mn) if p["near"] is None else float(p["near"])
                far = float(mx) if p["far"] is None else float(p["far"])
                D = (far - near) + 1e-10                                   # double
                inv = f32(1.0) / f32(D)
                v = v - f32(near)
                v = v * inv
                v = clip01(v)
            if p["normalize"]:
                lo, hi = extrema(v)
                v = v - lo
                top = f32(hi - lo)                                         # the max of the shifted values
                den = f32(top + f32(1e-9))
                v = (v / den).astype(f32)
            v = v * f32(float(p["cmax"]) - float(p["cmin"]))
            v = v + f32(p["cmin"])
            v = clip01(v)
            if p["invert"]:
                v = f32(1) - v
            v = np.where(np.isnan(v), f32(0), v).astype(f32)
            t = (v * f32(255)).astype(f32)
            if p["lut"] is None:
                out = np.repeat(v[..., None], 3, axis=-1)
            else:
                out = p["lut"][np.clip(t.astype(np.int64) + shift, 0, 255)].astype(f32)
            if p["kind"] == "depth" and p["acc"] is not None:
                a = p["acc"].astype(f32)
                oma = f32(1) - a
                out = out * a
                out = out + oma
    return (out, t) if want_t else out


def quantise_np(x, mode):
    """uint8 of a float frame: mode "truncate" or "round"; clamped to [0, 1] first, NaN -> 0"""
    x = np.where(np.isnan(x), f32(0), clip01(x)).astype(f32)
    x = x * f32(255)
    if mode == "round":
        x = x + f32(0.5)
    return x.astype(np.uint8)


def frame_np(panels, places, out_h, out_w, split_column=-1, fmt="truncate", shift=0):
    """The whole frame: places[j] = (y0, x0, h, w, src_x0) of panels[j]; uncovered pixels 0; column split_column, where covered,
    SPLIT_COLOR.  fmt "float" | "truncate" | "round".  Also returns the threshold map: where t = v * 255 of the pixel shown lies
    within 4 ulp of an integer."""
    frame = np.zeros((out_h, out_w, 3), dtype=f32)
    covered = np.zeros((out_h, out_w), dtype=bool)
    threshold = np.zeros((out_h, out_w), dtype=bool)
    for p, (y0, x0, h, w, sx) in reversed(list(zip(panels, places))):        # the first panel of the table wins
        colors, t = panel_np(p, shift, want_t=True)
        frame[y0:y0 + h, x0:x0 + w] = colors[:h, sx:sx + w]
        covered[y0:y0 + h, x0:x0 + w] = True
        if t is None:
            threshold[y0:y0 + h, x0:x0 + w] = False
        else:
            t = t[:h, sx:sx + w]
            threshold[y0:y0 + h, x0:x0 + w] = np.abs(t - np.rint(t)) <= f32(4) * np.spacing(np.maximum(np.abs(t), np.rint(t)).astype(f32))
    if split_column >= 0:
        rows = covered[:, split_column]
        frame[rows, split_column] = np.array(SPLIT_COLOR, dtype=f32)
        threshold[:, split_column] = False
    return (frame if fmt == "float" else quantise_np(frame, fmt)), threshold


def depth_resize_np(depth, out_h, out_w, scale):
    """torch's upsample_bilinear2d (align_corners = False) of depth [H, W], times scale; also the (min, max) of the four taps"""
    H, W = depth.shape

    def axis(n_in, n_out):
        r = f32(n_in) / f32(n_out)
        s = r * (np.arange(n_out, dtype=f32) + f32(0.5))
        s = s - f32(0.5)
        s = np.maximum(s, f32(0))
        i0 = s.astype(np.int64)
        i1 = i0 + (i0 < n_in - 1)
        l1 = s - i0.astype(f32)
        return i0, i1, f32(1) - l1, l1
    y0, y1, h0, h1 = axis(H, out_h)
    x0, x1, w0, w1 = axis(W, out_w)
    a, b, c, d = depth[y0][:, x0], depth[y0][:, x1], depth[y1][:, x0], depth[y1][:, x1]
    top = w0 * a
    top = top + w1 * b
    bottom = w0 * c
    bottom = bottom + w1 * d
    v = h0[:, None] * top
    v = v + h1[:, None] * bottom
    taps = np.stack([a, b, c, d])
    return (v * f32(scale)).astype(f32), taps.min(0), taps.max(0)


# ---- (b) nerfstudio's colormaps.py, transcribed -----------------------------------------------------------------------------------
class NSColormapOptions:
    def __init__(self, colormap="default", normalize=False, colormap_min=0, colormap_max=1, invert=False):
        self.colormap, self.normalize, self.colormap_min, self.colormap_max, self.invert = colormap, normalize, colormap_min, colormap_max, invert


_COLOR_LISTS = {}


def _colors(name):
    """stands for matplotlib.colormaps[name].colors: a Python list of 256 [r, g, b] lists (the tables of the golden file)"""
    if not _COLOR_LISTS:
        _COLOR_LISTS.update({k: v.astype(np.float64).tolist() for k, v in tables().items()})
    return _COLOR_LISTS[name]


def ns_apply_float_colormap(image, colormap="viridis"):
    if colormap == "default":
        colormap = "turbo"
    image = torch.nan_to_num(image, 0)
    if colormap == "gray":
        return image.repeat(1, 1, 3)
    image_long = (image * 255).long()
    image_long_min = torch.min(image_long)
    image_long_max = torch.max(image_long)
    assert image_long_min >= 0, f"the min value is {image_long_min}"
    assert image_long_max <= 255, f"the max value is {image_long_max}"
    return torch.tensor(_colors(colormap), device=image.device)[image_long[..., 0]]


def ns_apply_boolean_colormap(image):
    colored_image = torch.ones(image.shape[:-1] + (3,), device=image.device)
    colored_image[image[..., 0], :] = torch.tensor([1.0, 1.0, 1.0], device=image.device)
    colored_image[~image[..., 0], :] = torch.tensor([0.0, 0.0, 0.0], device=image.device)
    return colored_image


def ns_apply_colormap(image, colormap_options=None, eps=1e-9):
    colormap_options = colormap_options or NSColormapOptions()
    if image.shape[-1] == 3:
        return image
    if image.shape[-1] == 1 and torch.is_floating_point(image):
        output = image
        if colormap_options.normalize:
            output = output - torch.min(output)
            output = output / (torch.max(output) + eps)
        output = output * (colormap_options.colormap_max - colormap_options.colormap_min) + colormap_options.colormap_min
        output = torch.clip(output, 0, 1)
        if colormap_options.invert:
            output = 1 - output
        return ns_apply_float_colormap(output, colormap=colormap_options.colormap)
    if image.dtype == torch.bool:
        return ns_apply_boolean_colormap(image)
    if image.shape[-1] > 3:
        raise NotImplementedError("apply_pca_colormap")
    raise NotImplementedError


def ns_apply_depth_colormap(depth, accumulation=None, near_plane=None, far_plane=None, colormap_options=None):
    near_plane = near_plane if near_plane is not None else float(torch.min(depth))
    far_plane = far_plane if far_plane is not None else float(torch.max(depth))
    depth = (depth - near_plane) / (far_plane - near_plane + 1e-10)
    depth = torch.clip(depth, 0, 1)
    colored_image = ns_apply_colormap(depth, colormap_options=colormap_options)
    if accumulation is not None:
        colored_image = colored_image * accumulation + (1 - accumulation)
    return colored_image


# ---- (b) the frame code of the viewer and of the render tool, transcribed -----------------------------------------------------------
def viewer_frame_torch(outputs, output_render, options, split_output_render=None, split_options=None, split_percentage=0.5,
                       client_aspect=None):
    """render_state_machine.py:255-296 -> NumPy uint8"""
    selected_output = ns_apply_colormap(image=outputs[output_render], colormap_options=options)
    if split_output_render is not None:
        split_output = ns_apply_colormap(image=outputs[split_output_render], colormap_options=split_options)
        split_index = min(int(split_percentage * selected_output.shape[1]), selected_output.shape[1] - 1)
        selected_output = torch.cat([selected_output[:, :split_index], split_output[:, split_index:]], dim=1)
        selected_output[:, split_index] = torch.tensor([0.133, 0.157, 0.192], device=selected_output.device)
    selected_output = (selected_output * 255).type(torch.uint8)
    selected_output = selected_output.cpu().numpy()
    assert selected_output.shape[-1] == 3
    if client_aspect is not None:
        current_h, current_w = selected_output.shape[:2]
        desired_aspect = client_aspect
        pad_width = int(max(0, (desired_aspect * current_h - current_w) // 2))
        pad_height = int(max(0, (current_w / desired_aspect - current_h) // 2))
        if pad_width > 5 or pad_height > 5:
            selected_output = np.pad(selected_output, ((pad_height, pad_height), (pad_width, pad_width), (0, 0)), mode="constant",
                                     constant_values=0)
    return selected_output


def viewer_depth_torch(depth, state):
    """render_state_machine.py:180-190 -> the gl_z_buf_depth tensor [h, w, 1] (before `.cpu().numpy() * viser_scale_ratio`)"""
    desired_depth_pixels = {"low_move": 128, "low_static": 128, "high": 512}[state] ** 2
    current_depth_pixels = depth.shape[0] * depth.shape[1]
    scale = min(desired_depth_pixels / max(1, current_depth_pixels), 1.0)
    return F.interpolate(depth.squeeze(dim=-1)[None, None, ...], size=(int(depth.shape[0] * scale), int(depth.shape[1] * scale)),
                         mode="bilinear")[0, 0, :, :, None]


def render_frame_torch(outputs, rendered_output_names, depth_near_plane=None, depth_far_plane=None, options=None):
    """tools/render.py:131-165 -> the concatenated float frame as NumPy, and its uint8 by the rounding rule"""
    render_image = []
    for rendered_output_name in rendered_output_names:
        output_image = outputs[rendered_output_name]
        is_depth = rendered_output_name.find("depth") != -1
        if is_depth:
            output_image = ns_apply_depth_colormap(output_image, accumulation=outputs["accumulation"], near_plane=depth_near_plane,
                                                   far_plane=depth_far_plane, colormap_options=options).cpu().numpy()
        else:
            output_image = ns_apply_colormap(image=output_image, colormap_options=options).cpu().numpy()
        render_image.append(output_image)
    render_image = np.concatenate(render_image, axis=1)
    return render_image, (np.clip(render_image, 0.0, 1.0) * f32(255) + f32(0.5)).astype(np.uint8)
