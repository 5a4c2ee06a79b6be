"""A restatement of the DINOv2 similarity metric (include/mtgs_dino.h): the reference of tests/test_dino_host.py and
tests/test_gpu_dino.py.

  * sections 1-2 (image bytes, Pillow's BILINEAR resize, centre crop, normalisation; the mask's NEAREST resize and the patch weights)
    in NumPy, without PIL: integer arithmetic throughout, compared with Pillow bit for bit by tests/test_dino_host.py;
  * section 3 (the ViT) in torch.nn.functional on the CPU, fp64 or any dtype given;
  * section 4 with torch.nn.functional.cosine_similarity itself.

[RECALL] torchvision's transforms (output size, crop offsets, byte conversion), the hub model's forward_features and the hub
state-dict key names are recalled: neither torchvision nor the hub code was available to run.  Pillow's resampling is NOT recalled.

There are no trained weights here.  random_state_dict() draws seeded ones under the hub's key names: linear weights with std
1 / sqrt(fan_in), biases 0.1 randn, layer-scale gamma std 0.5, cls_token / pos_embed std 0.5, layer-norm weights 1 + 0.1 randn.  With these
the image matters: a 128 / 2 / 2 network on a random image against the same image with noise of at most +-40 / 255 per channel gives a
similarity of about 0.98 with per-patch cosines down to 0.96 (tests/test_dino_host.py::test_the_reference_discriminates).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

PATCH = 14
BITS = 22


# ---- sections 1-2 in NumPy -------------------------------------------------------------------------------------------------------
def to_bytes(img):
    """[H, W, 3] float32 in [0, 1] -> uint8: trunc(clamp(x, 0, 1) * 255), the product in fp32"""
    x = np.clip(np.asarray(img, np.float32), np.float32(0), np.float32(1)) * np.float32(255)
    return x.astype(np.uint8)


def resized_size(H, W, S):
    """(out_h, out_w): the short side becomes S, the long one int(S * long / short); unchanged when the short side is S"""
    short, long_ = (H, W) if H <= W else (W, H)
    if short == S:
        return H, W
    new_long = int(S * long_ / short)
    return (S, new_long) if H <= W else (new_long, S)


def crop_offset(size, S):
    return int(round((size - S) / 2.0))       # Python's round: half to even


def _coefficients(in_size, out_size):
    """per output position: (xmin, [quantised weights])"""
    scale = in_size / out_size
    fs = scale if scale > 1.0 else 1.0
    support, ss = fs, 1.0 / fs
    out = []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        xmin = xmin if xmin > 0 else 0
        xmax = int(center + support + 0.5)
        xmax = (xmax if xmax < in_size else in_size) - xmin
        w, ww = [], 0.0
        for x in range(xmax):
            v = (x + xmin - center + 0.5) * ss
            v = -v if v < 0 else v
            v = 1.0 - v if v < 1.0 else 0.0
            w.append(v)
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        out.append((xmin, [int(0.5 + v * (1 << BITS)) for v in w]))
    return out


def _pass(img, out_size, axis):
    """one pass of the two-pass resample along `axis` of a [h, w, c] uint8 array"""
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((out_size,) + src.shape[1:], np.uint8)
    for xx, (xmin, k) in enumerate(_coefficients(src.shape[0], out_size)):
        acc = np.full(src.shape[1:], 1 << (BITS - 1), np.int64)
        for j, kk in enumerate(k):
            acc += src[xmin + j] * kk
        out[xx] = np.clip(acc >> BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def bilinear_resize(img_u8, out_h, out_w):
    """Pillow's Image.resize((out_w, out_h), BILINEAR) of an 8-bit image: the horizontal pass, rounded to 8 bits, then the vertical"""
    h, w = img_u8.shape[:2]
    x = img_u8 if out_w == w else _pass(img_u8, out_w, 1)
    return x if out_h == h else _pass(x, out_h, 0)


def nearest_index(in_size, out_size, multiplied=False):
    """source index of Pillow's NEAREST resize per output position: repeated addition in double (the multiplied form is the WRONG
    one, kept for the test that tells them apart)"""
    step = in_size / out_size
    if multiplied:
        return np.array([int((x + 0.5) * step) for x in range(out_size)], np.int64)
    out, xo = [], step * 0.5
    for _ in range(out_size):
        out.append(int(xo))
        xo += step
    return np.array(out, np.int64)


def nearest_resize(m_u8, out_h, out_w):
    h, w = m_u8.shape
    return m_u8[nearest_index(h, out_h)][:, nearest_index(w, out_w)]


def center_crop(x, S):
    top, left = crop_offset(x.shape[0], S), crop_offset(x.shape[1], S)
    return x[top:top + S, left:left + S]


def preprocess_bytes(img, S):
    """[H, W, 3] float image -> the resized and cropped bytes [S, S, 3]"""
    b = to_bytes(img)
    oh, ow = resized_size(b.shape[0], b.shape[1], S)
    return center_crop(bilinear_resize(b, oh, ow), S)


def normalise(bytes_):
    """ToTensor and Normalize(0.5, 0.5) in fp32: [S, S, 3] uint8 -> [3, S, S] float32"""
    x = bytes_.astype(np.float32) / np.float32(255)
    return np.ascontiguousarray(((x - np.float32(0.5)) / np.float32(0.5)).transpose(2, 0, 1))


def patch_matrix(chw):
    """[3, S, S] -> [G^2, 588], columns in the convolution's (c, ky, kx) order"""
    c, S, _ = chw.shape
    G = S // PATCH
    return np.ascontiguousarray(chw.reshape(c, G, PATCH, G, PATCH).transpose(1, 3, 0, 2, 4).reshape(G * G, c * PATCH * PATCH))


def mask_bytes(mask, H, W):
    return np.full((H, W), 255, np.uint8) if mask is None else np.where(np.asarray(mask).reshape(H, W) != 0, 255, 0).astype(np.uint8)


def patch_weights(mask, H, W, S):
    """([G^2] float32 weights, float32 sum = total count / 196 in one rounding)"""
    oh, ow = resized_size(H, W, S)
    m = center_crop(nearest_resize(mask_bytes(mask, H, W), oh, ow), S)
    G = S // PATCH
    counts = (m != 0).reshape(G, PATCH, G, PATCH).sum(axis=(1, 3)).reshape(-1)
    return counts.astype(np.float32) / np.float32(PATCH * PATCH), np.float32(counts.sum()) / np.float32(PATCH * PATCH)


# ---- section 3 in torch ------------------------------------------------------------------------------------------------------------
def random_state_dict(dim, heads, depth, grid, seed=0, extra=()):
    assert dim == 64 * heads
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)       # noqa: E731
    lin = lambda o, i: r(o, i) / math.sqrt(i)          # noqa: E731
    sd = {"cls_token": 0.5 * r(1, 1, dim), "pos_embed": 0.5 * r(1, 1 + grid * grid, dim), "mask_token": r(1, dim),
          "patch_embed.proj.weight": r(dim, 3, PATCH, PATCH) / math.sqrt(3 * PATCH * PATCH), "patch_embed.proj.bias": 0.1 * r(dim)}
    for i in range(depth):
        b = f"blocks.{i}."
        sd.update({b + "norm1.weight": 1 + 0.1 * r(dim), b + "norm1.bias": 0.1 * r(dim), b + "attn.qkv.weight": lin(3 * dim, dim),
                   b + "attn.qkv.bias": 0.1 * r(3 * dim), b + "attn.proj.weight": lin(dim, dim), b + "attn.proj.bias": 0.1 * r(dim),
                   b + "ls1.gamma": 0.5 * r(dim), b + "norm2.weight": 1 + 0.1 * r(dim), b + "norm2.bias": 0.1 * r(dim),
                   b + "mlp.fc1.weight": lin(4 * dim, dim), b + "mlp.fc1.bias": 0.1 * r(4 * dim), b + "mlp.fc2.weight": lin(dim, 4 * dim),
                   b + "mlp.fc2.bias": 0.1 * r(dim), b + "ls2.gamma": 0.5 * r(dim)})
    sd.update({"norm.weight": 1 + 0.1 * r(dim), "norm.bias": 0.1 * r(dim)})
    for k in extra:
        sd[k] = r(1, 4, dim)
    return sd


def attention(qkv, heads, dtype=torch.float64):
    """qkv [n, T, 3 * heads * 64] -> [n, T, heads * 64]; q scaled by 64^-0.5 before q k^T, softmax over the keys"""
    n, T, _ = qkv.shape
    q, k, v = qkv.to(dtype).reshape(n, T, 3, heads, 64).permute(2, 0, 3, 1, 4)
    p = ((q * 64 ** -0.5) @ k.transpose(-2, -1)).softmax(dim=-1)
    return (p @ v).transpose(1, 2).reshape(n, T, heads * 64)


def vit_features(x, sd, heads, dtype=torch.float64, eps=1e-6):
    """[RECALL] forward_features(x)["x_norm_patchtokens"]: x [n, 3, S, S] -> [n, G^2, dim]"""
    w = {k: v.to(dtype) for k, v in sd.items()}
    dim = w["norm.weight"].numel()
    depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    x = F.conv2d(x.to(dtype), w["patch_embed.proj.weight"], w["patch_embed.proj.bias"], stride=PATCH).flatten(2).transpose(1, 2)
    x = torch.cat([w["cls_token"].expand(x.shape[0], -1, -1), x], dim=1)
    assert w["pos_embed"].shape[1] == x.shape[1], "pos_embed is added without interpolation"
    x = x + w["pos_embed"]
    for i in range(depth):
        b = f"blocks.{i}."
        y = F.layer_norm(x, (dim,), w[b + "norm1.weight"], w[b + "norm1.bias"], eps)
        y = attention(F.linear(y, w[b + "attn.qkv.weight"], w[b + "attn.qkv.bias"]), heads, dtype)
        x = x + w[b + "ls1.gamma"] * F.linear(y, w[b + "attn.proj.weight"], w[b + "attn.proj.bias"])
        y = F.layer_norm(x, (dim,), w[b + "norm2.weight"], w[b + "norm2.bias"], eps)
        y = F.linear(F.gelu(F.linear(y, w[b + "mlp.fc1.weight"], w[b + "mlp.fc1.bias"])), w[b + "mlp.fc2.weight"], w[b + "mlp.fc2.bias"])
        x = x + w[b + "ls2.gamma"] * y
    return F.layer_norm(x, (dim,), w["norm.weight"], w["norm.bias"], eps)[:, 1:]


def network_input(pred, gt, S):
    """both images through sections 1: [2, 3, S, S] float32"""
    return torch.from_numpy(np.stack([normalise(preprocess_bytes(np.asarray(t), S)) for t in (pred, gt)]))


def weighted_cosine(feat, weights, total, dtype=torch.float64):
    """section 4 on feat [2, G^2, dim]: (the scalar, the per-patch cosines)"""
    cos = F.cosine_similarity(feat[0].to(dtype), feat[1].to(dtype), dim=-1)
    w = torch.as_tensor(np.asarray(weights)).to(dtype)
    if float(total) <= 1e-6:
        return 0.0, cos
    return float((cos * w).sum() / torch.as_tensor(float(total)).to(dtype)), cos


def similarity_ref(pred, gt, mask, sd, heads, S, dtype=torch.float64):
    """the whole metric: (scalar, features [2, G^2, dim] in `dtype`, per-patch cosines)"""
    feat = vit_features(network_input(pred, gt, S), sd, heads, dtype)
    w, total = patch_weights(None if mask is None else np.asarray(mask), pred.shape[0], pred.shape[1], S)
    value, cos = weighted_cosine(feat, w, total, dtype)
    return value, feat, cos


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def images(H, W, seed, masked=False, noise=40):
    """a random fp32 image in [0, 1], the same image with noise of at most +-noise / 255 per channel, and, if asked, a random bool mask
    [H, W, 1] (about 70 % of the pixels visible)"""
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(H, W, 3, generator=g)
    pred = (gt + (2 * torch.rand(H, W, 3, generator=g) - 1) * (noise / 255)).clamp(0, 1)
    mask = (torch.rand(H, W, 1, generator=g) > 0.3) if masked else None
    return pred, gt, mask
