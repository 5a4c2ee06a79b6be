"""The DINOv2 similarity metric (mtgs_amd/dino.py, csrc/dino.hip, include/mtgs_dino.h) without a GPU: the NumPy restatement of the
preprocessing against Pillow's recorded output (tests/golden/dino_preprocess.npz) and against Pillow itself where it imports, the
host-built tables against the restatement, the crop and nearest rules, the weight handling and its refusals, and the header as a
group of its own."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

from mtgs_amd import dino as D
from tests import dino_refs as R

ROOT = Path(__file__).resolve().parents[1]
NAMES = ["mtgs_dino_attention", "mtgs_dino_features", "mtgs_dino_layernorm", "mtgs_dino_linear", "mtgs_dino_patch_weights", "mtgs_dino_preprocess",
         "mtgs_dino_similarity", "mtgs_dino_tail", "mtgs_dino_weight_floats", "mtgs_dino_workspace_bytes"]
FIXTURE_CASES = [(67, 131, 56), (40, 30, 56), (200, 333, 56), (56, 90, 56), (2000, 61, 56), (128, 228, 518)]
STRIP = (200, 264)


@pytest.fixture(scope="module")
def golden():
    return np.load(ROOT / "tests" / "golden" / "dino_preprocess.npz")


def _emulate(img_u8, mask_u8, S):
    """what csrc/dino.hip computes from the tables of mtgs_amd.dino.resample_tables, in NumPy integers"""
    H, W = img_u8.shape[:2]
    t, hk, vk = D.resample_tables(H, W, S)
    assert t.dtype == np.int32 and t.size == S * (6 + hk + vk)
    parts, o = [], 0
    for n in (2 * S, S * hk, 2 * S, S * vk, S, S):
        parts.append(t[o:o + n])
        o += n
    hb, hc, vb, vc, mx, my = parts[0].reshape(S, 2), parts[1].reshape(S, hk), parts[2].reshape(S, 2), parts[3].reshape(S, vk), parts[4], parts[5]
    assert hb[:, 0].min() >= 0 and (hb[:, 0] + hb[:, 1]).max() <= W and vb[:, 0].min() >= 0 and (vb[:, 0] + vb[:, 1]).max() <= H
    assert 0 <= mx.min() and mx.max() < W and 0 <= my.min() and my.max() < H
    src = img_u8.astype(np.int64)
    hor = np.zeros((H, S, 3), np.int64)
    for x in range(S):
        acc = np.full((H, 3), 1 << 21, np.int64)
        for j in range(hb[x, 1]):
            acc += src[:, hb[x, 0] + j] * hc[x, j]
        hor[:, x] = np.clip(acc >> 22, 0, 255)
    out = np.zeros((S, S, 3), np.uint8)
    for y in range(S):
        acc = np.full((S, 3), 1 << 21, np.int64)
        for j in range(vb[y, 1]):
            acc += hor[vb[y, 0] + j] * vc[y, j]
        out[y] = np.clip(acc >> 22, 0, 255)
    return out, mask_u8[my][:, mx]


# ---- sections 1-2 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,S", FIXTURE_CASES)
def test_the_restatement_and_the_tables_equal_pillows_record(golden, H, W, S):
    key = f"{H}x{W}_{S}"
    img, mask = golden[f"in_{key}"], golden[f"mask_in_{key}"]
    assert img.shape == (H, W, 3) and mask.shape == (H, W)
    oh, ow = R.resized_size(H, W, S)
    assert (oh, ow) == D.resized_size(H, W, S) and min(oh, ow) == S
    ref = R.center_crop(R.bilinear_resize(img, oh, ow), S)
    mref = R.center_crop(R.nearest_resize(mask * np.uint8(255), oh, ow), S) != 0
    emu, memu = _emulate(img, mask * np.uint8(255), S)
    assert np.array_equal(emu, ref) and np.array_equal(memu != 0, mref)
    if S == 518:
        ref, mref = ref[STRIP[0]:STRIP[1]], mref[STRIP[0]:STRIP[1]]
    assert np.array_equal(ref, golden[f"out_{key}"]), "BILINEAR"
    assert np.array_equal(mref, golden[f"mask_out_{key}"] != 0), "NEAREST"


@pytest.mark.parametrize("H,W,S", FIXTURE_CASES + [(1080, 1920, 518), (540, 960, 518)])
def test_the_restatement_equals_pillow_itself(H, W, S):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.RandomState(H + W)
    img, mask = rng.randint(0, 256, (H, W, 3)).astype(np.uint8), (rng.rand(H, W) > 0.3).astype(np.uint8) * np.uint8(255)
    oh, ow = R.resized_size(H, W, S)
    pil = np.asarray(Image.fromarray(img, "RGB").resize((ow, oh), Image.BILINEAR)) if (oh, ow) != (H, W) else img
    pm = np.asarray(Image.fromarray(mask, "L").resize((ow, oh), Image.NEAREST)) if (oh, ow) != (H, W) else mask
    assert np.array_equal(R.bilinear_resize(img, oh, ow), pil)
    assert np.array_equal(R.nearest_resize(mask, oh, ow), pm)
    emu, memu = _emulate(img, mask, S)
    assert np.array_equal(emu, R.center_crop(pil, S)) and np.array_equal(memu, R.center_crop(pm, S))


def test_sizes_crop_offsets_and_the_nearest_rule():
    assert R.resized_size(1080, 1920, 518) == (518, 920) and R.resized_size(40, 30, 56) == (74, 56) and R.resized_size(56, 90, 56) == (56, 90)
    assert R.resized_size(2000, 61, 56) == (1836, 56) and R.resized_size(56, 56, 56) == (56, 56)
    assert R.crop_offset(109, 56) == 26                       # (109 - 56) / 2 = 26.5: half to even, not 27
    assert R.crop_offset(93, 56) == 18 and R.crop_offset(920, 518) == 201 and R.crop_offset(56, 56) == 0      # 18.5 -> 18
    assert D.crop_offset(109, 56) == 26 and D.crop_offset(59, 56) == 2                                         # 1.5 -> 2
    added, multiplied = R.nearest_index(1080, 518), R.nearest_index(1080, 518, multiplied=True)
    assert not np.array_equal(added, multiplied)              # a test with the multiplied rule would fail at 1080 -> 518
    assert np.array_equal(D.nearest_sources(1080, 518, 0, 518), added)
    assert np.array_equal(D.nearest_sources(1920, 920, 201, 518), R.nearest_index(1920, 920)[201:201 + 518])


def test_bytes_normalisation_and_patch_order():
    x = np.array([[[0.0, 1.0, 0.5], [-0.2, 1.7, 0.999999], [1 / 255, 254.999 / 255, 0.00392]]], np.float32)
    assert R.to_bytes(x).tolist() == [[[0, 255, 127], [0, 255, 254], [1, 254, 0]]]
    b = np.arange(28 * 28 * 3, dtype=np.int64).reshape(28, 28, 3).astype(np.uint8)
    chw = R.normalise(b)
    assert chw.dtype == np.float32 and chw[1, 2, 3] == np.float32((np.float32(b[2, 3, 1]) / np.float32(255) - np.float32(0.5)) / np.float32(0.5))
    pm = R.patch_matrix(chw)
    assert pm.shape == (4, 588) and pm[3, 2 * 196 + 5 * 14 + 7] == chw[2, 14 + 5, 14 + 7]
    conv = torch.nn.functional.conv2d(torch.from_numpy(chw)[None].double(), torch.ones(1, 3, 14, 14, dtype=torch.float64), stride=14).reshape(-1)
    assert torch.allclose(conv, torch.from_numpy(pm).double().sum(dim=1))
    w, total = R.patch_weights(None, 67, 131, 56)
    assert (w == 1).all() and total == 16
    m = np.zeros((56, 56), bool)
    m[:14, :7] = True
    w, total = R.patch_weights(m, 56, 56, 56)
    assert w[0] == np.float32(0.5) and not w[1:].any() and total == np.float32(98) / np.float32(196)


# ---- weights ---------------------------------------------------------------------------------------------------------------------
def test_config_inference_and_the_round_trip():
    sd = R.random_state_dict(128, 2, 3, 5, seed=1)
    w = D.DinoWeights.from_state_dict(sd)
    assert w.config == D.DinoConfig(dim=128, heads=2, depth=3, image=70) and (w.config.grid, w.config.tokens) == (5, 26)
    assert w.flat.dtype == torch.float32 and w.flat.dim() == 1
    back = w.to_state_dict()
    assert set(back) == set(sd) - {"mask_token"}              # mask_token is ignored
    assert all(torch.equal(back[k], sd[k]) for k in back)
    assert torch.equal(w.tensor("blocks.1.attn.qkv.weight"), sd["blocks.1.attn.qkv.weight"].t())          # [K][N]
    pe = w.tensor("patch_embed.proj.weight")
    assert pe.shape == (588, 128) and pe[2 * 196 + 3 * 14 + 4, 7] == sd["patch_embed.proj.weight"][7, 2, 3, 4]       # K runs (c, ky, kx)
    assert torch.equal(w.tensor("pos_embed"), sd["pos_embed"][0]) and torch.equal(w.tensor("blocks.2.ls2.gamma"), sd["blocks.2.ls2.gamma"])
    assert D.DinoWeights.infer_config(R.random_state_dict(768, 12, 1, 37)) == D.DinoConfig(depth=1)          # ViT-B's width and grid
    assert D.DinoConfig().tokens == 1370


def test_each_refusal_names_its_reason():
    sd = R.random_state_dict(128, 2, 1, 4, seed=2)
    with pytest.raises(NotImplementedError, match="register_tokens"):
        D.DinoWeights.from_state_dict(R.random_state_dict(128, 2, 1, 4, extra=("register_tokens",)))
    with pytest.raises(NotImplementedError, match=r"blocks\.0\.mlp\.w12\.weight: SwiGLU"):
        D.DinoWeights.from_state_dict(dict(sd, **{"blocks.0.mlp.w12.weight": torch.zeros(4, 4)}))
    with pytest.raises(NotImplementedError, match="pos_embed has 17 tokens, the configuration 1 \\+ 5\\^2 = 26"):
        D.DinoWeights.from_state_dict(sd, config=D.DinoConfig(dim=128, heads=2, depth=1, image=70))
    with pytest.raises(ValueError, match="pos_embed .*not 1 \\+ G\\^2"):
        D.DinoWeights.from_state_dict(dict(sd, pos_embed=torch.zeros(1, 16, 128)))
    with pytest.raises(KeyError, match="blocks.0.ls1.gamma"):
        D.DinoWeights.from_state_dict({k: v for k, v in sd.items() if k != "blocks.0.ls1.gamma"})
    with pytest.raises(ValueError, match="blocks.0.attn.proj.bias: shape"):
        D.DinoWeights.from_state_dict(dict(sd, **{"blocks.0.attn.proj.bias": torch.zeros(64)}))
    with pytest.raises(NotImplementedError, match="patch_embed.proj.weight .*14 x 14"):
        D.DinoWeights.from_state_dict(dict(sd, **{"patch_embed.proj.weight": torch.zeros(128, 3, 16, 16)}))
    with pytest.raises(NotImplementedError, match="blocks.0.attn.q_norm.weight: a parameter this implementation does not know"):
        D.DinoWeights.from_state_dict(dict(sd, **{"blocks.0.attn.q_norm.weight": torch.zeros(64)}))
    with pytest.raises(NotImplementedError, match="head dimension must be 64"):
        D.DinoConfig(dim=128, heads=4)
    with pytest.raises(NotImplementedError, match="dim = 1280 exceeds 1024"):
        D.DinoConfig(dim=1280, heads=20)
    with pytest.raises(ValueError, match="multiple of the patch"):
        D.DinoConfig(image=512)
    with pytest.raises(NotImplementedError, match="mlp_ratio"):
        D.DinoWeights.from_state_dict(dict(sd, **{"blocks.0.mlp.fc1.weight": torch.zeros(256, 128)}))


# ---- the restatement's own properties ------------------------------------------------------------------------------------------------
def test_the_reference_discriminates():
    """With the seeded weights the image matters: identical images give 1, noise of +-40 / 255 gives about 0.98 with per-patch
    cosines clearly below 1, an all-masked image gives exactly 0."""
    sd = R.random_state_dict(128, 2, 2, 4, seed=132)
    pred, gt, mask = R.images(67, 131, seed=67, masked=True)
    v, feat, cos = R.similarity_ref(pred, gt, mask, sd, 2, 56)
    assert 0.5 < v < 0.9999 and float(cos.min()) < 0.99 and feat.shape == (2, 16, 128)
    same, _, _ = R.similarity_ref(pred, pred.clone(), mask, sd, 2, 56)
    assert abs(same - 1) <= 2.0 ** -23                        # the fp32 weights against their once-rounded fp32 sum
    assert R.similarity_ref(pred, gt, torch.zeros_like(mask), sd, 2, 56)[0] == 0.0
    assert R.similarity_ref(pred, gt, None, sd, 2, 56)[0] != v
    qkv = torch.randn(1, 5, 3 * 2 * 64, generator=torch.Generator().manual_seed(0))
    q, k, vv = qkv.double().reshape(1, 5, 3, 2, 64).permute(2, 0, 3, 1, 4)
    want = torch.nn.functional.scaled_dot_product_attention(q, k, vv).transpose(1, 2).reshape(1, 5, 128)
    assert torch.allclose(R.attention(qkv, 2), want, rtol=1e-12, atol=1e-12)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_the_header_is_declared_bound_and_exported():
    """include/mtgs_dino.h is a group of its own (tests/test_abi.py checks every group against its header, its reviewed record
    tests/golden/abi_signatures_dino.txt and the library): its entry points, its configuration record and its constants."""
    from mtgs_amd import _abi, _lib
    abi = _abi.header_abi("mtgs_dino.h")
    assert sorted(_lib.GROUPS["mtgs_dino.h"]) == NAMES
    assert abi.structs["mtgs_dino_config"].names == ("dim", "heads", "depth", "patch", "image", "mlp_ratio", "ln_eps") and abi.structs["mtgs_dino_config"].itemsize == 28
    assert [abi.constants[k] for k in ("MTGS_DINO_EPI_BIAS", "MTGS_DINO_EPI_BIAS_GELU", "MTGS_DINO_EPI_SCALE_RESIDUAL", "MTGS_DINO_EPI_PATCH_EMBED")] == [0, 1, 2, 3]
    assert (abi.constants["MTGS_DINO_PATCH"], abi.constants["MTGS_DINO_HEAD_DIM"], abi.constants["MTGS_DINO_MAX_DIM"]) == (14, 64, 1024) == (D.PATCH, D.HEAD_DIM, D.MAX_DIM)


def test_the_size_queries_need_no_device(hip_lib):
    """The flat weight array is what DinoWeights lays out; the workspace is the sum the header lists; a configuration the kernels do
    not implement is refused with the reason."""
    n = C.c_size_t(0)
    for dim, heads, depth, G in ((128, 2, 2, 4), (768, 12, 12, 37)):
        cfg = D.DinoConfig(dim=dim, heads=heads, depth=depth, image=14 * G)
        c = cfg.struct()
        assert hip_lib.mtgs_dino_weight_floats(c.ctypes.data, C.byref(n)) == 0
        assert n.value == sum(int(np.prod(shape)) for _, _, shape in D._layout(cfg))
        T, r4 = cfg.tokens, lambda v: (v + 3) // 4 * 4       # noqa: E731
        assert hip_lib.mtgs_dino_workspace_bytes(c.ctypes.data, C.byref(n)) == 0
        assert n.value == 4 * (r4(2 * G * G * 588) + 2 * r4(2 * T * dim) + r4(2 * T * 4 * dim) + r4(G * G + 1) + r4(G * G))
    assert D.DinoWeights.from_state_dict(R.random_state_dict(128, 2, 2, 4)).flat.numel() == 128 * (588 + 2 + 17) + 2 * (12 * 128 * 128 + 15 * 128) + 2 * 128
    bad = D.DinoConfig(dim=128, heads=2, depth=1, image=56).struct()
    bad["heads"] = 4
    assert hip_lib.mtgs_dino_workspace_bytes(bad.ctypes.data, C.byref(n)) != 0
    assert b"head dimension must be 64" in hip_lib.mtgs_rast_last_error()
    bad["heads"], bad["patch"] = 2, 16
    assert hip_lib.mtgs_dino_weight_floats(bad.ctypes.data, C.byref(n)) != 0
    assert b"patch = 16" in hip_lib.mtgs_rast_last_error()


def test_the_public_names():
    import mtgs_amd
    from mtgs_amd import metrics
    assert metrics.dino_similarity is D.dino_similarity and metrics.DinoWeights is D.DinoWeights
    assert mtgs_amd.DinoWeights is D.DinoWeights and mtgs_amd.DinoConfig is D.DinoConfig and mtgs_amd.dino_similarity is D.dino_similarity
    assert {"DinoConfig", "DinoWeights", "dino_similarity"} <= set(mtgs_amd.__all__)
    import inspect
    assert inspect.signature(metrics.image_metrics).parameters["dino_weights"].default is None
