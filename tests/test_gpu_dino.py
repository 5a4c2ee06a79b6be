"""The DINOv2 similarity metric on the GPU (mtgs_amd/dino.py, csrc/dino.hip) against the restatement of tests/dino_refs.py.

(1) the preprocessing BITWISE (bytes, patch-matrix floats, patch weights and their sum) against the NumPy restatement, which
    tests/test_dino_host.py compares with Pillow;
(2) the GEMM, every epilogue at the M edges of its 32-row MFMA tiles and 128-row workgroups, per element within the DERIVED bound
    B = 1e-6 (sum |a| |w| + |b|) of one k-ordered fp32 fma chain (tests/test_gpu_lpips.py: 3.5e-7 of sum |a b| measured at K = 4096)
    before the epilogue, propagated through it: 1.13 B for the GELU (its largest slope), |gamma| B for the scale.  What the epilogue
    itself rounds in fp32 is added, each term from the number format: the GELU's erf argument, erff (<= 4 ulp), 1 + erf and two
    products give 2^-24 |x| (0.4 |x| + 5); the scale's product and the residual add half an ulp each of |gamma x| and of the result;
    the position add half an ulp of the result;
(3) the layer norm: e <= 4 e32 + 4 ulp of the reference element, e32 the LARGEST error of the fp32 CPU F.layer_norm in that row (one
    element's own fp32 error is zero by chance too often to bound another summation order);
(4) attention alone: |out - ref64| <= (2 ds + 1e-6) sum_j p_j |v_j|, ds = 1e-6 max_j sum |q / 8| |k| of the row (a logit perturbation
    d changes every softmax weight by a relative e^{2d} - 1);
(5) the whole metric: features e <= 4 e32 + 2^-20 max |f| per element, the scalar e <= 4 e32 + 2^-21;
(6) exact and repeat behaviour, image_metrics; (7) graph capture; (8) errors.
All weights are seeded random ones (dino_refs.random_state_dict): there are no trained DINOv2 weights here."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import dino_refs as R
from tests import util

pytestmark = pytest.mark.gpu

_cache = {}


def _net(dim, heads, depth, G):
    """(state dict on the CPU, DinoWeights on the device), made once per network"""
    key = (dim, heads, depth, G)
    if key not in _cache:
        from mtgs_amd.dino import DinoWeights
        sd = R.random_state_dict(dim, heads, depth, G, seed=dim + G)
        _cache[key] = (sd, DinoWeights.from_state_dict(sd, device="cuda"))
    return _cache[key]


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- (1) preprocessing -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,S", [(67, 131, 56), (40, 30, 56), (2000, 61, 56), (56, 56, 56), (1080, 1920, 518)])
def test_preprocess_is_bitwise_the_restatement(H, W, S):
    from mtgs_amd.dino import dino_patch_weights, dino_preprocess
    pred, gt, mask = R.images(H, W, seed=H + W, masked=True)
    pred[0, 0, 0], pred[1, 1, 1], gt[0, 0, 1] = 1.5, -0.25, 1.0            # outside [0, 1]: clamped, not wrapped
    patches, out_bytes = dino_preprocess(pred.cuda(), gt.cuda(), S, return_bytes=True)
    G = S // 14
    assert patches.shape == (2 * G * G, 588) and out_bytes.shape == (2, S, S, 3) and out_bytes.dtype == torch.uint8
    for i, img in enumerate((pred, gt)):
        ref = R.preprocess_bytes(img.numpy(), S)
        assert np.array_equal(out_bytes[i].cpu().numpy(), ref), f"bytes of image {i}"
        want = R.patch_matrix(R.normalise(ref))
        assert np.array_equal(patches[i * G * G:(i + 1) * G * G].cpu().numpy().view(np.int32), want.view(np.int32)), f"patch matrix of image {i}"
    assert torch.equal(dino_preprocess(pred.cuda(), gt.cuda(), S), patches)
    for m in ((mask, torch.zeros_like(mask), None) if S == 56 else (mask,)):
        got = dino_patch_weights(None if m is None else m.cuda(), H, W, S, device="cuda").cpu().numpy()
        w, total = R.patch_weights(None if m is None else m.numpy(), H, W, S)
        assert np.array_equal(got[:-1].view(np.int32), w.view(np.int32)) and got[-1].view(np.int32) == total.view(np.int32)
        if m is None:
            assert (got[:-1] == 1).all() and got[-1] == G * G
        elif not m.any():
            assert (got == 0).all()
        else:
            assert 0 < got[-1] < G * G
    u8 = dino_patch_weights((mask.cuda().to(torch.uint8) * 255).reshape(H, W), H, W, S)
    assert torch.equal(u8, dino_patch_weights(mask.cuda(), H, W, S))


# ---- (2) the GEMM ------------------------------------------------------------------------------------------------------------------
MS = (32, 33, 34, 74, 130)


@pytest.mark.parametrize("epilogue", ["bias", "gelu", "scale_residual", "patch_embed"])
@pytest.mark.parametrize("K,N", [(588, 128), (128, 384), (512, 128), (3072, 768), (4, 64), (132, 64)])
def test_linear_every_epilogue(K, N, epilogue):
    """K = 4 is less than one K-step; K = 132 is the smallest K past one 128-k chain, and no multiple of 32."""
    from mtgs_amd.dino import dino_linear
    g = torch.Generator().manual_seed(K + N)
    w = torch.randn(K, N, generator=g) / K ** 0.5
    b, gamma, cls = 0.1 * torch.randn(N, generator=g), 0.5 * torch.randn(N, generator=g), 0.5 * torch.randn(N, generator=g)
    w_d, b_d = w.cuda(), b.cuda()
    for M in MS:
        if epilogue == "patch_embed" and M % 2:
            continue                       # its rows are the patches of two images
        a = torch.randn(M, K, generator=g)
        res, pos = torch.randn(M, N, generator=g), 0.5 * torch.randn(M // 2 + 1, N, generator=g)
        x = a.double() @ w.double() + b.double()
        B = 1e-6 * (a.double().abs() @ w.double().abs() + b.double().abs())
        if epilogue == "bias":
            got, ref, bound = dino_linear(a.cuda(), w_d, b_d), x, B
        elif epilogue == "gelu":
            got, ref = dino_linear(a.cuda(), w_d, b_d, "gelu"), F.gelu(x)
            bound = 1.13 * B + 2.0 ** -24 * x.abs() * (0.4 * x.abs() + 5)
        elif epilogue == "scale_residual":
            got = dino_linear(a.cuda(), w_d, b_d, "scale_residual", gamma=gamma.cuda(), residual=res.cuda())
            ref = res.double() + gamma.double() * x
            bound = gamma.double().abs() * B + 2.0 ** -24 * ((gamma.double() * x).abs() + ref.abs())
        else:
            T = M // 2 + 1
            got = dino_linear(a.cuda(), w_d, b_d, "patch_embed", pos=pos.cuda(), cls=cls.cuda())
            assert got.shape == (2 * T, N)
            for im in range(2):
                assert torch.equal(got[im * T].cpu(), cls + pos[0]), "class row"
            got = torch.cat([got[1:T], got[T + 1:]])
            ref = x + torch.cat([pos[1:], pos[1:]]).double()
            bound = B + 2.0 ** -24 * ref.abs()
        err = (got.cpu().double() - ref).abs()
        worst = float((err / bound).max())
        print(f"linear {epilogue} M={M} K={K} N={N}: max err / bound = {worst:.3g}, max err / B = {float((err / B).max()):.3g}")
        assert tuple(got.shape) == tuple(ref.shape) and bool((err <= bound).all()), f"{epilogue} M={M} K={K} N={N}: {worst:.3g} of the bound"
        if M == 33 and epilogue != "patch_embed":            # a misaligned input takes the scalar loader and gives the same bits
            shifted = torch.empty(a.numel() + 1, device="cuda")[1:]
            shifted.copy_(a.reshape(-1))
            assert shifted.data_ptr() % 16 == 4
            kw = dict(gamma=gamma.cuda(), residual=res.cuda()) if epilogue == "scale_residual" else {}
            assert torch.equal(dino_linear(shifted.view(M, K), w_d, b_d, epilogue, **kw), got)


@pytest.mark.parametrize("N", [16320, 16384])
def test_linear_on_both_sides_of_the_tile_threshold(N):
    """The 128 x 64 tile is used from 512 workgroups on, the 128 x 32 tile below: M = 130 makes two row tiles, so N = 16384 is 512
    workgroups of the wide tile and N = 16320 is 510, which take the narrow one (as every case above does).  K = 160 crosses the
    128-k restart and ends in a zero-filled step.  The same derived bound."""
    from mtgs_amd.dino import dino_linear
    M, K = 130, 160
    g = torch.Generator().manual_seed(N)
    a, w, b = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g) / K ** 0.5, 0.1 * torch.randn(N, generator=g)
    gamma, res = 0.5 * torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    x = a.double() @ w.double() + b.double()
    B = 1e-6 * (a.double().abs() @ w.double().abs() + b.double().abs())
    got = dino_linear(a.cuda(), w.cuda(), b.cuda())
    err = (got.cpu().double() - x).abs()
    print(f"linear bias M={M} K={K} N={N}: max err / B = {float((err / B).max()):.3g}")
    assert bool((err <= B).all())
    got = dino_linear(a.cuda(), w.cuda(), b.cuda(), "scale_residual", gamma=gamma.cuda(), residual=res.cuda())
    ref = res.double() + gamma.double() * x
    assert bool(((got.cpu().double() - ref).abs() <= gamma.double().abs() * B + 2.0 ** -24 * ((gamma.double() * x).abs() + ref.abs())).all())
    narrow = dino_linear(a.cuda(), w[:, :64].contiguous().cuda(), b[:64].cuda())           # the same columns through the other tile: the same chains
    assert torch.equal(narrow, dino_linear(a.cuda(), w.cuda(), b.cuda())[:, :64])


# ---- (3) layer norm ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [128, 768])
def test_layernorm(D):
    from mtgs_amd.dino import dino_layernorm
    g = torch.Generator().manual_seed(D)
    x = torch.randn(9, D, generator=g)
    x[3] = 1.5                             # a constant row: every partial sum is exact, the variance is exactly 0
    x[5, D // 3] = 1000.0                  # one large entry
    x[6] *= 50
    w, b = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    ref = F.layer_norm(x.double(), (D,), w.double(), b.double(), 1e-6)
    e32 = (F.layer_norm(x, (D,), w, b, 1e-6).double() - ref).abs().max(dim=1, keepdim=True).values
    got = dino_layernorm(x.cuda(), w.cuda(), b.cuda(), 1e-6).cpu()
    err = (got.double() - ref).abs()
    bound = 4 * e32 + 4 * 2.0 ** -23 * ref.abs()
    print(f"layernorm D={D}: max err {float(err.max()):.3g}, max err / bound {float((err / bound.clamp_min(1e-300)).max()):.3g}, e32 {float(e32.max()):.3g}")
    assert bool((err <= bound).all())
    assert torch.equal(got[3], b)          # (x - mean) is exactly 0


# ---- (4) attention -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qscale", [1.0, 4.0])
@pytest.mark.parametrize("T", [17, 26, 37, 65])
def test_attention_alone(T, qscale):
    from mtgs_amd.dino import dino_attention
    heads = 2
    g = torch.Generator().manual_seed(T)
    qkv = torch.randn(2, T, 3, heads, 64, generator=g)
    qkv[:, :, 0] *= qscale
    qkv = qkv.reshape(2, T, 3 * heads * 64)
    ref = R.attention(qkv, heads)
    q, k, v = qkv.double().reshape(2, T, 3, heads, 64).permute(2, 0, 3, 1, 4)
    p = ((q * 0.125) @ k.transpose(-2, -1)).softmax(dim=-1)
    ds = 1e-6 * ((q.abs() * 0.125) @ k.abs().transpose(-2, -1)).max(dim=-1, keepdim=True).values
    bound = ((2 * ds + 1e-6) * (p @ v.abs())).transpose(1, 2).reshape(2, T, heads * 64)
    got = dino_attention(qkv.cuda(), heads).cpu()
    err = (got.double() - ref).abs()
    print(f"attention T={T} q x {qscale}: max err / bound = {float((err / bound).max()):.3g}")
    assert got.shape == ref.shape and bool((err <= bound).all())


# ---- (5) the whole metric -------------------------------------------------------------------------------------------------------------
NETS = [(128, 2, 2, 4), (128, 2, 2, 5), (192, 3, 3, 6), (768, 12, 1, 8)]


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("H,W", [(67, 131), (40, 30)])
@pytest.mark.parametrize("dim,heads,depth,G", NETS)
def test_whole_metric(dim, heads, depth, G, H, W, masked):
    """e <= 4 e32 + floor, features and scalar; both recorded in the parity report.  Measured on the MI355X: the scalar within 9.1e-8
    of fp64 (fp32 CPU restatement: up to 7.1e-8), the features within 2.3e-6 of values up to 6.3 (fp32 CPU restatement: 2.9e-6)."""
    from mtgs_amd.dino import dino_features, dino_similarity
    sd, dev = _net(dim, heads, depth, G)
    pred, gt, mask = R.images(H, W, seed=H + W + G, masked=masked)
    v64, f64, _ = R.similarity_ref(pred, gt, mask, sd, heads, 14 * G)
    v32, f32, _ = R.similarity_ref(pred, gt, mask, sd, heads, 14 * G, dtype=torch.float32)
    assert 0.5 < v64 < 0.9999
    feat = dino_features(pred.cuda(), gt.cuda(), weights=dev)
    got = dino_similarity(pred.cuda(), gt.cuda(), None if mask is None else mask.cuda(), weights=dev)
    assert feat.shape == (2, G * G, dim) and got.dim() == 0 and got.dtype == torch.float32 and got.is_cuda
    fe, fe32 = (feat.cpu().double() - f64).abs(), (f32.double() - f64).abs()
    e, e32 = abs(float(got.double()) - v64), abs(v32 - v64)
    case = f"{dim}x{depth}_G{G}_{H}x{W}{'_masked' if masked else ''}"
    print(f"dinov2_sim {case}: value {v64:.9g} e = {e:.3g} e32 = {e32:.3g}; features e = {float(fe.max()):.3g} e32 = {float(fe32.max()):.3g} "
          f"max |f| = {float(f64.abs().max()):.3g}")
    util.REPORT.append({"kind": "dinov2_sim", "case": case, "value": v64, "e": e, "e32": e32, "features_e": float(fe.max()), "features_e32": float(fe32.max())})
    assert bool((fe <= 4 * fe32 + 2.0 ** -20 * float(f64.abs().max())).all()), f"features: {float(fe.max()):.3g}"
    assert e <= 4 * e32 + 2.0 ** -21, f"e = {e:.3g} > 4 * {e32:.3g} + 2^-21"


# ---- (6) exact and repeat behaviour ---------------------------------------------------------------------------------------------------
def test_identical_images_all_masked_and_repeats():
    from mtgs_amd.dino import dino_features, dino_patch_weights, dino_similarity, dino_tail
    _, dev = _net(128, 2, 2, 4)
    pred, gt, mask = (t.cuda() for t in R.images(67, 131, seed=3, masked=True))
    same = dino_similarity(pred, pred.clone(), mask, weights=dev)
    feat = dino_features(pred, pred.clone(), weights=dev)
    assert torch.equal(feat[0], feat[1])
    own = dino_tail(feat, dino_patch_weights(mask, 67, 131, 56))             # the device's own tail on equal rows
    assert _bits(same).item() == _bits(own).item() and abs(same.item() - 1) <= 2.0 ** -22
    assert dino_similarity(pred, gt, torch.zeros_like(mask), weights=dev).item() == 0.0
    a, b = dino_similarity(pred, gt, mask, weights=dev), dino_similarity(pred, gt, mask, weights=dev)
    assert _bits(a).item() == _bits(b).item() and 0.5 < a.item() < 1
    assert a.item() != dino_similarity(pred, gt, None, weights=dev).item()
    assert dino_similarity(pred, gt, mask.reshape(67, 131).to(torch.uint8) * 255, weights=dev).item() == a.item()


def test_the_scratch_is_per_stream():
    """The metric on the default stream and on two others, one call at a time: the results are bitwise equal, and each stream has a
    scratch tensor of its own (mtgs_amd._lib.scratch keys on the stream), allocated once."""
    from mtgs_amd import _lib
    from mtgs_amd.dino import dino_similarity
    _, dev = _net(128, 2, 2, 4)
    pred, gt, mask = (t.cuda() for t in R.images(40, 30, seed=4, masked=True))
    torch.cuda.synchronize()
    results, scratches = [], []

    def run(stream):
        with torch.cuda.stream(stream):
            out = dino_similarity(pred, gt, mask, weights=dev)
        torch.cuda.synchronize()
        results.append(out.view(torch.int32).item())
        scratches.append(_lib.scratch(("dino", dev.config), lambda: pytest.fail("the call left no scratch for its stream"), pred.device, stream.cuda_stream))

    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    for stream in (torch.cuda.current_stream(), a, b):
        run(stream)
    assert results[0] == results[1] == results[2]
    assert len({t.data_ptr() for t in scratches}) == 3 and all(t.numel() > 0 and t.dtype == torch.uint8 for t in scratches)
    entries = len(_lib._scratch)
    run(a)
    assert scratches[3] is scratches[1] and len(_lib._scratch) == entries and results[3] == results[0]


def test_image_metrics_gains_the_key_and_keeps_the_others():
    from mtgs_amd import image_metrics
    from mtgs_amd.metrics import dino_similarity
    _, dev = _net(128, 2, 2, 4)
    pred, gt, mask = (t.cuda() for t in R.images(64, 96, seed=8, masked=True))
    depth, lidar = 1 + 40 * torch.rand(64, 96, 1, device="cuda"), 1 + 40 * torch.rand(64, 96, 1, device="cuda")
    plain = image_metrics(pred, gt, mask, pred_depth=depth, lidar_depth=lidar)
    more = image_metrics(pred, gt, mask, pred_depth=depth, lidar_depth=lidar, dino_weights=dev)
    assert "dinov2_sim" not in plain and sorted(more) == sorted(list(plain) + ["dinov2_sim"])
    for k in plain:
        assert _bits(plain[k]).item() == _bits(more[k]).item(), k
    assert _bits(more["dinov2_sim"]).item() == _bits(dino_similarity(pred, gt, mask, weights=dev)).item()


# ---- (7) graph -----------------------------------------------------------------------------------------------------------------------
def test_similarity_captures_in_a_graph():
    """One stream, no parallel branches; replayed on rewritten inputs the result equals the eager one bitwise."""
    from mtgs_amd.dino import dino_similarity
    _, dev = _net(128, 2, 2, 5)
    H, W = 67, 131
    first = [t.cuda() for t in R.images(H, W, seed=11, masked=True)]
    second = [t.cuda() for t in R.images(H, W, seed=12, masked=True)]
    static = [t.clone() for t in first]

    def step():
        return dino_similarity(static[0], static[1], static[2], weights=dev)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                              # warm-up outside the capture: the tables and the workspace are made here
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    seen = []
    for src in (second, first):
        for dst, t in zip(static, src):
            dst.copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        eager = dino_similarity(src[0], src[1], src[2], weights=dev)
        assert _bits(out).item() == _bits(eager).item()
        seen.append(out.item())
    assert seen[0] != seen[1]


# ---- (8) errors ----------------------------------------------------------------------------------------------------------------------
def test_errors():
    from mtgs_amd.dino import DinoWeights, dino_attention, dino_layernorm, dino_linear, dino_similarity
    sd, dev = _net(128, 2, 2, 4)
    good = torch.rand(40, 40, 3, device="cuda")
    rgba = torch.rand(40, 40, 4, device="cuda")
    with pytest.raises(NotImplementedError, match="4 channels"):
        dino_similarity(rgba, rgba, weights=dev)
    with pytest.raises(ValueError, match="same shape"):
        dino_similarity(good, torch.rand(40, 41, 3, device="cuda"), weights=dev)
    with pytest.raises(ValueError, match="mask must have"):
        dino_similarity(good, good, torch.ones(40, 41, dtype=torch.bool, device="cuda"), weights=dev)
    needs = torch.rand(40, 40, 3, device="cuda").requires_grad_(True)
    with pytest.raises(RuntimeError, match="requires grad"):
        dino_similarity(needs, good, weights=dev)
    with torch.no_grad():
        assert dino_similarity(needs, good, weights=dev).item() > 0
    with pytest.raises(RuntimeError, match="weights are on cpu"):
        dino_similarity(good, good, weights=DinoWeights.from_state_dict(sd))
    with pytest.raises(RuntimeError, match="HIP device"):
        dino_similarity(good.cpu(), good.cpu(), weights=dev)
    with pytest.raises(NotImplementedError, match="N = 96"):
        dino_linear(torch.rand(4, 8, device="cuda"), torch.rand(8, 96, device="cuda"), torch.rand(96, device="cuda"))
    with pytest.raises(NotImplementedError, match="K = 6"):
        dino_linear(torch.rand(4, 6, device="cuda"), torch.rand(6, 64, device="cuda"), torch.rand(64, device="cuda"))
    with pytest.raises(NotImplementedError, match="D = 96"):
        dino_layernorm(torch.rand(4, 96, device="cuda"), torch.rand(96, device="cuda"), torch.rand(96, device="cuda"))
    with pytest.raises(ValueError, match="qkv must be"):
        dino_attention(torch.rand(2, 5, 3 * 2 * 32, device="cuda"), 2)
