#!/usr/bin/env python
"""Times mtgs_amd.dino_similarity (ViT-B / 14 at 518 x 518, the hub's dinov2_vitb14 shape, seeded random weights) against a
torch.nn.functional chain of the same definition on the same GPU.

    whole metric   1920 x 1080 and 960 x 540 inputs; one call on two images and a mask, eager and as a replayed HIP graph.  The torch
                   chain is the network and the tail in fp32 on the device (conv2d patch embedding, layer_norm, linear, softmax
                   attention written out as the hub code has it, gelu, cosine_similarity), fed with OUR preprocessed images: the
                   definition's preprocessing is Pillow's integer resample, which torch has no operator for.  With PIL importable the
                   reference's host round trip for the preprocessing (images and mask to the host, Pillow, back) is timed beside it.
    per stage      the preprocessing, the patch weights, the layer norm, the tail, the five GEMM shapes and attention of one block,
                   with achieved TFLOP/s = 2 M K N / time (attention: 4 n heads T^2 64 / time), each beside torch's operator
    accuracy       e = |ours - fp64|, e32 = |fp32 CPU restatement - fp64| on small networks (the shapes of tests/test_gpu_dino.py)

Device events around one call on the current stream, `--reps` calls after `--warmup` untimed ones; median (min .. max); the host
round trip by the wall clock around a synchronised call.  There are no trained DINOv2 weights here, and the time does not depend
on them.  Writes profiles/dino.txt.

    python scripts/dino_bench.py [--reps 20] [--warmup 3] [--out profiles/dino.txt]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from mtgs_amd import dino as D  # noqa: E402
from tests import dino_refs as R  # noqa: E402

SIZES = ((1080, 1920), (540, 960))
ACCURACY = ((128, 2, 2, 4, 67, 131, True), (192, 3, 3, 6, 40, 30, False), (768, 12, 1, 8, 67, 131, True))


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ms.append(s.elapsed_time(e))
    return ms


def fmt(ms):
    return f"{statistics.median(ms) * 1e3:9.1f} us  ({min(ms) * 1e3:.1f} .. {max(ms) * 1e3:.1f})"


def graphed(fn):
    """fn captured once on a side stream (after a warm-up there); returns the replay"""
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        fn()
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        fn()
    return graph.replay


class TorchChain:
    """Sections 3 and 4 of the definition in torch.nn.functional on the device, fp32; returns a 0-dim tensor."""

    def __init__(self, sd, heads):
        self.w = {k: v.cuda() for k, v in sd.items()}
        self.heads, self.dim = heads, sd["norm.weight"].numel()
        self.depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))

    def features(self, x):
        w, dim = self.w, self.dim
        x = F.conv2d(x, w["patch_embed.proj.weight"], w["patch_embed.proj.bias"], stride=14).flatten(2).transpose(1, 2)
        x = torch.cat([w["cls_token"].expand(x.shape[0], -1, -1), x], dim=1) + w["pos_embed"]
        n, T, _ = x.shape
        for i in range(self.depth):
            b = f"blocks.{i}."
            y = F.layer_norm(x, (dim,), w[b + "norm1.weight"], w[b + "norm1.bias"], 1e-6)
            q, k, v = F.linear(y, w[b + "attn.qkv.weight"], w[b + "attn.qkv.bias"]).reshape(n, T, 3, self.heads, 64).permute(2, 0, 3, 1, 4)
            y = (((q * 0.125) @ k.transpose(-2, -1)).softmax(dim=-1) @ v).transpose(1, 2).reshape(n, T, dim)
            x = x + w[b + "ls1.gamma"] * F.linear(y, w[b + "attn.proj.weight"], w[b + "attn.proj.bias"])
            y = F.layer_norm(x, (dim,), w[b + "norm2.weight"], w[b + "norm2.bias"], 1e-6)
            y = F.linear(F.gelu(F.linear(y, w[b + "mlp.fc1.weight"], w[b + "mlp.fc1.bias"])), w[b + "mlp.fc2.weight"], w[b + "mlp.fc2.bias"])
            x = x + w[b + "ls2.gamma"] * y
        return F.layer_norm(x, (dim,), w["norm.weight"], w["norm.bias"], 1e-6)[:, 1:]

    def __call__(self, x, pw):
        f = self.features(x)
        cos = F.cosine_similarity(f[0], f[1], dim=-1)
        total = pw[-1]
        return torch.where(total > 1e-6, (cos * pw[:-1]).sum() / total, torch.zeros_like(total))


def host_round_trip(pred, gt, mask, S):
    """the reference's preprocessing: both images and the mask to the host, Pillow, the normalised tensors and the weights back"""
    from PIL import Image
    H, W = pred.shape[:2]
    oh, ow = R.resized_size(H, W, S)
    out = []
    for img in (pred, gt):
        pil = Image.fromarray(img.mul(255).byte().cpu().numpy(), "RGB").resize((ow, oh), Image.BILINEAR)
        x = torch.from_numpy(R.center_crop(np.asarray(pil), S).copy()).permute(2, 0, 1).float().div(255)
        out.append(((x - 0.5) / 0.5).cuda())
    m = Image.fromarray(mask.reshape(H, W).to(torch.uint8).mul(255).cpu().numpy(), "L").resize((ow, oh), Image.NEAREST)
    m = torch.from_numpy(R.center_crop(np.asarray(m), S).copy() > 127).float().cuda()
    weights = m.unfold(0, 14, 14).unfold(1, 14, 14).sum(dim=(-1, -2)).flatten() / 196
    torch.cuda.synchronize()
    return torch.stack(out), weights


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "dino.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "dino_bench.py measures on the device: there is no CPU timing"
    cfg = D.DinoConfig()
    sd = R.random_state_dict(cfg.dim, cfg.heads, cfg.depth, cfg.grid, seed=7)
    dev = D.DinoWeights.from_state_dict(sd, device="cuda")
    chain = TorchChain(sd, cfg.heads)
    S, G2, T, d = cfg.image, cfg.patches, cfg.tokens, cfg.dim
    lines = [f"mtgs_amd.dino_similarity (ViT-B/14 at {S} x {S}: {d} wide, {cfg.heads} heads, {cfg.depth} blocks, {T} tokens per image) against the "
             f"torch.nn.functional chain, {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"device events around one call, median (min .. max) of {a.reps} after {a.warmup} warm-ups; seeded random weights; "
             f"workspace {D.workspace_bytes(cfg) / 1e6:.1f} MB", ""]

    def say(*new):
        lines.extend(new)
        print("\n".join(new), flush=True)

    for H, W in SIZES:
        pred, gt, mask = (t.cuda() for t in R.images(H, W, seed=H, masked=True))
        patches = D.dino_preprocess(pred, gt, S)
        x_in = patches.reshape(2, cfg.grid, cfg.grid, 3, 14, 14).permute(0, 3, 1, 4, 2, 5).reshape(2, 3, S, S).contiguous()
        pw = D.dino_patch_weights(mask, H, W, S)
        ours = lambda: D.dino_similarity(pred, gt, mask, weights=dev)           # noqa: E731
        theirs = lambda: chain(x_in, pw)                                        # noqa: E731
        vo, vt = ours().item(), theirs().item()
        say(f"whole metric, {W} x {H}: ours {vo:.7g}, torch chain {vt:.7g}, |difference| {abs(vo - vt):.3g}")
        t_e = timed(ours, a.reps, a.warmup)
        say(f"  ours, eager ({4 + 7 * cfg.depth + 2} launches, preprocessing included)   {fmt(t_e)}")
        t_g = timed(graphed(ours), a.reps, a.warmup)
        say(f"  ours, replayed graph                               {fmt(t_g)}")
        c_e = timed(theirs, a.reps, a.warmup)
        say(f"  torch chain (network + tail), eager                {fmt(c_e)}")
        try:
            c_g = timed(graphed(theirs), a.reps, a.warmup)
            say(f"  torch chain (network + tail), replayed graph       {fmt(c_g)}")
            ratio_g = f"{statistics.median(c_g) / statistics.median(t_g):.2f}x"
        except Exception as exc:        # a library kernel may refuse a capture; that is a finding, not a failure of this script
            say(f"  torch chain, replayed graph                        not captured: {type(exc).__name__}: {str(exc).splitlines()[0][:120]}")
            ratio_g = "n/a"
        say(f"  ratio torch chain / ours (ours includes the preprocessing): eager {statistics.median(c_e) / statistics.median(t_e):.2f}x, graph {ratio_g}")
        try:
            host_round_trip(pred, gt, mask, S)
            wall = []
            for _ in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                xr, wr = host_round_trip(pred, gt, mask, S)
                wall.append((time.perf_counter() - t0) * 1e3)
            say(f"  the reference's host round trip for the preprocessing (Pillow, wall clock)   {statistics.median(wall) * 1e3:9.1f} us; "
                f"its images equal ours bitwise: {bool(torch.equal(xr, x_in))}; its patch weights (count / 196 by torch on the device) "
                f"within {float((wr - pw[:-1]).abs().max()):.3g} of ours")
        except ImportError:
            say("  the reference's host round trip: PIL does not import here")
        say(f"  preprocessing (one launch, both images)            {fmt(timed(lambda: D.dino_preprocess(pred, gt, S), a.reps, a.warmup))}")
        say(f"  patch weights (one launch)                         {fmt(timed(lambda: D.dino_patch_weights(mask, H, W, S), a.reps, a.warmup))}", "")

    # per stage, at the token count of the metric
    M = 2 * T
    g = torch.Generator().manual_seed(1)
    say(f"per stage at M = 2 T = {M} rows:")
    for name, K, N, epi in (("patch embedding", 588, d, "patch_embed"), ("qkv", d, 3 * d, "bias"), ("proj + ls1 + residual", d, d, "scale_residual"),
                            ("fc1 + GELU", d, 4 * d, "gelu"), ("fc2 + ls2 + residual", 4 * d, d, "scale_residual")):
        rows = 2 * G2 if epi == "patch_embed" else M
        x = torch.randn(rows, K, generator=g).cuda()
        w = (torch.randn(K, N, generator=g) / K ** 0.5).cuda()
        b, gamma, res = torch.randn(N, generator=g).cuda(), torch.randn(N, generator=g).cuda(), torch.randn(rows, N, generator=g).cuda()
        pos, cls = torch.randn(T, N, generator=g).cuda(), torch.randn(N, generator=g).cuda()
        wt = w.t().contiguous()
        if epi == "patch_embed":
            fn = lambda: D.dino_linear(x, w, b, epi, pos=pos, cls=cls)                       # noqa: E731
            lib = lambda: F.linear(x, wt, b) + pos[1:].repeat(2, 1)                           # noqa: E731
        elif epi == "scale_residual":
            fn = lambda: D.dino_linear(x, w, b, epi, gamma=gamma, residual=res)              # noqa: E731  (includes the copy of the residual)
            lib = lambda: res + gamma * F.linear(x, wt, b)                                    # noqa: E731
        elif epi == "gelu":
            fn = lambda: D.dino_linear(x, w, b, epi)                                          # noqa: E731
            lib = lambda: F.gelu(F.linear(x, wt, b))                                          # noqa: E731
        else:
            fn = lambda: D.dino_linear(x, w, b, epi)                                          # noqa: E731
            lib = lambda: F.linear(x, wt, b)                                                  # noqa: E731
        t_o, t_l = timed(fn, a.reps, a.warmup), timed(lib, a.reps, a.warmup)
        flop = 2.0 * rows * K * N
        say(f"  {name:22s} {rows} x {K:4d} x {N:4d}, {flop / 1e9:6.2f} GFLOP: ours {fmt(t_o)} = {flop / statistics.median(t_o) / 1e9:6.1f} TFLOP/s;  "
            f"torch {fmt(t_l)} = {flop / statistics.median(t_l) / 1e9:6.1f} TFLOP/s")
    qkv = torch.randn(2, T, 3 * d, generator=g).cuda()
    q, k, v = qkv.reshape(2, T, 3, cfg.heads, 64).permute(2, 0, 3, 1, 4)
    att = lambda: D.dino_attention(qkv, cfg.heads)                                           # noqa: E731
    sdpa = lambda: F.scaled_dot_product_attention(q, k, v)                                   # noqa: E731
    plain = lambda: ((q * 0.125) @ k.transpose(-2, -1)).softmax(dim=-1) @ v                  # noqa: E731
    flop = 4.0 * 2 * cfg.heads * T * T * 64
    for name, fn in (("attention, ours", att), ("attention, torch sdpa", sdpa), ("attention, torch written out", plain)):
        t = timed(fn, a.reps, a.warmup)
        say(f"  {name:29s} 2 x {cfg.heads} x {T}^2 x 64, {flop / 1e9:6.2f} GFLOP: {fmt(t)} = {flop / statistics.median(t) / 1e9:6.1f} TFLOP/s")
    x = torch.randn(M, d, generator=g).cuda()
    lw, lb = torch.randn(d, generator=g).cuda(), torch.randn(d, generator=g).cuda()
    say(f"  layer norm {M} x {d}: ours {fmt(timed(lambda: D.dino_layernorm(x, lw, lb), a.reps, a.warmup))};  "
        f"torch {fmt(timed(lambda: F.layer_norm(x, (d,), lw, lb, 1e-6), a.reps, a.warmup))}")
    feat, pw = torch.randn(2, G2, d, generator=g).cuda(), torch.rand(G2 + 1, generator=g).cuda()
    say(f"  tail (two launches): ours {fmt(timed(lambda: D.dino_tail(feat, pw), a.reps, a.warmup))}", "")

    say("accuracy on small networks (e = |ours - fp64|, e32 = |fp32 CPU restatement - fp64|; the test asserts e <= 4 e32 + 2^-21):")
    for dim, heads, depth, G, H, W, masked in ACCURACY:
        sd_s = R.random_state_dict(dim, heads, depth, G, seed=dim + G)
        dev_s = D.DinoWeights.from_state_dict(sd_s, device="cuda")
        pred, gt, mask = R.images(H, W, seed=H + W + G, masked=masked)
        v64, f64, _ = R.similarity_ref(pred, gt, mask, sd_s, heads, 14 * G)
        v32, f32, _ = R.similarity_ref(pred, gt, mask, sd_s, heads, 14 * G, dtype=torch.float32)
        got = D.dino_similarity(pred.cuda(), gt.cuda(), None if mask is None else mask.cuda(), weights=dev_s).item()
        fe = float((D.dino_features(pred.cuda(), gt.cuda(), weights=dev_s).cpu().double() - f64).abs().max())
        say(f"  {dim} wide, {depth} deep, G = {G}, {H} x {W}{' masked' if masked else ''}: value {v64:.9g}  e {abs(got - v64):.3g}  e32 {abs(v32 - v64):.3g};  "
            f"features e {fe:.3g}  e32 {float((f32.double() - f64).abs().max()):.3g}")

    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
