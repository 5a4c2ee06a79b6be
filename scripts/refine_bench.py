"""Times mtgs_amd.densify.refine_scene against the loop it replaces -- refine_gaussians + reset_opacities per node, each call a
pass over a table of one node -- on the same seeded scenes, in one process, the two alternating, every timed call ending in a device synchronisation (host clock: the host
work between the launches is what the per-node loop pays for).

    python scripts/refine_bench.py [--out profiles/refine_scene.txt] [--repeats 9] [--small]

Scenes: (a) 1.6 M multi-colour Gaussians (T = 3) + 0.4 M road Gaussians, the scene of profiles/r04_training_phases.txt;
(b) the same plus a 100 000-Gaussian sky node and 100 object nodes of about 3000.  In the timed comparison the sky node is culled
by the vanilla rule in BOTH paths (refine_gaussians knows no other), so that the two compute the same tensors -- which the script
checks, bit for bit, before it times anything; refine_scene with the sky node's own rule is timed as a third line.
The row move's achieved bytes/s: bytes counted from the shapes (every output row written once; parameter rows read once, moment
rows read for old Gaussians only; 5 bytes of src_index / kind per row and tensor) over the launch's device time (HIP events)."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from mtgs_amd import _lib  # noqa: E402
from mtgs_amd.densify import NodeRefine, RefineConfig, refine_gaussians, refine_scene, reset_opacities  # noqa: E402

STEP = 3100            # a reset step of the shipped schedule (3100 % (30 * 100) == 100): the loop also pays reset_opacities


def make_node(N, seed, kind, dev, sky=False):
    g = torch.Generator(device=dev).manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g, device=dev)
    rn = lambda *s: torch.randn(*s, generator=g, device=dev)
    if sky:
        d = rn(N, 3)
        d[:, 1].abs_()
        means = d / d.norm(dim=-1, keepdim=True) * (1000.0 + 1000.0 * r(N, 1))
        scales = torch.log(torch.tensor(2.0, device=dev)) + r(N, 3) * 4.0                # exp(scale) 2 .. 109: metres, as a dome's spacing
    else:
        means = (r(N, 3) * 2 - 1) * torch.tensor([60.0, 8.0, 140.0], device=dev)
        scales = torch.log(r(N, 3) * 0.3 + 0.01)
    p = {"means": means, "scales": scales, "quats": rn(N, 4), "opacities": rn(N, 1) * 2.0 + 1.0, "features_dc": rn(N, 3)}
    if kind == "multi":
        p["features_rest"] = rn(N, 3, 15, 3)
        p["features_adapters"] = rn(N, 3, 3)
    else:
        p["features_rest"] = rn(N, 15, 3)
    vc = torch.randint(1, 12, (N,), generator=g, device=dev).float()
    stats = (r(N) * 0.0011 * vc, vc, r(N) * 110.0)       # about a tenth above the gradient threshold, a tenth above split_screen_size
    moments = {k: (rn(*v.shape), r(*v.shape)) for k, v in p.items()}
    return p, stats, moments


def make_scene(which, dev, small):
    f = 50 if small else 1
    cfg = RefineConfig(densify_from_iter=500)
    nodes = []
    for i, (N, kind, sky) in enumerate([(1_600_000 // f, "multi", False), (400_000 // f, "plain", False)] +
                                       ([(100_000 // f, "multi", True)] + [(2500 + 37 * (j % 28), "plain", False) for j in range(100)] if which == "b" else [])):
        p, stats, moments = make_node(N, 1 + i, kind, dev, sky)
        nodes.append(NodeRefine(p, stats, cfg, 11 + i, moments=moments, cull_rule=(100.0, 1000.0) if sky else (100.0, 40.0)))
    return nodes


def loop(nodes, step):
    out = []
    for nd in nodes:
        new, new_m, info = refine_gaussians(nd.params, nd.stats, nd.cfg, step, nd.seed, moments=nd.moments)
        if step % (nd.cfg.reset_alpha_every * nd.cfg.refine_every) == nd.cfg.refine_every:
            reset_opacities(new["opacities"], nd.cfg, new_m["opacities"])
        out.append((new, new_m, info))
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def move_bytes(nodes, results, step):
    """bytes the row move has to read and write, from the shapes and the counts"""
    total = 0
    for nd, res in zip(nodes, results):
        if res is None:
            continue
        n_after, n_old = res[2]["n_after"], res[2]["n_old_kept"]
        reset = step % (nd.cfg.reset_alpha_every * nd.cfg.refine_every) == nd.cfg.refine_every
        for k, v in nd.params.items():
            w = v[0].numel() * 4
            if k not in ("means", "scales"):               # (their values come from the geometry launch; their moments move here)
                total += n_after * (2 * w + 5)
            if k == "opacities" and reset:
                total += 2 * n_after * w                   # zero-all: written, nothing read
            else:
                total += 2 * (n_after * (w + 5) + n_old * w)
    return total


def spread(xs):
    return f"[{' '.join('%.2f' % x for x in xs)}]  median {statistics.median(xs):8.2f} ms  min {min(xs):8.2f}  max {max(xs):8.2f}  stdev {statistics.pstdev(xs):6.2f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "refine_scene.txt"))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--small", action="store_true", help="1/50 of the static nodes: a rehearsal of the script, not a measurement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("refine_bench.py measures on the device: no GPU found")
    dev = torch.device("cuda")
    lines = ["# refine_scene against the per-node loop (refine_gaussians + reset_opacities), scripts/refine_bench.py" + (" --small" if args.small else ""),
             f"# step {STEP} (a reset step), {args.repeats} repeats after 2 warm-up calls each, the two paths alternating; host clock around calls that",
             "# end in a device synchronisation.  " + torch.cuda.get_device_name(0)]
    verdict = {}
    for which in ("a", "b"):
        nodes = make_scene(which, dev, args.small)
        same = [nd if nd.cull_rule == (100.0, 40.0) else NodeRefine(nd.params, nd.stats, nd.cfg, nd.seed, moments=nd.moments) for nd in nodes]
        n_total = sum(nd.params["means"].shape[0] for nd in nodes)
        a, b = loop(same, STEP), refine_scene(same, STEP)
        for i, ((pa, ma, ia), (pb, mb, ib)) in enumerate(zip(a, b)):        # faster and different is not faster
            assert ia["n_after"] == ib["n_after"] and torch.equal(ia["src_index"], ib["src_index"]), i
            for k in pa:
                assert torch.equal(pa[k], pb[k]) and torch.equal(ma[k][0], mb[k][0]) and torch.equal(ma[k][1], mb[k][1]), (i, k)
        n_after = sum(r[2]["n_after"] for r in b)
        nbytes = move_bytes(same, b, STEP)
        del a, b
        for _ in range(2):
            loop(same, STEP), refine_scene(same, STEP)
        t_loop, t_scene, t_sky = [], [], []
        for _ in range(args.repeats):
            t_loop.append(timed(lambda: loop(same, STEP))[0])
            t_scene.append(timed(lambda: refine_scene(same, STEP))[0])
        if which == "b":                                   # (apart from the comparison: other sizes, so the allocator's blocks change hands)
            for _ in range(3):
                refine_scene(nodes, STEP)
            t_sky = [timed(lambda: refine_scene(nodes, STEP))[0] for _ in range(args.repeats)]
        _lib.time_calls(["mtgs_refine_scene_rows"])
        refine_scene(same, STEP)
        torch.cuda.synchronize()
        rows_scene = sum(_lib.timed_ms()["mtgs_refine_scene_rows"])
        _lib.time_calls(["mtgs_refine_scene_rows"])
        loop(same, STEP)                                   # (one launch per node: refine_gaussians is the one-entry table)
        torch.cuda.synchronize()
        rows_loop = _lib.timed_ms()["mtgs_refine_scene_rows"]
        _lib.time_calls(())
        med_l, med_s = statistics.median(t_loop), statistics.median(t_scene)
        noise = max(max(t_loop) - min(t_loop), max(t_scene) - min(t_scene))
        lines += [f"scene ({which}): {len(nodes)} nodes, {n_total} Gaussians -> {n_after}; results of the two paths bit-identical",
                  f"  per-node loop : {spread(t_loop)}",
                  f"  refine_scene  : {spread(t_scene)}"]
        if t_sky:
            lines.append(f"  refine_scene, sky node by its own rule (100, 1000): {spread(t_sky)}")
        lines += [f"  difference of the medians {med_l - med_s:+.2f} ms (loop - scene); largest spread (max - min) of either {noise:.2f} ms",
                  f"  row move: {nbytes / 1e9:.3f} GB counted from the shapes; refine_scene ONE launch {rows_scene:.3f} ms = {nbytes / rows_scene / 1e6:.0f} GB/s; "
                  f"loop {len(rows_loop)} launches of mtgs_refine_scene_rows {sum(rows_loop):.3f} ms = {nbytes / sum(rows_loop) / 1e6:.0f} GB/s (device time, HIP events)"]
        verdict[which] = (med_l - med_s, noise)
        del nodes, same
        torch.cuda.empty_cache()
    ok_b = verdict["b"][0] > verdict["b"][1]
    ok_a = verdict["a"][0] > -verdict["a"][1]
    lines.append(f"verdict: (b) faster than the loop by more than the spread: {'yes' if ok_b else 'NO'}; (a) not slower beyond the spread: {'yes' if ok_a else 'NO'}")
    text = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)
    print(json.dumps({"a": verdict["a"], "b": verdict["b"]}))


if __name__ == "__main__":
    main()
