#!/usr/bin/env python3
"""WildGaussians appearance colours (config/WildGaussians.py) at the headline size: 2M Gaussians, 960x540, RGB+ED with MTGS's three
camera-space normal channels (7 blended channels), antialiased, absgrad.  Forward + backward per step, device events, median of
--steps steps after --warmup, for four forms of the colour path:

    torch   the reference's PyTorch expression over all N (mtgs_scene_graph.py:623-632) + rasterization(colors=[N, 6])
    dense   mtgs_amd.wild_colors over all N + rasterization(colors=[N, 6])
    source  mtgs_amd.wild_color_source: the visible Gaussians only, inside the rasterization
    touch   the same with touch_first (colours written for the Gaussians the frame composites from; the MLP kernels still walk
            every visible row, the others as zero rows)

The normal channels come from mtgs_amd.nodes.camera_space_normals in the first two forms and from inside the rasterization in the
other two, so the forms differ in the colour path only.  Prints one JSON line per form and the rows each form evaluates.  With
--stats KERNEL_STATS.csv (rocprofv3 --kernel-trace --stats of a run of this script) it prints the MLP kernels' achieved FLOP/s:
rows x FLOP per row (below, from the layer widths) over their kernel time, against the 157.3 TF f32 MFMA peak."""
import argparse
import csv
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

C0 = 0.28209479177387814
PEAK_F32 = 157.3e12
# FLOP per row of the kernels (layer 1 is 27 -> 128: the embedding is folded into the bias)
FLOP_FWD = 2 * (27 * 128 + 128 * 128 + 128 * 6)
FLOP_BWD = 2 * (27 * 128 + 128 * 128 + 128 * 6) + 2 * (128 * 6 * 2 + 128 * 128 * 2 + 27 * 128 * 2)   # recomputed forward + VJPs
KERNELS = {"wild_fwd_kernel": FLOP_FWD, "wild_bwd_kernel": FLOP_BWD}


def torch_colors(dc, rest, emb, mlp):
    N = dc.shape[0]
    rgb = torch.clamp(dc * C0 + 0.5, 0.0, 1.0)
    x = torch.cat([rgb, rest.reshape(N, -1)[:, :24], emb.reshape(1, 32).expand(N, 32)], dim=-1)
    y = 0.01 * mlp(x)
    return rgb * (1 + y[:, 3:6]) + y[:, :3]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2_000_000)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--height", type=int, default=540)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--forms", default="torch,dense,source,touch")
    ap.add_argument("--stats", default=None, help="rocprofv3 kernel_stats.csv of a run of this script: print achieved FLOP/s")
    ap.add_argument("--rows", default=None, help="JSON lines of an earlier run of this script (rows per form, for --stats)")
    args = ap.parse_args()
    if args.stats:
        return report_stats(args)
    from mtgs_amd import rasterization, wild_color_source, wild_colors
    from mtgs_amd.nodes import camera_space_normals
    from mtgs_amd.synthetic import make_camera, make_scene
    dev = torch.device("cuda")
    N, W, H = args.n, args.width, args.height
    sc = make_scene(N, seed=0, sh_degree=3)
    vm, K = make_camera(W, H)
    vm, K = vm.to(dev), K.to(dev)
    c2w = torch.inverse(vm)[:, :3, :]
    g = torch.Generator().manual_seed(1)
    P = {k: sc[k].to(dev).requires_grad_(True) for k in ("means", "quats", "scales", "opacities")}
    dc = sc["coeffs"][:, 0, :].contiguous().to(dev).requires_grad_(True)
    rest = sc["coeffs"][:, 1:, :].contiguous().to(dev).requires_grad_(True)
    emb = torch.randn(32, generator=g).to(dev).requires_grad_(True)
    torch.manual_seed(0)
    mlp = torch.nn.Sequential(torch.nn.Linear(59, 128), torch.nn.ReLU(), torch.nn.Linear(128, 128), torch.nn.ReLU(),
                              torch.nn.Linear(128, 6)).to(dev)
    Gc = torch.randn(1, H, W, 7, generator=g).to(dev)
    Ga = torch.randn(1, H, W, 1, generator=g).to(dev)
    leaves = list(P.values()) + [dc, rest, emb] + list(mlp.parameters())

    def step(form):
        for t in leaves:
            t.grad = None
        src, cols = None, None
        if form in ("torch", "dense"):
            rgb = torch_colors(dc, rest, emb, mlp) if form == "torch" else wild_colors(dc, rest, emb, mlp)
            cols = camera_space_normals(P["quats"], P["scales"], P["means"], c2w, rgb)
        else:
            src = wild_color_source(dc, rest, emb, mlp, camera_normals=c2w[0].contiguous(), touch_first=form == "touch")
        r, a, info = rasterization(P["means"], P["quats"], P["scales"], P["opacities"], cols, vm, K, W, H, packed=False,
                                   render_mode="RGB+ED", rasterize_mode="antialiased", absgrad=True, color_source=src)
        torch.autograd.backward([r, a], [Gc, Ga])
        return info, src

    for form in args.forms.split(","):
        for _ in range(args.warmup):
            info, src = step(form)
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.steps):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            info, src = step(form)
            e.record()
            torch.cuda.synchronize()
            ms.append(s.elapsed_time(e))
        n_vis = int((info["radii"] > 0).sum())
        rows = N if form in ("torch", "dense") else n_vis      # rows the MLP kernels walk (touch_first: unflagged rows are zero rows)
        flagged = int(src.row_flags[:n_vis].sum()) if form == "touch" else None
        print(json.dumps({"form": form, "measured": True, "N": N, "width": W, "height": H, "channels": 7, "steps": args.steps,
                          "fwd_bwd_ms_median": round(statistics.median(ms), 4), "fwd_bwd_ms_min": round(min(ms), 4),
                          "fwd_bwd_ms_max": round(max(ms), 4), "n_visible": n_vis, "mlp_rows_fwd": rows, "mlp_rows_bwd": rows,
                          "flagged_rows": flagged}),
              flush=True)


def report_stats(args):
    """Achieved FLOP/s of the MLP kernels: (rows per call x FLOP per row) summed over the calls of each form, over the kernel time
    rocprofv3 recorded.  The stats file aggregates every call of a kernel, so the rows of all forms and steps that ran are summed."""
    rows = [json.loads(l) for l in Path(args.rows).read_text().splitlines() if l.startswith("{")]
    calls = args.warmup + args.steps
    walked = [r["N"] if r["form"] in ("torch", "dense") else r["n_visible"] for r in rows if r["form"] != "torch"]
    rows_total = {"wild_fwd_kernel": sum(walked) * calls, "wild_bwd_kernel": sum(walked) * calls}
    with open(args.stats) as f:
        for rec in csv.DictReader(f):
            name = rec.get("Name", rec.get("KernelName", ""))
            k = next((k for k in KERNELS if k in name), None)
            if k is None:
                continue
            t_ns = float(rec["TotalDurationNs"])
            flop = rows_total[k] * KERNELS[k]
            print(json.dumps({"kernel": k, "measured": True, "calls": int(rec["Calls"]), "total_ms": round(t_ns / 1e6, 3),
                              "avg_us": round(float(rec["AverageNs"]) / 1e3, 2), "flop_per_row": KERNELS[k], "rows": rows_total[k],
                              "achieved_tflops": round(flop / (t_ns * 1e-9) / 1e12, 2),
                              "share_of_f32_peak": round(flop / (t_ns * 1e-9) / PEAK_F32, 3)}))


if __name__ == "__main__":
    main()
