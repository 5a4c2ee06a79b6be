#!/usr/bin/env python
"""Times mtgs_amd.crop.crop_gaussians on the 2 M-Gaussian WB-v1 scene (mtgs_amd.synthetic) with the six collected tensors of
get_gaussians (means, scales, quats, opacities, rgbs, model_id), at a box that keeps about 3 % and one that keeps about half,
against the reference's own composition on the same device (mtgs_scene_graph.py:457-459):

    crop_ids = within_torch(means)                   # nerfstudio's OrientedBox.within: homogeneous matmul, strict compares
    {k: v[crop_ids] for k, v in gaussians.items()}   # one boolean-mask index per tensor

The inverse of the box matrix is taken ONCE outside the timed region for the reference (nerfstudio inverts per call), so the
comparison favours the reference.  Device events around every call, `--reps` timed calls after `--warmup` untimed ones; the median
and the spread (min .. max) of each side are printed, and the outputs of the two sides are compared bit for bit before timing.
Writes profiles/crop_bench.txt.

    python scripts/crop_bench.py [--n 2000000] [--reps 30] [--warmup 5] [--out profiles/crop_bench.txt]
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from mtgs_amd.crop import OrientedBox, crop_gaussians  # noqa: E402
from mtgs_amd.synthetic import make_scene  # noqa: E402

POS = (3.0, -2.0, 1.0)
BOXES = [("3 %", (0.3, -0.2, 1.1), (40.0, 10.0, 25.0)), ("half", (0.0, 0.6, 0.0), (75.0, 16.0, 75.0))]


def within_torch(h_world2bbox, half, pts):
    p = torch.cat((pts, torch.ones_like(pts[..., :1])), dim=-1)
    p = torch.matmul(h_world2bbox, p.T).T[..., :3]
    return torch.all(torch.cat([p > -half, p < half], dim=-1), dim=-1)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "crop_bench.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "crop_bench needs a HIP device"
    assert a.reps >= 20 and a.warmup >= 5
    dev = torch.device("cuda")
    sc = make_scene(a.n, seed=0)
    gs = {"means": sc["means"], "scales": sc["scales"], "quats": sc["quats"], "opacities": sc["opacities"], "rgbs": sc["colors"],
          "model_id": torch.arange(a.n) * 4 // a.n}
    gs = {k: v.to(dev) for k, v in gs.items()}
    lines = []
    for name, rpy, size in BOXES:
        box = OrientedBox.from_params(POS, rpy, size)
        H = torch.eye(4)
        H[:3, :3], H[:3, 3] = torch.from_numpy(box.R).float(), torch.from_numpy(box.T).float()
        h_inv, half = torch.inverse(H).to(dev), (torch.from_numpy(box.S).float() / 2).to(dev)

        def reference():
            ids = within_torch(h_inv, half, gs["means"])
            return {k: v[ids] for k, v in gs.items()}

        def device():
            return crop_gaussians(gs, box)

        got, want = device(), {k: v[box.within(gs["means"])] for k, v in gs.items()}
        kept = got["means"].shape[0]
        assert all(torch.equal(got[k], want[k]) for k in gs), "crop_gaussians differs from torch indexing by its own mask"
        ref_kept = reference()["means"].shape[0]
        # alternate the two sides so that a drift of the machine's load falls on both
        t_dev, t_ref = [], []
        for _ in range(2):
            t_dev += timed(device, a.reps // 2, a.warmup)
            t_ref += timed(reference, a.reps // 2, a.warmup)
        med_d, med_r = statistics.median(t_dev), statistics.median(t_ref)
        line = (f"WB-v1 N={a.n} box {name:>4}: kept {kept} ({100.0 * kept / a.n:.2f} %; the fp32-inverse evaluation keeps {ref_kept})   "
                f"crop_gaussians median {med_d:.3f} ms (min {min(t_dev):.3f}, max {max(t_dev):.3f}, n={len(t_dev)})   "
                f"torch within + 6 mask indexings median {med_r:.3f} ms (min {min(t_ref):.3f}, max {max(t_ref):.3f}, n={len(t_ref)})   "
                f"ratio {med_r / med_d:.2f}x")
        print(line, flush=True)
        lines.append(line)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
