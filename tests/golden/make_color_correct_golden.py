#!/usr/bin/env python3
"""Golden vectors for mtgs_amd.metrics.color_correct, produced by the REFERENCE's own function in the build container:
/root/reference/mtgs/utils/pnsr.py is imported by path (it needs torch only at import time) and color_correct is run as MTGS
calls it (mtgs_scene_graph.py:762-765): color_correct(pred * mask, gt * mask) with a [H, W, 1] bool mask, or
color_correct(pred, gt) without one.  Every case runs in float64 (the expected output) and float32; the reference's own
f32-vs-f64 gap is stored per case as the tolerance floor.  Writes tests/golden/color_correct_ref.npz (inputs + outputs only)."""
import importlib.util
from pathlib import Path

import numpy as np
import torch

spec = importlib.util.spec_from_file_location("ref_pnsr", "/root/reference/mtgs/utils/pnsr.py")
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)

g = torch.Generator().manual_seed(7)


def shifted(gt, scale=1.0):
    """gt under a random per-channel quadratic colour shift, plus a little noise"""
    a = 1.0 + 0.3 * scale * (torch.rand(3, generator=g) - 0.5)
    b = 0.4 * scale * (torch.rand(3, generator=g) - 0.5)
    c = 0.1 * scale * (torch.rand(3, generator=g) - 0.5)
    return (c + a * gt + b * gt * gt + 0.02 * torch.randn(gt.shape, generator=g, dtype=gt.dtype)).clamp(0, 1)


out = {}
cases = {}
# a: correlated pred / gt under a quadratic colour shift, no mask
gt = torch.rand(24, 32, 3, generator=g, dtype=torch.float64)
cases["a"] = (shifted(gt), gt, None, 5)
# b: MTGS's masked call, odd size
gt = torch.rand(27, 35, 3, generator=g, dtype=torch.float64)
cases["b"] = (shifted(gt), gt, torch.rand(27, 35, 1, generator=g) > 0.3, 5)
# c: many pixels saturated at 0 and 1 in both images (the clip masks matter)
gt = (1.6 * torch.rand(30, 30, 3, generator=g, dtype=torch.float64) - 0.3).clamp(0, 1)
cases["c"] = (shifted(gt, 2.0), gt, None, 5)
# d: one iteration, masked
gt = torch.rand(20, 41, 3, generator=g, dtype=torch.float64)
cases["d"] = (shifted(gt), gt, torch.rand(20, 41, 1, generator=g) > 0.5, 1)
# e: a strong shift that pushes pixels out of [0, 1] (the corrected estimate clips), 5 iterations
gt = torch.rand(33, 29, 3, generator=g, dtype=torch.float64)
cases["e"] = ((0.2 + 0.9 * gt - 0.3 * gt * gt + 0.03 * torch.randn(gt.shape, generator=g, dtype=gt.dtype)).clamp(0, 1), gt, None, 5)

for name, (pred, gt, mask, iters) in cases.items():
    pred, gt = pred.float().double(), gt.float().double()     # inputs exactly representable in f32
    res = {}
    for dt in (torch.float64, torch.float32):
        p, t = pred.to(dt), gt.to(dt)
        if mask is not None:
            p, t = p * mask, t * mask
        res[dt] = ref.color_correct(p, t, num_iters=iters)
        assert not torch.equal(res[dt], p), f"case {name} {dt}: the reference fell back"
    out[f"{name}_pred"] = pred.to(torch.float32).numpy()
    out[f"{name}_gt"] = gt.to(torch.float32).numpy()
    out[f"{name}_mask"] = np.zeros(0, dtype=bool) if mask is None else mask.numpy()
    out[f"{name}_iters"] = np.int32(iters)
    out[f"{name}_cc_f64"] = res[torch.float64].numpy()
    out[f"{name}_cc_f32"] = res[torch.float32].numpy()
    out[f"{name}_gap"] = np.float64((res[torch.float32].double() - res[torch.float64]).abs().max())
np.savez_compressed(Path(__file__).parent / "color_correct_ref.npz", **out)
print({k: float(v) for k, v in out.items() if k.endswith("_gap")})
