"""bench.py's --dump-outputs arrays (bench.output_arrays): float32, within the 64 MiB cap at the headline size, and the same
seeded sample of rows in every run.  CPU."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import bench  # noqa: E402


def _outputs(n, w, h, seed):
    g = torch.Generator().manual_seed(seed)
    grads = {"means": torch.randn(n, 3, generator=g), "quats": torch.randn(n, 4, generator=g), "scales": torch.randn(n, 3, generator=g),
             "opacities": torch.randn(n, generator=g), "coeffs": torch.randn(n, 16, 3, generator=g), "viewmat": torch.randn(1, 4, 4, generator=g)}
    return torch.rand(1, h, w, 4, generator=g), torch.rand(1, h, w, 1, generator=g), grads


def test_headline_size_fits_and_samples_the_same_rows():
    render, alpha, grads = _outputs(2_000_000, 1920, 1080, 0)
    grads["means"][:, 0] = torch.arange(2_000_000, dtype=torch.float32)
    out = bench.output_arrays(render, alpha, grads)
    assert sum(a.nbytes for a in out.values()) <= 64 << 20
    assert all(a.dtype == np.float32 for a in out.values())
    assert out["render"].shape == (1, 1080, 1920, 4) and np.array_equal(out["render"], render.numpy())
    assert out["alpha"].shape == (1, 1080, 1920, 1) and out["grad_viewmat"].shape == (1, 4, 4)
    assert out["grad_coeffs"].shape == (bench.DUMP_GAUSSIANS, 16, 3) and out["grad_opacities"].shape == (bench.DUMP_GAUSSIANS,)
    # the sampled rows are rows of the gradient, in index order, and the same rows for every tensor and every run
    rows = out["grad_means"][:, 0].astype(np.int64)       # (column 0 of grad_means holds the row index)
    assert np.all(np.diff(rows) > 0) and np.array_equal(grads["means"].numpy()[rows], out["grad_means"])
    assert np.array_equal(grads["coeffs"].numpy()[rows], out["grad_coeffs"])
    again = bench.output_arrays(render, alpha, {k: v.clone() for k, v in grads.items()})
    assert all(np.array_equal(out[k], again[k]) for k in out)


def test_large_image_is_sampled_within_the_cap():
    render, alpha, grads = _outputs(1000, 3840, 2160, 1)
    out = bench.output_arrays(render, alpha, grads)
    assert sum(a.nbytes for a in out.values()) <= 64 << 20
    assert out["render"].shape[1] == 4 and out["render"].shape[0] == out["alpha"].shape[0] < 3840 * 2160
    assert out["grad_means"].shape == (1000, 3) and np.array_equal(out["grad_means"], grads["means"].numpy())


def test_steps_must_be_positive(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse_args()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "7", "--dump-outputs", "d"])
    a = bench.parse_args()
    assert a.steps == 7 and a.dump_outputs == "d" and not a.full
