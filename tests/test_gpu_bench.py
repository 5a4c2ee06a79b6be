"""bench.py's plain line and --dump-outputs on the GPU, at a small size: K timed steps, no --full extras, and the outputs of the
graph-replayed step equal those of the eager loop on the same inputs."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def _bench(out_dir, *extra):
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--n-gaussians", "50000",
           "--width", "640", "--height", "480", "--dump-outputs", str(out_dir)] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_line_and_dumped_outputs(tmp_path, hip_lib):
    graph = _bench(tmp_path / "graph")
    assert graph["steps"] == 3 and graph["ms_per_step"] > 0 and graph["unit"] == "Mpix/s" and graph["dtype"] == "f32"
    assert graph["config"]["launch"].startswith("one HIP graph launch") == (graph["ms_per_step"] == graph["ms_per_step_graph"])
    assert "also" not in graph and "cpu_baseline" not in graph and graph["roofline"]["entry_points"] is None
    assert graph["ms_per_step_tight_lists"] is None
    eager = _bench(tmp_path / "eager", "--launch", "eager")
    assert eager["ms_per_step"] == eager["ms_per_step_eager"] and eager["ms_per_step_graph"] is None
    names = sorted(p.name for p in (tmp_path / "graph").glob("*.npy"))
    assert names == sorted(p.name for p in (tmp_path / "eager").glob("*.npy")) == sorted(
        f"{n}.npy" for n in ("render", "alpha", "grad_means", "grad_quats", "grad_scales", "grad_opacities", "grad_coeffs", "grad_viewmat"))
    for n in names:
        g, e = np.load(tmp_path / "graph" / n), np.load(tmp_path / "eager" / n)
        assert g.dtype == np.float32 and g.shape == e.shape and np.isfinite(g).all(), n
        assert np.abs(e).max() > 0, n
        np.testing.assert_allclose(g, e, rtol=1e-3, atol=1e-5 * float(np.abs(e).max()), err_msg=n)
    assert np.load(tmp_path / "graph" / "render.npy").shape == (1, 480, 640, 4)
