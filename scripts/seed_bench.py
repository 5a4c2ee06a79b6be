#!/usr/bin/env python3
"""Times mtgs_amd.seed: the neighbour search (mtgs_knn) and the fused seeding kernel (mtgs_seed_fwd) at N = 100 k, 500 k and 2 M
on a street-like cloud and a sky shell, next to what a user had before: (a) a chunked torch brute force on the same GPU at
100 k and (b) scikit-learn on this machine's host, when it can be imported.

    python scripts/seed_bench.py [--out profiles/seed_bench.txt] [--sklearn-n 2000000]

Every step is a child process of its own under its own time limit; the first step that fails or times out ends the run
(nothing else is started on the device after it)."""
import argparse
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def cloud(kind, n, dev):
    import torch
    from mtgs_amd import seed
    g = torch.Generator(device=dev).manual_seed(21)
    if kind == "sky":
        return seed.sky_points(n, 3000.0, 150.0, "spheric", generator=g, device=dev)["xyz"].contiguous()
    u = lambda m, lo, hi: torch.rand(m, device=dev, generator=g) * (hi - lo) + lo
    n_far, n_fac = max(n // 40, 8), n // 3
    n_gr = n - n_far - n_fac
    ground = torch.stack([u(n_gr, 0, 400), u(n_gr, -6, 6), torch.randn(n_gr, device=dev, generator=g) * 0.02], -1)
    side = torch.where(torch.rand(n_fac, device=dev, generator=g) < 0.5, -9.0, 9.0)
    facade = torch.stack([u(n_fac, 0, 400), side + torch.randn(n_fac, device=dev, generator=g) * 0.05, u(n_fac, 0, 20)], -1)
    far = torch.tensor([900.0, 400.0, 30.0], device=dev) + torch.randn(n_far, 3, device=dev, generator=g) * 40.0
    x = torch.cat([ground, facade, far])
    return x[torch.randperm(n, device=dev, generator=g)].contiguous()


def timed(fn, repeats):
    """median wall time in ms of fn(), each run ending in a device synchronise; one warm-up"""
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[len(ts) // 2]


def step_knn(kind, n):
    import torch
    from mtgs_amd import _lib, seed
    dev = torch.device("cuda")
    x = cloud(kind, n, dev)
    total = timed(lambda: seed.knn_distances(x, 3), 5)
    d = seed.knn_distances(x, 3)
    pts = {"xyz": x, "rgb": torch.full((n, 3), 128.0, device=dev), "normals": torch.randn(n, 3, device=dev)}
    _lib.time_calls(("mtgs_knn", "mtgs_seed_fwd"))
    for _ in range(5):
        seed.seed_gaussians(pts, 3)
    torch.cuda.synchronize()
    ms = {k: sorted(v)[len(v) // 2] for k, v in _lib.timed_ms().items()}
    _lib.time_calls(())
    print(f"{kind:6s} N={n:8d}  knn_distances {total:8.2f} ms wall   mtgs_knn {ms['mtgs_knn']:8.2f} ms   mtgs_seed_fwd {ms['mtgs_seed_fwd']:6.3f} ms"
          f"   mean neighbour distance {float(d.mean()):.4f}")


def step_brute(kind, n):
    """(a) what torch offers without a neighbour search: squared distances chunk by chunk, topk of 4, first column dropped"""
    import torch
    dev = torch.device("cuda")
    x = cloud(kind, n, dev)

    def run():
        out = []
        for s in range(0, n, 4096):
            d = torch.cdist(x[s:s + 4096], x, compute_mode="donot_use_mm_for_euclid_dist")
            out.append(torch.topk(d, 4, dim=1, largest=False).values[:, 1:])
        return torch.cat(out)

    print(f"{kind:6s} N={n:8d}  torch brute force (cdist + topk, 4096-row chunks) {timed(run, 3):8.2f} ms wall")


def step_sklearn(kind, n):
    """(b) the reference's call on this machine's host"""
    try:
        from sklearn.neighbors import NearestNeighbors
    except ImportError:
        print(f"{kind:6s} N={n:8d}  scikit-learn is not installed on this machine: not measured")
        return
    import torch
    x = cloud(kind, n, torch.device("cuda")).cpu().numpy()
    t0 = time.perf_counter()
    NearestNeighbors(n_neighbors=4, algorithm="auto", metric="euclidean").fit(x).kneighbors(x)
    print(f"{kind:6s} N={n:8d}  sklearn NearestNeighbors on the host {(time.perf_counter() - t0) * 1e3:10.1f} ms wall")


STEPS = {"knn": step_knn, "brute": step_brute, "sklearn": step_sklearn}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sklearn-n", type=int, default=2_000_000)
    ap.add_argument("--step", choices=list(STEPS))
    ap.add_argument("--kind", default="street")
    ap.add_argument("--n", type=int, default=100_000)
    a = ap.parse_args()
    if a.step:
        STEPS[a.step](a.kind, a.n)
        return 0
    plan = [("knn", kind, n, 240) for kind in ("street", "sky") for n in (100_000, 500_000, 2_000_000)]
    plan += [("brute", "street", 100_000, 240), ("brute", "sky", 100_000, 240), ("sklearn", "street", a.sklearn_n, 600)]
    lines = []
    for step, kind, n, limit in plan:
        cmd = [sys.executable, str(Path(__file__).resolve()), "--step", step, "--kind", kind, "--n", str(n)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            lines.append(f"{step} {kind} N={n}: no result within {limit} s; stopping")
            print(lines[-1], flush=True)
            break
        text = r.stdout.strip() if r.returncode == 0 else f"{step} {kind} N={n}: exit status {r.returncode}; stopping\n{r.stderr[-2000:]}"
        lines.append(text)
        print(text, flush=True)
        if r.returncode != 0:
            break
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")
    return 0 if len(lines) == len(plan) and "stopping" not in lines[-1] else 1


if __name__ == "__main__":
    sys.exit(main())
