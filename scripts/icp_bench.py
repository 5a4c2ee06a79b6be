#!/usr/bin/env python
"""Times mtgs_amd.registration on a synthetic street at an ASSUMED nuPlan top-lidar shape -- 35 000-point sweeps (64 elevations x 547
azimuths), max_range 200, voxel_size 2.0 -- that nobody has measured on real logs: ms per frame and us per ICP iteration with the
local map at 10 and at 200 frames, the frame time for several sizes of the iteration group, the bytes of the association kernel
against the HBM and Infinity Cache peaks, and the small sweep (24 x 120 rays, max_range 80) of the test scene, where launch and read
costs weigh most.  The 200 frames are eight traversals of 25 frames over the same stretch in three lanes, each anchored at its log pose as
MTGS's warm-up does.  (ONE drive of 200 frames down this street does not survive: from frame 38 on the heading error triples per frame
-- under the constant-velocity guess, with the adaptive threshold down to 0.55 m -- and the pose leaves the road at frame 43, in the
NumPy restatement exactly as on the device.  Whether kiss-icp itself survives that drive is not known.)

The host baseline is a vectorised NumPy / scipy.spatial.cKDTree formulation of the same frame on the same machine (np.unique
down-sampling, a k-d tree over the device's own map cloud built once per frame, tree queries, einsum sums, numpy.linalg.solve).  It is
NOT kiss-icp's TBB C++, which cannot be built where this project is tested.

Frame times are a host clock around `register_frame`, which ends in a device read; the iteration time is HIP events around one
`mtgs_icp_align_iterate` call of 64 iterations that cannot converge (convergence 0).  The share of the association kernel comes from a
run of its own under the profiler:

    python scripts/icp_bench.py [--out profiles/icp.txt] [--frames 200]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/icp_bench.py --trace        # 40 frames, nothing timed
    python scripts/icp_bench.py --kernel-stats <dir>/.../*_results.db                        # appends the shares to --out
"""
import argparse
import csv
import math
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from mtgs_amd import _lib, registration as G  # noqa: E402

HBM_PEAK, MALL_PEAK = 8.0e12, 14.0e12        # bytes / s: HBM3E, and the Infinity Cache's peak read rate (MI355X_MICROARCH.md)


def yaw_pose(x, y, z, yaw):
    c, s = math.cos(yaw), math.sin(yaw)
    return np.array([[c, -s, 0.0, x], [s, c, 0.0, y], [0.0, 0.0, 1.0, z], [0.0, 0.0, 0.0, 1.0]])


def street(rng, length=700.0):
    """a ground slab and buildings, parked cars and poles along a street of `length` metres: [B, 2, 3] axis-aligned boxes"""
    boxes = [[(-250.0, -250.0, -0.5), (length + 250.0, 250.0, 0.0)]]
    x = -200.0
    while x < length + 200.0:
        w, d, h = rng.uniform(12.0, 40.0), rng.uniform(10.0, 30.0), rng.uniform(6.0, 30.0)
        for side in (-1.0, 1.0):
            off = rng.uniform(14.0, 22.0)
            y0, y1 = sorted((side * off, side * (off + d)))
            boxes.append([(x, y0, 0.0), (x + w, y1, h * rng.uniform(0.6, 1.4))])
        x += w + rng.uniform(2.0, 15.0)
    for _ in range(int(length / 6)):
        cx, side = rng.uniform(-100.0, length + 100.0), rng.choice([-1.0, 1.0])
        boxes.append([(cx, side * 6.0 - 1.0, 0.0), (cx + rng.uniform(3.5, 5.5), side * 6.0 + 1.0, rng.uniform(1.4, 2.2))])
        px = rng.uniform(-100.0, length + 100.0)
        boxes.append([(px, -side * 9.0, 0.0), (px + 0.3, -side * 9.0 + 0.3, rng.uniform(4.0, 9.0))])
    return np.asarray(boxes)


def cast(boxes, pose, rng, n_el, n_az, el_range, max_t):
    el = np.deg2rad(np.linspace(*el_range, n_el))
    az = np.deg2rad(np.arange(n_az) * (360.0 / n_az))
    e, a = np.meshgrid(el, az, indexing="ij")
    # every ray turned by up to 0.3 degrees both ways: with exact rings point-to-point ICP locks the ring pattern of a sweep onto the
    # map's and the height drifts (0.8 m in 30 frames with exact elevations, 0.16 m with the jitter, NumPy restatement)
    a = a + np.deg2rad(rng.uniform(-0.3, 0.3, a.shape))
    e = e + np.deg2rad(rng.uniform(-0.3, 0.3, e.shape))
    d = np.stack([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)], -1).reshape(-1, 3)
    dw, o = d @ pose[:3, :3].T, pose[:3, 3]
    near_b = boxes[np.all((boxes[:, 0, :2] < o[:2] + max_t) & (boxes[:, 1, :2] > o[:2] - max_t), axis=1)]
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (near_b[None, :, 0, :] - o) / dw[:, None, :], (near_b[None, :, 1, :] - o) / dw[:, None, :]
    near, far = np.minimum(t0, t1).max(axis=2), np.maximum(t0, t1).min(axis=2)
    t = np.where((near <= far) & (far > 0.0), np.where(near > 0.0, near, far), np.inf).min(axis=1)
    hit = np.isfinite(t) & (t < max_t)
    r = t[hit] + rng.normal(0.0, 0.02, int(hit.sum()))
    return (d[hit] * r[:, None]).astype(np.float32)


PER_TRAVERSAL = 25       # frames of one traversal: the road block is driven again and again, as the reference's script registers it


def traversal_of(f):
    return f // PER_TRAVERSAL


def scene(frames, n_el, n_az, el_range, max_t, seed=0, step=2.5):
    """`frames` sweeps of traversals of PER_TRAVERSAL frames each over the same 60 m of the street, in one of three lanes"""
    rng = np.random.default_rng(seed)
    boxes = street(rng, 100.0)
    scans, true, log = [], [], []
    for f in range(frames):
        k, lane = f % PER_TRAVERSAL, traversal_of(f) % 3 - 1
        pose = yaw_pose(step * k, 1.75 * lane + 0.3 * math.sin(f / 15.0), 1.9, 0.02 * math.sin(f / 20.0))
        scans.append(cast(boxes, pose, rng, n_el, n_az, el_range, max_t))
        noisy = pose @ yaw_pose(0.0, 0.0, 0.0, np.deg2rad(rng.normal(0.0, 0.5)))
        noisy[:3, 3] = pose[:3, 3] + (rng.normal(0.0, 0.15, 3) if f else 0.0)
        true.append(pose)
        log.append(noisy)
    return scans, np.stack(true), np.stack(log)


# ---- the host baseline -------------------------------------------------------------------------------------------------------------------
def host_downsample(p, c):
    p = p.astype(np.float64)
    n = np.linalg.norm(p, axis=1)
    p = p[(n > c.min_range) & (n < c.max_range)]
    frame = p[np.sort(np.unique(np.floor(p / (0.5 * c.voxel_size)), axis=0, return_index=True)[1])]
    return frame, frame[np.sort(np.unique(np.floor(frame / (1.5 * c.voxel_size)), axis=0, return_index=True)[1])]


def host_frame(points, map_cloud, guess, c, sigma=2.0):
    """(pose, iterations) of one frame against a map given as a point cloud: NumPy / cKDTree, vectorised"""
    from scipy.linalg import expm
    from scipy.spatial import cKDTree
    frame, source = host_downsample(points, c)
    tree = cKDTree(map_cloud)
    src = source @ guess[:3, :3].T + guess[:3, 3]
    T, k = np.eye(4), sigma / 3.0
    for it in range(1, c.max_num_iterations + 1):
        d, i = tree.query(src, distance_upper_bound=3.0 * sigma)
        ok = np.isfinite(d)
        s, r = src[ok], src[ok] - map_cloud[i[ok]]
        w = k * k / (k + (r * r).sum(1)) ** 2
        J = np.zeros((len(s), 3, 6))
        J[:, :, :3] = np.eye(3)
        J[:, 0, 4], J[:, 0, 5], J[:, 1, 3], J[:, 1, 5], J[:, 2, 3], J[:, 2, 4] = s[:, 2], -s[:, 1], -s[:, 2], s[:, 0], s[:, 1], -s[:, 0]
        dx = np.linalg.solve(np.einsum("nij,n,nik->jk", J, w, J), -np.einsum("nij,n,ni->j", J, w, r))
        tw = np.zeros((4, 4))
        tw[:3, :3] = [[0.0, -dx[5], dx[4]], [dx[5], 0.0, -dx[3]], [-dx[4], dx[3], 0.0]]
        tw[:3, 3] = dx[:3]
        E = expm(tw)
        src = src @ E[:3, :3].T + E[:3, 3]
        T = E @ T
        if np.linalg.norm(dx) < c.convergence_criterion:
            break
    return T @ guess, it


# ---- the device runs -----------------------------------------------------------------------------------------------------------------------
def run_device(scans, log, config, group, capacity, marks=()):
    """(poses, per-frame ms, iterations, {frame: state at that frame}) of one odometry run; the scans are uploaded beforehand"""
    odo = G.LidarOdometry(config, capacity=capacity, group_size=group)
    ms, poses, kept = [], [], {}
    for f, (scan, pose) in enumerate(zip(scans, log)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        poses.append(odo.register_frame(scan, pose, traversal_of(f)))
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        if not np.isfinite(poses[-1]).all() or np.linalg.norm(poses[-1][:3, 3] - pose[:3, 3]) > 5.0:      # 5 m from the log pose
            ds = odo._last_downsample
            odo.left_the_road = (f"the odometry left the road at frame {f}: iterations {odo.iterations[-6:]}, status {odo.last_status}, counts "
                                 f"{ds.counts.cpu().tolist()}, map {odo.local_map.status()}, pose {poses[-1][:3, 3]}, log pose {pose[:3, 3]}")
            poses.pop(), ms.pop(), odo.iterations.pop()
            break
        if f + 1 in marks:
            kept[f + 1] = iteration_us(odo, scan, config) + (association_bytes(odo, scan, config),)
    if not hasattr(odo, "left_the_road"):
        odo.check()
    return np.stack(poses), np.array(ms), np.array(odo.iterations), kept, odo


def iteration_us(odo, scan, config, n=64):
    """(us per iteration, source points): HIP events around one group of n iterations that cannot converge, median of 7"""
    ds = G.downsample(scan, config)
    S = scan.shape[0]
    rec = torch.empty(G.RECORD, dtype=torch.float64, device=scan.device)
    guess = torch.from_numpy(odo.last_pose[:3].reshape(12).copy()).to(scan.device)
    ws = _lib.workspace("mtgs_icp_align_workspace_bytes", S, device=scan.device, dtype=torch.uint8)
    st = _lib.stream_of(scan)
    times = []
    for _ in range(9):
        _lib.call("mtgs_icp_align_begin", S, _lib.ptr(ds.source), 1, 3, _lib.ptr(ds.counts[1:]), _lib.ptr(guess), _lib.ptr(rec), _lib.ptr(ws), ws.numel(), st)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _lib.call("mtgs_icp_align_iterate", *odo.local_map._args(), config.voxel_size, S, _lib.ptr(ds.counts[1:]), 6.0, 2.0 / 3.0, 0.0, n,
                  _lib.ptr(rec), _lib.ptr(ws), ws.numel(), st)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e3 / n)
    if int(rec[25].item()) != n or int(rec[27].item()) != 0:
        raise RuntimeError(f"the timed group did not run {n} iterations: record {rec[24:28].cpu().tolist()}, guess {odo.last_pose[:3, 3]}, map {odo.local_map.status()}")
    return float(np.median(times[2:])), int(ds.counts[1].item())


def association_bytes(odo, scan, config):
    """the bytes one association needs, from the counts: per source point its row read and written (48), per probe a binary search over
    the table's keys (ceil(log2 V) x 8), per found voxel its slot and count (8), per candidate a point (24); plus 176 per block"""
    ds = G.downsample(scan, config)
    src = ds.trimmed()[1].cpu().numpy() @ odo.last_pose[:3, :3].T + odo.last_pose[:3, 3]
    cloud = odo.local_map.point_cloud().cpu().numpy()
    vs = config.voxel_size
    key = lambda v: ((v[..., 0] + (1 << 20)) << 42) | ((v[..., 1] + (1 << 20)) << 21) | (v[..., 2] + (1 << 20))
    keys, counts = np.unique(key(np.floor(cloud / vs).astype(np.int64)), return_counts=True)
    off = np.array([[i, j, k] for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)])
    probe = key(np.floor(src / vs).astype(np.int64)[:, None, :] + off[None])
    at = np.minimum(np.searchsorted(keys, probe), len(keys) - 1)
    found = keys[at] == probe
    voxels = odo.local_map.status()[0]
    S = len(src)
    return int(S * 48 + S * 27 * math.ceil(math.log2(max(voxels, 2))) * 8 + found.sum() * 8 + (counts[at] * found).sum() * 24 + -(-S // 256) * 176)


def fmt(ms):
    return f"{np.mean(ms):7.3f} ms (min {np.min(ms):.3f}, max {np.max(ms):.3f})"


def kernel_shares(path, out):
    """The kernels of the traced run by total time, from the profiler's result database (its `kernels` view) or a kernel_stats.csv;
    the frame's own kernels are told from torch's copies and fills by name."""
    if str(path).endswith(".db"):
        import sqlite3
        rows = sqlite3.connect(path).execute("select name, count(*), sum(duration) from kernels group by name").fetchall()
    else:
        rows = [(r.get("Name") or r.get("KernelName") or "", int(float(r.get("Calls") or 0)), float(r.get("TotalDurationNs") or 0.0))
                for r in csv.DictReader(open(path))]
    ours = [r for r in rows if any(k in r[0] for k in ("associate_kernel", "finish_kernel", "ds_key", "ds_flag", "ins_key", "merge_", "insert_kernel", "commit_kernel",
                                                       "prune_kernel", "begin_kernel", "map_init", "mtgs_sort", "mtgs_scan", "zero"))]
    all_ns = float(sum(r[2] for r in ours))
    lines = [f"kernel shares of a traced run (52 frames, rocprofv3 --kernel-trace; the library's kernels: {all_ns / 1e6:.1f} ms in all, everything else on the "
             f"device {sum(r[2] for r in rows if r not in ours) / 1e6:.1f} ms)"]
    for name, calls, total in sorted(ours, key=lambda r: r[2], reverse=True)[:8]:
        lines.append(f"    {100.0 * total / all_ns:5.1f} %  {total / max(calls, 1) / 1e3:8.2f} us x {calls:6d}  {name[:110]}")
    with open(out, "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "icp.txt"))
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--trace", action="store_true", help="40 frames of the large shape and nothing else: the run to put under the profiler")
    ap.add_argument("--kernel-stats", help="a kernel_stats.csv of a traced run: append the kernels' shares to --out")
    args = ap.parse_args()
    if args.kernel_stats:
        return kernel_shares(args.kernel_stats, args.out)
    assert torch.cuda.is_available(), "icp_bench needs the GPU: nothing here is a timing without one"
    dev = torch.device("cuda")
    big = G.KissConfig(max_range=200.0)
    frames = 40 if args.trace else args.frames
    scans, true, log = scene(frames, 64, 547, (-25.0, 15.0), 220.0)
    d_scans = [torch.from_numpy(s).to(dev) for s in scans]
    run_device(d_scans[:12], log[:12], big, G.GROUP_SIZE, 1 << 18)               # warm-up: code objects, allocator
    if args.trace:
        run_device(d_scans, log, big, G.GROUP_SIZE, 1 << 18)
        return
    class Report(list):          # written out after every line: a run that stops keeps what it measured
        def append(self, line):
            super().append(line)
            Path(args.out).write_text("\n".join(self) + "\n")
            print(line, flush=True)
    L = Report()
    report = L.append
    report(f"icp_bench: {torch.cuda.get_device_name(0)}; a frame is a host clock around register_frame (it ends in a device read); an iteration is HIP "
           f"events around 64 iterations in one group, median of 7")
    report(f"ASSUMED shape, not measured on real logs: sweeps of {int(np.mean([len(s) for s in scans]))} float32 points (64 x 547 rays on a synthetic street), "
           f"max_range 200, voxel_size 2.0, 2.5 m between frames; {frames} frames in traversals of {PER_TRAVERSAL} over the same stretch")
    marks = tuple(m for m in (10, 200) if m <= frames)
    poses, ms, its, kept, odo = run_device(d_scans, log, big, G.GROUP_SIZE, 1 << 18, marks)
    if hasattr(odo, "left_the_road"):
        report(odo.left_the_road + f"; everything below is over the {len(poses)} frames before it")
    frames, true, log = len(poses), true[:len(poses)], log[:len(poses)]
    d_scans, scans = d_scans[:frames], scans[:frames]
    marks = tuple(m for m in marks if m in kept)
    err = lambda p: float(np.linalg.norm(p[:, :3, 3] - true[:, :3, 3], axis=1).mean())
    voxels, _, live = odo.local_map.status()
    L.append(f"registration: mean translational error {err(log):.3f} m (log poses) -> {err(poses):.3f} m; iterations per frame min {its[1:].min()}, "
             f"median {int(np.median(its[1:]))}, max {its[1:].max()}; the map ends with {voxels} voxels ({live} hold points)")
    poses2 = run_device(d_scans, log, big, G.GROUP_SIZE, 1 << 18)[0]
    L.append(f"a second run repeats every bit of every pose: {np.array_equal(poses.view(np.int64), poses2.view(np.int64))}")
    cloud = {}
    for m in marks:
        lo, hi = max(m - 8, 1), min(m + 2, frames)
        us, S, nbytes = kept[m]
        L.append(f"map at {m} frames: register_frame {fmt(ms[lo:hi])} over frames {lo}..{hi - 1} with {its[lo:hi].mean():.1f} iterations on average; "
                 f"{S} source points")
        L.append(f"    one iteration (associate + finish) {us:.1f} us; the association needs {nbytes / 1e6:.2f} MB -> {nbytes / us / 1e3:.1f} GB/s over the WHOLE "
                 f"iteration = {100 * nbytes / (us * 1e-6) / HBM_PEAK:.2f} % of the {HBM_PEAK / 1e12:.1f} TB/s HBM peak, {100 * nbytes / (us * 1e-6) / MALL_PEAK:.2f} % of "
                 f"the Infinity Cache's {MALL_PEAK / 1e12:.0f} TB/s: latency-bound (27 dependent binary searches per lane), not bandwidth-bound")
    L.append("iteration group (frames 10.. of the same run, mean ms per frame; the group in use is %d):" % G.GROUP_SIZE)
    sub = min(frames, 60)
    for group in (1, 2, 4, 8, 16, 32):
        t = [run_device(d_scans[:sub], log[:sub], big, group, 1 << 18)[1][10:].mean() for _ in range(3)]
        L.append(f"    group {group:2d}: {np.median(t):.3f} ms (three runs: {', '.join(f'{v:.3f}' for v in t)})")
    # the host formulation against the device's own map, at the marked frames
    for m in marks:
        odo_m = G.LidarOdometry(big, capacity=1 << 18)
        for f in range(m - 1):
            odo_m.register_frame(d_scans[f], log[f], traversal_of(f))
        cloud = odo_m.local_map.point_cloud().cpu().numpy()
        f = m - 1
        guess = odo_m.last_pose @ odo_m.last_delta
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            pose_h, it_h = host_frame(scans[f], cloud, guess, big)
            t.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        pose_d = odo_m.register_frame(d_scans[f], log[f], traversal_of(f))
        torch.cuda.synchronize()
        t_d = (time.perf_counter() - t0) * 1e3
        L.append(f"host (NumPy / cKDTree over the same map, {len(cloud)} points; NOT kiss-icp's C++) frame {f}: {fmt(t)}, {it_h} iterations, against "
                 f"{t_d:.3f} ms and {odo_m.iterations[-1]} iterations on the device = {np.median(t) / t_d:.1f} x; |t_host - t_device| = "
                 f"{np.linalg.norm(pose_h[:3, 3] - pose_d[:3, 3]):.3f} m")
    # the small shape
    small = G.KissConfig(max_range=80.0, voxel_size=0.8)
    s_scans, s_true, s_log = scene(30, 24, 120, (-12.0, 12.0), 100.0, seed=1)
    sd = [torch.from_numpy(s).to(dev) for s in s_scans]
    run_device(sd[:5], s_log[:5], small, G.GROUP_SIZE, 1 << 16)
    _, s_ms, s_its, _, s_odo = run_device(sd, s_log, small, G.GROUP_SIZE, 1 << 16)
    cloud = s_odo.local_map.point_cloud().cpu().numpy()
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        _, it_h = host_frame(s_scans[-1], cloud, s_odo.last_pose, small)
        t.append((time.perf_counter() - t0) * 1e3)
    L.append(f"small sweeps ({int(np.mean([len(s) for s in s_scans]))} points, max_range 80, voxel_size 0.8): register_frame {fmt(s_ms[10:])} with "
             f"{s_its[10:].mean():.1f} iterations; host formulation of the last frame (already converged guess) {fmt(t)}, {it_h} iterations")
    # the recorded traversals of the tests (tests/golden/icp_ref.npz): the device against the NumPy restatement's poses
    with np.load(ROOT / "tests" / "golden" / "icp_ref.npz") as z:
        g = {k: z[k] for k in z.files}
    g_scans = [torch.from_numpy(g["points"][a:b]).to(dev) for a, b in zip(g["offsets"][:-1], g["offsets"][1:])]
    g_poses, g_its = G.register_traversals(g_scans, g["log_poses"], g["traj_ids"], small, capacity=1 << 16)
    L.append(f"recorded traversals (2 x 5 frames): largest difference of a pose entry from the NumPy restatement's poses {np.abs(g_poses - g['poses']).max():.3g} "
             f"(allowed 64 d = {64 * float(g['d']):.3g}); iteration counts equal: {np.array_equal(g_its, g['iterations'])}")


if __name__ == "__main__":
    main()
