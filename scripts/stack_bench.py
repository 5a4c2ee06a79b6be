#!/usr/bin/env python
"""Times mtgs_amd.stack at the sizes a user runs: `split_sweep` and a whole `SweepStack.add_frame` on a sweep of 120 000 points with 8
cameras of 1920 x 1080, for 20 and for 100 boxes, and `SweepStack.finish` for a traversal of 40 and of 300 frames.  Each against two
baselines on the same machine:

    host     the reference's formulation on the host: the loop over the boxes in torch fp64 on the CPU (one [N, 4] x [4, 4] product
             and two masked copies of the remaining sweep per box), NumPy concatenation for the traversal, with the upload of the result
    torch    the same formulas as torch operations on device tensors: every box's product at once, the first owner by argmax, a
             stable sort by slot; boolean-mask indexing and concatenation for the traversal (a host read per mask)

Device times are HIP events around windows of repeated calls (median of the windows); times of work that reads back to the host are a
wall clock around work that ends in a device synchronise.  The partition's and the gather's achieved rates are the bytes the
algorithm needs (computed from the counts) over the event time of the entry point, against the HBM peak.  Writes profiles/stack.txt.

    python scripts/stack_bench.py [--out profiles/stack.txt] [--windows 5] [--frames 40 300]
"""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

from lidar_bench import HBM_PEAK, camera, device_ms, fmt, sweep, wall_ms  # noqa: E402
from mtgs_amd import _lib, stack  # noqa: E402

N, CAMERAS, WIDTH, HEIGHT = 120_000, 8, 1920, 1080


def boxes_in_the_sweep(rng, n_boxes, pts, per_box=60):
    """car-sized boxes 5 to 55 m from the sensor, every fifth one overlapping its neighbour, and per_box points of the sweep moved
    into and around each of them"""
    r, a = rng.uniform(5.0, 55.0, n_boxes), rng.uniform(0.0, 2 * np.pi, n_boxes)
    b = np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(0.0, 1.0, n_boxes), rng.uniform(3.0, 5.0, n_boxes), rng.uniform(1.5, 2.2, n_boxes),
                  rng.uniform(1.4, 2.0, n_boxes), rng.uniform(-np.pi, np.pi, n_boxes)], -1)
    b[1::5, :3] = b[0::5][: len(b[1::5]), :3] + [1.0, 0.2, 0.0]
    pts = pts.astype(np.float64)
    for box in b:
        c, s = np.cos(box[6]), np.sin(box[6])
        local = rng.uniform(-1.0, 1.0, (per_box, 3)) * (box[3:6] / 2 + 0.3)
        where = rng.choice(len(pts), per_box, replace=False)
        pts[where] = np.stack([c * local[:, 0] - s * local[:, 1] + box[0], s * local[:, 0] + c * local[:, 1] + box[1], local[:, 2] + box[2]], -1)
    return b, pts.astype(np.float32)


# ---- the two baselines of the split -----------------------------------------------------------------------------------------------------
def host_split(points, lidar2box, sizes, include, fill=0.25):
    """the reference's loop in torch fp64 on the CPU: (background [M, 3], [box-frame points per included box])"""
    rest = torch.cat([points.to(torch.float64), torch.ones((points.shape[0], 1), dtype=torch.float64)], dim=-1)
    inside = []
    for b in range(lidar2box.shape[0]):
        if not include[b]:
            continue
        q = rest @ lidar2box[b].T
        a = q[:, :3].abs()
        inflated = (a <= (sizes[b] + fill) / 2).all(1)
        tight = (a <= sizes[b] / 2).all(1)
        inside.append(q[tight][:, :3])
        rest = rest[~inflated]
    return rest[:, :3], inside


def torch_split(points, lidar2box, sizes, include, fill=0.25):
    """the rule as torch operations on device tensors, no host read: (rows [N, 3] in group order, slot [N], counts [B + 2])"""
    B = lidar2box.shape[0]
    x = torch.cat([points.to(torch.float64), torch.ones((points.shape[0], 1), dtype=torch.float64, device=points.device)], dim=-1)
    q = torch.einsum("bkj,nj->bnk", lidar2box[:, :3], x)                                  # [B, N, 3]
    a = q.abs()
    inflated = (a <= ((sizes + fill) / 2)[:, None, :]).all(-1) & include[:, None]
    owned = inflated.any(0)
    owner = torch.argmax(inflated.to(torch.uint8), dim=0)                                 # the first True
    mine = q.gather(0, owner[None, :, None].expand(1, -1, 3))[0]
    tight = (mine.abs() <= (sizes / 2)[owner]).all(-1)
    slot = torch.where(owned, torch.where(tight, owner + 1, torch.full_like(owner, B + 1)), torch.zeros_like(owner))
    order = torch.sort(slot, stable=True).indices
    rows = torch.where((slot == 0)[:, None], x[:, :3], mine)[order]
    return rows, slot, torch.bincount(slot, minlength=B + 2)


# ---- the two baselines of the traversal ---------------------------------------------------------------------------------------------------
def concat_traversal(frames, xp):
    """frames: (points, rgb, labels, offsets as a host list, tokens of the slots, lidar2global) in NumPy (xp = np) or torch"""
    cat = np.concatenate if xp is np else torch.cat
    xyz, rgb, labels, tracks = [], [], [], {}
    for pts, col, lab, off, tokens, g in frames:
        keep = lab[: off[1]] < 10
        p = pts[: off[1]][keep]
        xyz.append(p @ g[:3, :3].T + g[:3, 3])
        rgb.append(col[: off[1]][keep])
        labels.append(lab[: off[1]][keep])
        for slot, token in tokens:
            tracks.setdefault(token, []).append((pts[off[slot]: off[slot + 1]], col[off[slot]: off[slot + 1]]))
    return cat(xyz), cat(rgb), cat(labels), {t: (cat([a for a, _ in v]), cat([b for _, b in v])) for t, v in tracks.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "stack.txt"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--boxes", type=int, nargs="+", default=[20, 100])
    ap.add_argument("--frames", type=int, nargs="+", default=[40, 300])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "stack_bench needs a HIP device"
    dev = torch.device("cuda")
    rng = np.random.default_rng(7)
    lines = [f"stack_bench: {torch.cuda.get_device_name(0)}; device times are HIP events, median of {a.windows} windows of >= 0.2 s; times of "
             "work that reads back to the host are wall clocks that end in a synchronise",
             f"a sweep of {N} float32 points, {CAMERAS} cameras of {WIDTH} x {HEIGHT}"]

    def say(line):
        print(line, flush=True)
        lines.append(line)

    mats = np.stack([camera(45.0 * c, 1100.0, rng.uniform(-0.5, 0.5, 3), WIDTH, HEIGHT)[0] for c in range(CAMERAS)])
    images = torch.randint(0, 256, (CAMERAS, HEIGHT, WIDTH, 3), dtype=torch.uint8, device=dev)
    masks = torch.randint(0, 20, (CAMERAS, HEIGHT, WIDTH, 1), dtype=torch.uint8, device=dev)
    d_mats = torch.from_numpy(mats).to(dev)
    base = sweep(rng, N)
    scenes = {}
    for B in a.boxes:
        boxes, pts = boxes_in_the_sweep(rng, B, base)
        scenes[B] = (boxes, pts)
        include = np.ones(B, dtype=bool)
        include[3::7] = False
        d_pts = torch.from_numpy(pts).to(dev)
        table = stack.upload_boxes(boxes, include)
        lidar2box = torch.from_numpy(stack.box_matrices(boxes)[0])
        sizes = torch.from_numpy(boxes[:, 3:6])
        h_pts, h_inc = torch.from_numpy(pts), torch.from_numpy(include)
        got = stack.split_sweep(d_pts, table)
        offsets = got.offsets.cpu().numpy()
        bg, inside = host_split(h_pts, lidar2box, sizes, h_inc)
        rows, slot, counts = torch_split(d_pts, lidar2box.to(dev), sizes.to(dev), h_inc.to(dev))
        sizes_host = [len(bg)] + [len(p) for p in inside]
        same = (np.diff(offsets)[: B + 1][np.concatenate([[True], include])].tolist() == sizes_host and torch.equal(got.points[: offsets[1]], bg.to(dev))
                and torch.equal(counts[: B + 1].cpu(), torch.from_numpy(np.diff(offsets)[: B + 1])))
        near = float((got.points[: offsets[-1]] - rows[: offsets[-1]]).abs().max())
        say(f"split_sweep B={B} ({int(include.sum())} included): background {offsets[1]}, in boxes {offsets[-1] - offsets[1]}, dropped {N - offsets[-1]}; "
            f"group sizes and background equal to the host loop and to torch on the device: {same}; max |rows - torch| {near:.3g}")
        t_dev = device_ms(lambda: stack.split_sweep(d_pts, table), a.windows)
        t_up = wall_ms(lambda: stack.split_sweep(torch.from_numpy(pts).to(dev), boxes, include), 20)
        t_host = wall_ms(lambda: [t.to(dev) for t in (lambda r: [r[0]] + r[1])(host_split(h_pts, lidar2box, sizes, h_inc))], 5)
        l2b_d, sizes_d, inc_d = lidar2box.to(dev), sizes.to(dev), h_inc.to(dev)
        t_torch = device_ms(lambda: torch_split(d_pts, l2b_d, sizes_d, inc_d), a.windows)
        say(f"    mtgs_amd.stack.split_sweep             {fmt(t_dev)}   with the sweep's and the boxes' upload {fmt(t_up)}")
        say(f"    host loop (torch fp64 CPU) + upload    {fmt(t_host)}   = {t_host[0] / t_up[0]:.1f} x the device path with its uploads")
        say(f"    torch on the device                    {fmt(t_torch)}   = {t_torch[0] / t_dev[0]:.1f} x split_sweep")
        # the partition alone: the radix sort of (slot, index) as mtgs_stack_split runs it
        bits = max(1, int(B + 1).bit_length())
        keys = torch.where(got.slot < 0, torch.full_like(got.slot, B + 1), got.slot).contiguous()
        vals = torch.arange(N, dtype=torch.int32, device=dev)
        ko, vo = torch.empty_like(keys), torch.empty_like(vals)
        ws = _lib.workspace("mtgs_sort_u32_workspace_bytes", N, device=dev, dtype=torch.uint8)
        st = torch.cuda.current_stream().cuda_stream
        t_sort = device_ms(lambda: _lib.call("mtgs_sort_pairs_u32", N, bits, keys.data_ptr(), vals.data_ptr(), ko.data_ptr(), vo.data_ptr(),
                                             ws.data_ptr(), ws.numel(), st), a.windows)
        passes = -(-bits // 8)
        need = passes * (N * 4 + 2 * N * 8)
        say(f"    partition: {passes} pass(es) on {bits} key bits, {need / 1e6:.2f} MB needed in {t_sort[0]:.3f} ms -> {need / t_sort[0] / 1e6:.1f} GB/s = "
            f"{100 * need / (t_sort[0] * 1e-3) / HBM_PEAK:.2f} % of the {HBM_PEAK / 1e12:.1f} TB/s HBM peak")
        # a whole frame
        names, tokens = ["vehicle" if i else "barrier" for i in include], [f"t{i}" for i in range(B)]

        def frame():
            s = stack.SweepStack()
            s.add_frame(d_pts, boxes, names, tokens, np.eye(4), d_mats, images, masks)
        t_frame = device_ms(frame, a.windows)
        t_stack = device_ms(lambda: stack.stack_frame(d_pts, table, d_mats, images, masks), a.windows)
        say(f"    SweepStack.add_frame (boxes uploaded)  {fmt(t_frame)}   stack_frame on an uploaded table {fmt(t_stack)}")
    # ---- the traversal -------------------------------------------------------------------------------------------------------------
    boxes, pts = scenes[a.boxes[0]]
    B = len(boxes)
    d_pts = torch.from_numpy(pts).to(dev)
    for F in a.frames:
        s = stack.SweepStack()
        for f in range(F):
            moved = boxes.copy()
            moved[:, :2] += [0.05 * f, 0.02 * f]
            g = np.eye(4)
            g[:3, 3] = [664430.0 + 0.5 * f, 3997650.0, 606.0]
            tokens = [f"t{(f // 10) * (B // 4) + i}" for i in range(B)]                   # a quarter of the tracks changes every 10 frames
            s.add_frame(d_pts, moved, ["vehicle"] * B, tokens, g, d_mats, images, masks)
        clouds = s.finish()
        torch.cuda.synchronize()
        rows = clouds.background[0].shape[0] + sum(v[0].shape[0] for v in clouds.instances.values())
        t_fin = wall_ms(s.finish, 10)
        _lib.time_calls(("mtgs_stack_plan", "mtgs_stack_gather"))
        for _ in range(10):
            s.finish()
        torch.cuda.synchronize()
        timed = {k: float(np.median(v)) for k, v in _lib.timed_ms().items()}
        _lib.time_calls(())
        need = rows * 2 * (24 + 24 + 4) + clouds.background[0].shape[0] * 4
        # the baselines read the frames as they are on the device / on the host
        d_frames = [(fr.points, fr.rgb, fr.labels, fr.offsets.cpu().tolist(), slots, torch.from_numpy(g).to(dev)) for fr, g, slots in s._frames]
        h_frames = [(p.cpu().numpy(), c.cpu().numpy(), l.cpu().numpy(), o, t, g.cpu().numpy()) for p, c, l, o, t, g in d_frames]
        want = concat_traversal(d_frames, torch)
        same = torch.equal(want[2], clouds.background[2]) and float((want[0] - clouds.background[0]).abs().max()) < 1e-6
        t_torch = wall_ms(lambda: concat_traversal(d_frames, torch), 5)
        t_host = wall_ms(lambda: [torch.from_numpy(x).to(dev) for x in concat_traversal(h_frames, np)[:3]], 3)
        say(f"finish F={F}: {clouds.background[0].shape[0]} background rows, {len(clouds.instances)} tracks with points, {rows} rows in all; labels equal "
            f"to torch on the device and |xyz - torch| < 1e-6: {same}")
        say(f"    SweepStack.finish (one host read)      {fmt(t_fin)}   of it plan {timed['mtgs_stack_plan']:.3f} ms, gather {timed['mtgs_stack_gather']:.3f} ms")
        say(f"    gather: {need / 1e6:.1f} MB needed -> {need / timed['mtgs_stack_gather'] / 1e6:.1f} GB/s = "
            f"{100 * need / (timed['mtgs_stack_gather'] * 1e-3) / HBM_PEAK:.2f} % of the {HBM_PEAK / 1e12:.1f} TB/s HBM peak")
        say(f"    torch on the device (masks, cat)       {fmt(t_torch)}   = {t_torch[0] / t_fin[0]:.1f} x finish")
        say(f"    host (NumPy) + upload of the background {fmt(t_host)}   = {t_host[0] / t_fin[0]:.1f} x finish (the frames already on the host)")
        del s, clouds, d_frames, h_frames, want
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
