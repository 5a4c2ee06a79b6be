"""The reference of mtgs_amd.registration (tests/test_icp_host.py, tests/test_gpu_icp.py): the KISS-ICP odometry in the canonical order
include/mtgs_icp.h states, restated in NumPy and plain Python floats, operation by operation -- every product and sum below is one
IEEE double operation, as the kernels' are under -ffp-contract=off.  Nothing here imports mtgs_amd.

    downsample(points, min_range, max_range, voxel_size)   -> frame, source, frame_index, source_index
    RefMap(voxel_size, max_points, capacity)               insert / prune / point_cloud / empty / tables
    associate(source, map, max_distance, kernel)           -> nn_index, distance, mask, contributions [S, 28]
    tree_sums(contributions, rows)                         the 28 sums in the kernels' order (block tree, block partials, tree)
    ldlt_solve, se3_exp, compose, inverse                  the written-out solver, the closed-form exponential, 3 x 4 algebra
    align(source, map, guess, ...)                         -> pose [4, 4], iterations, status
    RefOdometry(config).register_frame(points, log_pose, traj_id);   register_traversals(scans, log_poses, traj_ids, config)
    make_scene(seed)                                       the ray-cast test scene;  golden() / write_golden()

Run `python -m tests.icp_refs` from the repository root to rewrite tests/golden/icp_ref.npz."""
from __future__ import annotations

import math
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden" / "icp_ref.npz"
BLOCK = 256
HALF = 1 << 20
CONVERGED, DEGENERATE, EMPTY_MAP = 1, 2, 4
# the summed columns: contributions 0..14 and 21..27 (15..20 are identically zero)
COLUMNS = list(range(15)) + list(range(21, 28))
DBL_MAX = np.finfo(np.float64).max


# ---- voxels and down-sampling ----------------------------------------------------------------------------------------------------------
def voxels(points, size):
    """floor(p / size) per axis as int64 [N, 3] and ok [N]: inside [-2^20, 2^20) on every axis"""
    f = np.floor(np.asarray(points, dtype=np.float64) / np.float64(size))
    with np.errstate(invalid="ignore"):
        ok = ((f >= -HALF) & (f < HALF)).all(axis=1)
    return np.where(ok[:, None], f, 0.0).astype(np.int64), ok


def pack(v):
    v = np.asarray(v, dtype=np.int64)
    return ((v[..., 0] + HALF) << 42) | ((v[..., 1] + HALF) << 21) | (v[..., 2] + HALF)


def first_per_voxel(points, size):
    """(indices of the point of least index in every voxel, ascending; whether a point fell outside the grid)"""
    v, ok = voxels(points, size)
    idx = np.flatnonzero(ok)
    keys = pack(v[idx])
    order = np.argsort(keys, kind="stable")
    ks = keys[order]
    head = np.ones(len(ks), dtype=bool)
    head[1:] = ks[1:] != ks[:-1]
    return np.sort(idx[order[head]]), bool((~ok).any())


def downsample(points, min_range, max_range, voxel_size):
    p = np.asarray(points).astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    norm = np.sqrt((x * x + y * y) + z * z)
    with np.errstate(invalid="ignore"):
        kept = np.flatnonzero((norm < max_range) & (norm > min_range))
    i1, bad1 = first_per_voxel(p[kept], 0.5 * voxel_size)
    frame_index = kept[i1]
    frame = p[frame_index]
    i2, bad2 = first_per_voxel(frame, 1.5 * voxel_size)
    return frame, frame[i2], frame_index.astype(np.int32), frame_index[i2].astype(np.int32), int(bad1 or bad2)


def apply34(m, p):
    """rows ((m0 x + m1 y) + m2 z) + m3 of a 3 x 4 (or 4 x 4) m over points [N, 3]"""
    m = np.asarray(m, dtype=np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((m[k, 0] * x + m[k, 1] * y) + m[k, 2] * z) + m[k, 3] for k in range(3)], axis=1)


def sq(a, b):
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


# ---- the map -------------------------------------------------------------------------------------------------------------------------
class RefMap:
    """key -> ordered list of points; a voxel emptied by prune keeps its entry (and its slot) with an empty list"""

    def __init__(self, voxel_size, max_points=20, capacity=1 << 20):
        self.voxel_size, self.max_points, self.capacity = float(voxel_size), int(max_points), int(capacity)
        self.lists = {}
        self.status = 0
        self._tables = None

    def insert(self, points, pose=None):
        p = np.asarray(points).astype(np.float64)
        if pose is not None:
            p = apply34(pose, p)
        v, ok = voxels(p, self.voxel_size)
        if not ok.all():
            self.status |= 1
        idx = np.flatnonzero(ok)
        keys = pack(v[idx])
        order = np.argsort(keys, kind="stable")
        ks = keys[order]
        starts = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]]) if len(ks) else np.zeros(0, dtype=np.int64)
        new = [int(ks[s]) for s in starts if int(ks[s]) not in self.lists]
        if len(self.lists) + len(new) > self.capacity:
            self.status |= 2
            return
        self._tables = None
        resolution = math.sqrt(self.voxel_size * self.voxel_size / self.max_points)
        ends = np.r_[starts[1:], len(ks)]
        for s, e in zip(starts, ends):
            held = self.lists.setdefault(int(ks[s]), [])
            for o in idx[order[s:e]]:
                if len(held) == self.max_points:
                    break
                if held and bool((np.sqrt(sq(np.asarray(held), p[o])) < resolution).any()):
                    continue
                held.append(p[o])

    def prune(self, origin, max_distance):
        origin = np.asarray(origin, dtype=np.float64)
        for held in self.lists.values():
            if held and sq(held[0], origin) >= max_distance * max_distance:
                self._tables = None
                held.clear()

    def empty(self):
        return not any(self.lists.values())

    def point_cloud(self):
        rows = [q for key in sorted(self.lists) for q in self.lists[key]]
        return np.asarray(rows, dtype=np.float64).reshape(-1, 3)

    def tables(self):
        """(sorted keys [V], counts [V], points [V, max_points, 3]) for the vectorised neighbour search"""
        if self._tables is None:
            keys = np.array(sorted(self.lists), dtype=np.int64)
            cnt = np.array([len(self.lists[int(k)]) for k in keys], dtype=np.int64)
            pts = np.zeros((len(keys), self.max_points, 3))
            for i, k in enumerate(keys):
                if cnt[i]:
                    pts[i, :cnt[i]] = np.asarray(self.lists[int(k)])
            self._tables = keys, cnt, pts
        return self._tables


# ---- association and the linear system -------------------------------------------------------------------------------------------------
OFFSETS = np.array([[i, j, k] for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)], dtype=np.int64)


def associate(source, ref_map, max_distance, kernel):
    """nn_index [S] (32 * probe + list position, -1 without a neighbour), distance [S], mask [S], contributions [S, 28]"""
    p = np.asarray(source, dtype=np.float64).reshape(-1, 3)
    S = len(p)
    keys, cnt, pts = ref_map.tables()
    mp = ref_map.max_points
    v, ok = voxels(p, ref_map.voxel_size)
    nv = v[:, None, :] + OFFSETS[None]
    inside = ((nv >= -HALF) & (nv < HALF)).all(axis=2) & ok[:, None]
    pk = pack(np.where(inside[..., None], nv, 0))
    d = np.full((S, 27, mp), np.inf)
    q_all = np.zeros((S, 27, mp, 3))
    if len(keys) and S:
        at = np.minimum(np.searchsorted(keys, pk), len(keys) - 1)
        found = inside & (keys[at] == pk)
        q_all = pts[at]
        valid = found[..., None] & (np.arange(mp)[None, None, :] < cnt[at][..., None])
        d = np.where(valid, np.sqrt(sq(q_all, p[:, None, None, :])), np.inf)
    flat = d.reshape(S, 27 * mp)
    best = flat.argmin(axis=1) if S else np.zeros(0, dtype=np.int64)          # the first of equal distances
    dist = flat[np.arange(S), best] if S else np.zeros(0)
    has = np.isfinite(dist)
    nn_index = np.where(has, (best // mp) * 32 + best % mp, -1).astype(np.int32)
    distance = np.where(has, dist, DBL_MAX)
    mask = has & (distance < max_distance)
    q = q_all.reshape(S, 27 * mp, 3)[np.arange(S), best] if S else np.zeros((0, 3))
    k = np.float64(kernel)
    r = p - q
    r2 = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
    with np.errstate(all="ignore"):
        w = (k * k) / ((k + r2) * (k + r2))
        ux, uy, uz = w * r[:, 0], w * r[:, 1], w * r[:, 2]
        sx, sy, sz = p[:, 0], p[:, 1], p[:, 2]
        zero = np.zeros(S)
        c = np.stack([w, w, w, w * sz, -(w * sy), -(w * sz), w * sx, w * sy, -(w * sx),
                      w * (sy * sy + sz * sz), -(w * (sx * sy)), -(w * (sx * sz)),
                      w * (sx * sx + sz * sz), -(w * (sy * sz)), w * (sx * sx + sy * sy),
                      zero, zero, zero, zero, zero, zero,
                      ux, uy, uz, sy * uz - sz * uy, sz * ux - sx * uz, sx * uy - sy * ux, np.ones(S)], axis=1)
    return nn_index, distance, mask, np.where(mask[:, None], c, 0.0)


def _tree(a):
    """the halving tree over axis -2 (256 rows): a[t] += a[t + o], o = 128, 64, ..., 1"""
    a = a.copy()
    o = BLOCK // 2
    while o:
        a[..., :o, :] += a[..., o:2 * o, :]
        o //= 2
    return a[..., 0, :]


def tree_sums(contributions, rows=None, reverse=False):
    """The 28 sums as the kernels form them for a source buffer of `rows` rows (default: as many as there are contributions)."""
    c = np.asarray(contributions, dtype=np.float64)[:, COLUMNS]
    if reverse:
        c = c[::-1]
    rows = max(len(c) if rows is None else rows, 1)
    nb = -(-rows // BLOCK)
    padded = np.zeros((nb * BLOCK, len(COLUMNS)))
    padded[:len(c)] = c
    part = _tree(padded.reshape(nb, BLOCK, -1))
    acc = np.zeros((BLOCK, len(COLUMNS)))
    for b0 in range(0, nb, BLOCK):
        chunk = part[b0:b0 + BLOCK]
        acc[:len(chunk)] += chunk
    s = np.zeros(28)
    s[COLUMNS] = _tree(acc)
    return s


def system_of(s):
    """(A [6, 6] symmetric, b [6]) of the 28 sums: JTJ and -JTr"""
    A = np.zeros((6, 6))
    A[0, 0], A[1, 1], A[2, 2] = s[0], s[1], s[2]
    A[4, 0], A[5, 0], A[3, 1], A[5, 1], A[3, 2], A[4, 2] = s[3], s[4], s[5], s[6], s[7], s[8]
    A[3, 3], A[4, 3], A[5, 3], A[4, 4], A[5, 4], A[5, 5] = s[9], s[10], s[11], s[12], s[13], s[14]
    A = A + np.tril(A, -1).T
    return A, -s[21:27]


def ldlt_solve(A, b):
    """x of A x = b by LDL^T without pivoting, in the header's order; plain Python floats"""
    A = [[float(v) for v in row] for row in A]
    b = [float(v) for v in b]
    L = [[0.0] * 6 for _ in range(6)]
    d, y, x = [0.0] * 6, [0.0] * 6, [0.0] * 6
    with np.errstate(all="ignore"):
        for j in range(6):
            s = A[j][j]
            for k in range(j):
                s = s - L[j][k] * (L[j][k] * d[k])
            d[j] = s
            for i in range(j + 1, 6):
                t = A[i][j]
                for k in range(j):
                    t = t - L[i][k] * (L[j][k] * d[k])
                L[i][j] = float(np.float64(t) / np.float64(d[j]))
        for i in range(6):
            s = b[i]
            for k in range(i):
                s = s - L[i][k] * y[k]
            y[i] = s
        for i in range(5, -1, -1):
            s = float(np.float64(y[i]) / np.float64(d[i]))
            for k in range(i + 1, 6):
                s = s - L[k][i] * x[k]
            x[i] = s
    return np.array(x)


def se3_exp(dx, use_expm=False):
    """SE3::exp(dx), dx = (upsilon, omega), as a 3 x 4; use_expm: scipy.linalg.expm of the 4 x 4 twist instead of the closed form"""
    u, o = [float(v) for v in dx[:3]], [float(v) for v in dx[3:]]
    W = [[0.0, -o[2], o[1]], [o[2], 0.0, -o[0]], [-o[1], o[0], 0.0]]
    if use_expm:
        from scipy.linalg import expm
        tw = np.zeros((4, 4))
        tw[:3, :3], tw[:3, 3] = W, u
        return expm(tw)[:3]
    t2 = (o[0] * o[0] + o[1] * o[1]) + o[2] * o[2]
    if t2 < 1e-8:
        A, B, C = 1.0 - t2 / 6.0, 0.5 - t2 / 24.0, 1.0 / 6.0 - t2 / 120.0
    else:
        t = math.sqrt(t2)
        sn, cs = math.sin(t), math.cos(t)
        A, B, C = sn / t, (1.0 - cs) / t2, (t - sn) / (t2 * t)
    E = np.zeros((3, 4))
    V = [[0.0] * 3 for _ in range(3)]
    for a in range(3):
        for b in range(3):
            W2 = o[a] * o[b] - (t2 if a == b else 0.0)
            I = 1.0 if a == b else 0.0
            E[a, b] = I + (A * W[a][b] + B * W2)
            V[a][b] = I + (B * W[a][b] + C * W2)
    for a in range(3):
        E[a, 3] = (V[a][0] * u[0] + V[a][1] * u[1]) + V[a][2] * u[2]
    return E


def compose(a, b):
    """a b of two rigid 3 x 4 (or 4 x 4) matrices as a 4 x 4: (a_0 b_0 + a_1 b_1) + a_2 b_2 per entry, + a's translation"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    out = np.eye(4)
    for r in range(3):
        row = (a[r, 0] * b[0, :4] + a[r, 1] * b[1, :4]) + a[r, 2] * b[2, :4]
        row[3] = row[3] + a[r, 3]
        out[r] = row
    return out


def inverse(a):
    """[R^T | -(R^T t)] of a rigid matrix, as a 4 x 4"""
    a = np.asarray(a, dtype=np.float64)
    out = np.eye(4)
    out[:3, :3] = a[:3, :3].T
    for r in range(3):
        out[r, 3] = -((a[0, r] * a[0, 3] + a[1, r] * a[1, 3]) + a[2, r] * a[2, 3])
    return out


def align(source, ref_map, guess, max_distance, kernel, max_num_iterations=500, convergence_criterion=1e-4, rows=None, variant=False):
    """AlignPointsToMap: (pose [4, 4], iterations, status).  variant: the rounding-only variation behind the sensitivity d
    (scipy's expm, a reversed summation order)."""
    guess = np.asarray(guess, dtype=np.float64)
    guess4 = compose(guess, np.eye(4))
    if ref_map.empty():
        return guess4, 0, EMPTY_MAP
    src = apply34(guess, np.asarray(source).astype(np.float64).reshape(-1, 3))
    T, inc = np.eye(4), np.eye(4)
    iterations, status = 0, 0
    while iterations < max_num_iterations and not status:
        src = apply34(inc, src)
        _, _, _, c = associate(src, ref_map, max_distance, kernel)
        s = tree_sums(c, rows, reverse=variant)
        iterations += 1
        if not s[27] > 0.0:
            status = DEGENERATE
            break
        A, b = system_of(s)
        dx = ldlt_solve(A, b)
        n2 = dx[0] * dx[0]
        for a in range(1, 6):
            n2 = n2 + dx[a] * dx[a]
        if not np.isfinite(dx).all():
            status = DEGENERATE
            break
        inc = compose(se3_exp(dx, use_expm=variant), np.eye(4))
        T = compose(inc, T)
        if math.sqrt(n2) < convergence_criterion:
            status = CONVERGED
    return compose(T, guess4), iterations, status


# ---- the odometry ----------------------------------------------------------------------------------------------------------------------
def rotation_angle(R):
    """2 atan2(|vec|, |w|) of the quaternion of a rotation matrix (the branch on the trace, then on the largest diagonal entry)"""
    m = [[float(v) for v in row] for row in np.asarray(R)[:3, :3]]
    t = (m[0][0] + m[1][1]) + m[2][2]
    if t > 0.0:
        t = math.sqrt(t + 1.0)
        w, t = 0.5 * t, 0.5 / t
        vec = [(m[2][1] - m[1][2]) * t, (m[0][2] - m[2][0]) * t, (m[1][0] - m[0][1]) * t]
    else:
        i = 0
        if m[1][1] > m[0][0]:
            i = 1
        if m[2][2] > m[i][i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = math.sqrt(((m[i][i] - m[j][j]) - m[k][k]) + 1.0)
        vec = [0.0, 0.0, 0.0]
        vec[i], t = 0.5 * t, 0.5 / t
        w = (m[k][j] - m[j][k]) * t
        vec[j], vec[k] = (m[j][i] + m[i][j]) * t, (m[k][i] + m[i][k]) * t
    return 2.0 * math.atan2(math.sqrt((vec[0] * vec[0] + vec[1] * vec[1]) + vec[2] * vec[2]), abs(w))


class Config:
    def __init__(self, max_range, min_range=5.0, voxel_size=None, max_points_per_voxel=20, max_num_iterations=500,
                 convergence_criterion=1e-4, initial_threshold=2.0, min_motion_th=0.1):
        self.max_range, self.min_range = float(max_range), float(min_range)
        self.voxel_size = float(max_range / 100.0 if voxel_size is None else voxel_size)
        self.max_points_per_voxel, self.max_num_iterations = int(max_points_per_voxel), int(max_num_iterations)
        self.convergence_criterion, self.initial_threshold, self.min_motion_th = float(convergence_criterion), float(initial_threshold), float(min_motion_th)


class RefOdometry:
    """MTGS's KissICP.register_frame (deskew off): the warm-up of two frames per traversal from the log pose with sigma = 2, the
    constant-velocity guess otherwise, the adaptive threshold, the map update through the new pose."""

    def __init__(self, config, capacity=1 << 20, variant=False):
        self.c, self.variant = config, variant
        self.last_pose, self.last_delta = np.eye(4), np.eye(4)
        self.last_traj_id, self.warmup = -1, -1
        self.model_sse, self.num_samples = config.initial_threshold * config.initial_threshold, 1
        self.map = RefMap(config.voxel_size, config.max_points_per_voxel, capacity)
        self.iterations = []

    def register_frame(self, points, log_pose, traj_id):
        c = self.c
        frame, source, _, _, _ = downsample(points, c.min_range, c.max_range, c.voxel_size)
        sigma = math.sqrt(self.model_sse / self.num_samples)
        log_pose = compose(log_pose, np.eye(4))
        if self.last_traj_id != traj_id:
            self.warmup = 1
            self.last_pose = log_pose
        if self.warmup >= 0:
            self.warmup -= 1
            guess, sigma = log_pose, 2.0
        else:
            guess = compose(self.last_pose, self.last_delta)
        pose, it, _ = align(source, self.map, guess, 3.0 * sigma, sigma / 3.0, c.max_num_iterations, c.convergence_criterion,
                            rows=len(np.asarray(points)), variant=self.variant)
        dev = compose(inverse(guess), pose)
        t = dev[:3, 3]
        error = math.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]) + 2.0 * c.max_range * math.sin(rotation_angle(dev) / 2.0)
        if error > c.min_motion_th:
            self.model_sse += error * error
            self.num_samples += 1
        self.map.insert(frame, pose)
        self.map.prune(pose[:3, 3], 2.0 * c.max_range)
        self.last_delta = compose(inverse(self.last_pose), pose)
        self.last_pose, self.last_traj_id = pose, traj_id
        self.iterations.append(it)
        return pose


def register_traversals(scans, log_poses, traj_ids, config, variant=False):
    """([F, 4, 4] poses in the log poses' frame, [F] iteration counts): the poses are registered relative to the first pose's
    translation (datasets/mtgs.py:64-66) and moved back afterwards (apply_calibration)."""
    log_poses = np.asarray(log_poses, dtype=np.float64).copy()
    first = log_poses[0, :3, 3].copy()
    log_poses[:, :3, 3] = log_poses[:, :3, 3] - first[None]
    odo = RefOdometry(config, variant=variant)
    poses = np.stack([odo.register_frame(s, p, t) for s, p, t in zip(scans, log_poses, traj_ids)])
    poses[:, :3, 3] = poses[:, :3, 3] + first[None]
    return poses, np.array(odo.iterations, dtype=np.int64)


# ---- the test scene ----------------------------------------------------------------------------------------------------------------------
def yaw_pose(x, y, z, yaw):
    c, s = math.cos(yaw), math.sin(yaw)
    return np.array([[c, -s, 0.0, x], [s, c, 0.0, y], [0.0, 0.0, 1.0, z], [0.0, 0.0, 0.0, 1.0]])


def scene_boxes(rng):
    """[B, 2, 3] axis-aligned boxes: a ground slab, three walls and ten objects"""
    boxes = [[(-80.0, -80.0, -0.5), (110.0, 60.0, 0.0)],
             [(-60.0, 25.0, 0.0), (71.0, 26.0, 30.0)], [(70.0, -27.0, 0.0), (71.0, 25.0, 30.0)], [(-60.0, -27.0, 0.0), (71.0, -26.0, 30.0)]]
    for _ in range(10):
        cx, cy = rng.uniform(-25.0, 55.0), rng.uniform(5.0, 18.0) * rng.choice([-1.0, 1.0])
        sx, sy, sz = rng.uniform(2.0, 7.0), rng.uniform(2.0, 6.0), rng.uniform(2.0, 6.0)
        boxes.append([(cx - sx / 2, cy - sy / 2, 0.0), (cx + sx / 2, cy + sy / 2, sz)])
    return np.asarray(boxes, dtype=np.float64)


def cast_sweep(boxes, pose, rng, noise=0.01, jitter=1.5):
    """One sweep of 24 elevations x 120 azimuths from `pose` (sensor to world): float32 points in the sensor frame.  Every ray is
    turned by up to `jitter` degrees in azimuth and a third of that in elevation: with an exact pattern this sparse, point-to-point
    ICP locks the pattern of one sweep onto the pattern of the last and reports no motion."""
    el = np.deg2rad(np.linspace(-12.0, 12.0, 24))
    az = np.deg2rad(np.arange(120) * 3.0 + 0.7)
    e, a = np.meshgrid(el, az, indexing="ij")
    a = a + np.deg2rad(rng.uniform(-jitter, jitter, a.shape))
    e = e + np.deg2rad(rng.uniform(-jitter, jitter, e.shape) / 3.0)
    d = np.stack([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)], axis=-1).reshape(-1, 3)
    dw = d @ pose[:3, :3].T
    o = pose[:3, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        t0 = (boxes[None, :, 0, :] - o) / dw[:, None, :]
        t1 = (boxes[None, :, 1, :] - o) / dw[:, None, :]
    near, far = np.minimum(t0, t1).max(axis=2), np.maximum(t0, t1).min(axis=2)
    t = np.where((near <= far) & (far > 0.0), np.where(near > 0.0, near, far), np.inf).min(axis=1)
    hit = np.isfinite(t) & (t < 150.0)
    r = t[hit] + rng.normal(0.0, noise, int(hit.sum()))
    return (d[hit] * r[:, None]).astype(np.float32)


def make_scene(seed=5, traversals=2, frames=5):
    """(scans, true poses [F, 4, 4], log poses [F, 4, 4], traj ids): sensor 1.9 m above the ground, 2.5 m per frame; the second
    traversal drives the next lane with a small heading offset.  The log poses are the true ones, perturbed by about 0.25 m and 1
    degree from the second frame of the scene on."""
    rng = np.random.default_rng(seed)
    boxes = scene_boxes(rng)
    origin = np.array([664000.0, 3997000.0, 600.0])        # a city-scale offset: register_traversals works relative to the first pose
    scans, true, log, ids = [], [], [], []
    for tr in range(traversals):
        for f in range(frames):
            pose = yaw_pose(2.5 * f + 1.3 * tr, -1.75 + 3.5 * tr, 1.9, 0.02 * f + 0.05 * tr)
            scans.append(cast_sweep(boxes, pose, rng))
            noisy = pose.copy()
            if true:
                dyaw = np.deg2rad(rng.normal(0.0, 1.0))
                noisy = pose @ yaw_pose(0.0, 0.0, 0.0, dyaw)
                noisy[:3, 3] = pose[:3, 3] + rng.normal(0.0, 0.25 / math.sqrt(3.0) * 1.4, 3)
            for m in (pose, noisy):
                m[:3, 3] += origin
            true.append(pose)
            log.append(noisy)
            ids.append(tr)
    return scans, np.stack(true), np.stack(log), np.array(ids, dtype=np.int64)


SCENE_CONFIG = dict(max_range=80.0, voxel_size=0.8)


def golden():
    with np.load(GOLDEN) as z:
        g = {k: z[k] for k in z.files}
    g["scans"] = [g["points"][a:b] for a, b in zip(g["offsets"][:-1], g["offsets"][1:])]
    return g


def write_golden(seed=5):
    scans, true, log, ids = make_scene(seed)
    config = Config(**SCENE_CONFIG)
    poses, its = register_traversals(scans, log, ids, config)
    poses2, its2 = register_traversals(scans, log, ids, config, variant=True)
    assert np.array_equal(its, its2), (its, its2)
    d = float(np.abs(poses - poses2).max())
    err = lambda p: float(np.linalg.norm(p[:, :3, 3] - true[:, :3, 3], axis=1).mean())
    print(f"seed {seed}: points per sweep {[len(s) for s in scans]}, iterations {its.tolist()}, d = {d:.3g}, "
          f"mean translation error: log {err(log):.3f} m, registered {err(poses):.3f} m")
    offsets = np.cumsum([0] + [len(s) for s in scans]).astype(np.int64)
    np.savez_compressed(GOLDEN, points=np.concatenate(scans), offsets=offsets, true_poses=true, log_poses=log, traj_ids=ids, poses=poses,
                        iterations=its, d=np.float64(d))
    return poses, its, d


if __name__ == "__main__":
    write_golden()
