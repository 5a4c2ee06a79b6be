"""Lidar registration (mtgs_amd/registration.py, csrc/icp.hip, include/mtgs_icp.h) without a GPU: the NumPy restatement of
tests/icp_refs.py against independent formulations of each of its parts, the recorded fixture tests/golden/icp_ref.npz, the header
group and the host-side argument checks.  kiss-icp itself cannot be built here (Eigen, Sophus, TBB, tsl::robin_map): nothing is
compared with its binary."""
import ctypes as C
import math
from pathlib import Path

import numpy as np
import pytest

from tests import icp_refs as R

ROOT = Path(__file__).resolve().parents[1]
NAMES = ["mtgs_icp_align_begin", "mtgs_icp_align_iterate", "mtgs_icp_align_workspace_bytes", "mtgs_icp_associate", "mtgs_icp_downsample",
         "mtgs_icp_downsample_workspace_bytes", "mtgs_icp_map_bytes", "mtgs_icp_map_export", "mtgs_icp_map_export_workspace_bytes",
         "mtgs_icp_map_init", "mtgs_icp_map_insert", "mtgs_icp_map_insert_workspace_bytes", "mtgs_icp_map_prune"]


@pytest.fixture(scope="module")
def gold():
    return R.golden()


@pytest.fixture(scope="module")
def cloud():
    """3000 points in a 40 m cube, a quarter of them snapped to a 0.25 m lattice (voxel faces, duplicates)"""
    rng = np.random.default_rng(11)
    p = rng.uniform(-20.0, 20.0, (3000, 3))
    p[::4] = np.round(p[::4] * 4.0) / 4.0
    p[5] = p[4]
    return p


def test_level_one_downsample_is_first_per_voxel(cloud):
    """against np.unique over the voxel rows with return_index: the first occurrence of every voxel, in ascending index"""
    frame, source, fi, si, status = R.downsample(cloud, 5.0, 30.0, 1.0)
    norm = np.linalg.norm(cloud, axis=1)
    kept = np.flatnonzero((norm > 5.0) & (norm < 30.0))
    _, first = np.unique(np.floor(cloud[kept] / 0.5), axis=0, return_index=True)
    assert np.array_equal(fi, kept[np.sort(first)]) and np.array_equal(frame, cloud[fi]) and status == 0
    _, first2 = np.unique(np.floor(frame / 1.5), axis=0, return_index=True)
    assert np.array_equal(si, fi[np.sort(first2)]) and np.array_equal(source, cloud[si])
    assert 0 < len(si) < len(fi) < len(kept)


def test_map_insert_equals_a_direct_sequential_loop(cloud):
    """the points one by one in offered order, as VoxelHashMap::AddPoints walks them"""
    size, maxp = 4.0, 3
    m = R.RefMap(size, maxp)
    m.insert(cloud[:2000])
    m.insert(cloud[2000:], R.yaw_pose(0.3, -0.2, 0.1, 0.05))
    direct = {}
    resolution = math.sqrt(size * size / maxp)
    second = R.apply34(R.yaw_pose(0.3, -0.2, 0.1, 0.05), cloud[2000:])
    for p in np.concatenate([cloud[:2000], second]):
        held = direct.setdefault(tuple(np.floor(p / size).astype(int)), [])
        if len(held) == maxp or any(np.linalg.norm(q - p) < resolution for q in held):
            continue
        held.append(p)
    assert len(direct) == len(m.lists) and max(len(v) for v in direct.values()) == maxp
    for voxel, held in direct.items():
        assert np.array_equal(np.asarray(held), np.asarray(m.lists[int(R.pack(np.asarray(voxel)))])), voxel
    cloud_out = m.point_cloud()
    assert len(cloud_out) == sum(len(v) for v in direct.values())
    order = sorted(direct, key=lambda v: int(R.pack(np.asarray(v))))
    assert np.array_equal(cloud_out, np.concatenate([np.asarray(direct[v]) for v in order]))


def test_prune_empties_by_the_first_point_and_keeps_the_entry():
    m = R.RefMap(1.0, 4)
    m.insert(np.array([[0.5, 0.5, 0.5], [0.9, 0.9, 0.9], [3.5, 0.5, 0.5], [5.0, 0.0, 0.0]]))
    m.prune([0.5, 0.5, 0.5], 3.0)                       # |(3.5, .5, .5) - origin| = 3 exactly: removed; (0.9, ...) stays with its voxel
    assert np.array_equal(m.point_cloud(), np.array([[0.5, 0.5, 0.5], [0.9, 0.9, 0.9]])) and len(m.lists) == 3 and not m.empty()
    m.insert(np.array([[3.6, 0.5, 0.5]]))
    assert np.array_equal(m.point_cloud()[-1], [3.6, 0.5, 0.5])
    m.prune([100.0, 0.0, 0.0], 1.0)
    assert m.empty() and len(m.point_cloud()) == 0


def test_neighbour_search_agrees_with_a_kd_tree(cloud):
    """on every query whose global nearest neighbour is closer than voxel_size the 27 voxels must hold it"""
    from scipy.spatial import cKDTree
    size = 2.0
    m = R.RefMap(size, 20)
    m.insert(cloud[:2500])
    held = m.point_cloud()
    rng = np.random.default_rng(3)
    query = np.concatenate([cloud[2500:], held[:50] + rng.normal(0.0, 0.2, (50, 3))])
    nn, dist, mask, _ = R.associate(query, m, 1.0, 0.5)
    d_tree, i_tree = cKDTree(held).query(query)
    near = d_tree < size
    assert near.sum() > 300
    exact = np.sqrt(R.sq(held[i_tree], query))
    assert np.array_equal(dist[near], exact[near]) and (nn[near] >= 0).all()
    assert np.array_equal(mask, (nn >= 0) & (dist < 1.0)) and mask.any() and not mask.all()
    keys, cnt, pts = m.tables()
    v, _ = R.voxels(query, size)
    for i in np.flatnonzero(near)[:100]:                    # the index names that point
        at = np.searchsorted(keys, R.pack(v[i] + R.OFFSETS[nn[i] // 32]))
        assert np.array_equal(pts[at, nn[i] % 32], held[i_tree[i]]) or exact[i] == np.sqrt(R.sq(pts[at, nn[i] % 32], query[i]))


def test_exponential_against_expm():
    rng = np.random.default_rng(0)
    for scale in (1e-9, 1e-5, 9e-5, 1.1e-4, 1e-2, 0.3, 2.5):
        dx = rng.normal(0.0, 1.0, 6) * scale
        E, ref = R.se3_exp(dx), R.se3_exp(dx, use_expm=True)
        assert np.abs(E - ref).max() <= 8 * np.finfo(np.float64).eps * max(1.0, np.abs(ref).max()), scale
        assert np.abs(E[:, :3] @ E[:, :3].T - np.eye(3)).max() < 1e-14


def test_solver_against_numpy():
    rng = np.random.default_rng(1)
    for _ in range(20):
        G = rng.normal(0.0, 1.0, (40, 6))
        A, b = G.T @ G, rng.normal(0.0, 1.0, 6)
        x = R.ldlt_solve(A, b)
        ref = np.linalg.solve(A, b)
        assert np.abs(x - ref).max() <= 1e-10 * np.linalg.cond(A) * max(1.0, np.abs(ref).max()) * 1e-3


def test_sums_tree_and_system(cloud):
    m = R.RefMap(2.0, 20)
    m.insert(cloud[:2500])
    _, _, mask, c = R.associate(cloud[1500:] + 0.05, m, 1.5, 0.4)
    s = R.tree_sums(c)
    assert s[27] == mask.sum() > 256 and np.allclose(s, c.sum(axis=0), rtol=1e-12, atol=1e-9) and not s[15:21].any()
    assert np.array_equal(s, R.tree_sums(c, rows=len(c) + 700))         # blocks of zeros change no bit
    A, b = R.system_of(s)
    p = cloud[1500:][mask] + 0.05
    J = np.zeros((len(p), 3, 6))
    J[:, :, :3] = np.eye(3)
    J[:, 0, 4], J[:, 0, 5], J[:, 1, 3], J[:, 1, 5], J[:, 2, 3], J[:, 2, 4] = p[:, 2], -p[:, 1], -p[:, 2], p[:, 0], p[:, 1], -p[:, 0]
    w = c[mask][:, 0]
    assert np.allclose(A, np.einsum("nij,n,nik->jk", J, w, J), rtol=1e-10, atol=1e-8) and np.array_equal(A, A.T)
    r = c[mask][:, 21:24] / w[:, None]
    assert np.allclose(b, -np.einsum("nij,n,ni->j", J, w, r), rtol=1e-10, atol=1e-8)


def test_rotation_angle():
    for yaw in (0.0, 1e-4, 0.3, 3.0, -2.0):
        assert abs(R.rotation_angle(R.yaw_pose(0, 0, 0, yaw)) - abs(yaw)) < 1e-7
    flip = np.diag([-1.0, -1.0, 1.0])                       # trace < 0: the other branch
    assert abs(R.rotation_angle(flip) - math.pi) < 1e-12


def test_fixture_registration_registers(gold):
    """2 traversals x 5 frames, voxel_size 0.8: the registered poses halve the log poses' mean translational error, with margin"""
    err = lambda p: float(np.linalg.norm(p[:, :3, 3] - gold["true_poses"][:, :3, 3], axis=1).mean())
    log, reg = err(gold["log_poses"]), err(gold["poses"])
    print(f"mean translational error: log poses {log:.3f} m, registered {reg:.3f} m; iterations {gold['iterations'].tolist()}")
    assert len(gold["scans"]) == 10 and gold["traj_ids"].tolist() == [0] * 5 + [1] * 5
    assert all(2600 < len(s) < 2900 and s.dtype == np.float32 for s in gold["scans"])
    assert 0.2 < log < 0.45 and reg <= 0.5 * log and reg < 0.1
    assert np.array_equal(gold["log_poses"][0], gold["true_poses"][0]) and gold["iterations"][0] == 0 and (gold["iterations"][1:] > 0).all()
    assert (ROOT / "tests" / "golden" / "icp_ref.npz").stat().st_size < 400_000


@pytest.fixture(scope="module")
def rerun(gold):
    config = R.Config(**R.SCENE_CONFIG)
    return (R.register_traversals(gold["scans"], gold["log_poses"], gold["traj_ids"], config),
            R.register_traversals(gold["scans"], gold["log_poses"], gold["traj_ids"], config, variant=True))


def test_odometry_reproduces_the_fixture(gold, rerun):
    """the restatement run again: the same iteration counts; poses within 64 d (sin / cos of another libm may differ in the last place)"""
    (poses, its), _ = rerun
    assert np.array_equal(its, gold["iterations"])
    assert np.abs(poses - gold["poses"]).max() <= 64 * float(gold["d"])


def test_sensitivity_d(gold, rerun):
    """d: the largest difference of any pose entry between the restatement and its rounding-only variant (scipy's expm for the closed
    form, the contributions summed in reversed order).  The iteration counts do not move."""
    _, (poses, its) = rerun
    d = float(np.abs(poses - gold["poses"]).max())
    print(f"d measured {d:.3g}, recorded {float(gold['d']):.3g}")
    assert np.array_equal(its, gold["iterations"])
    assert 0.0 < float(gold["d"]) < 1e-12 and 0.0 < d <= 64 * float(gold["d"])


def test_scene_is_the_recorded_one(gold):
    scans, true, log, ids = R.make_scene()
    assert np.array_equal(true, gold["true_poses"]) and np.array_equal(log, gold["log_poses"]) and np.array_equal(ids, gold["traj_ids"])
    assert all(np.array_equal(a, b) for a, b in zip(scans, gold["scans"]))


def test_align_poses_recovers_a_planar_motion():
    from mtgs_amd.registration import align_poses, registration_errors
    rng = np.random.default_rng(2)
    F = 12
    orig = np.stack([R.yaw_pose(3.0 * f, 0.4 * f * f, 1.0, 0.05 * f) for f in range(F)])
    T = R.yaw_pose(4.0, -3.0, 0.0, 0.2)
    moved = np.linalg.inv(T)[None] @ orig
    aligned = align_poses(orig, moved)
    # the quirk: the translation applied is the difference of the mean positions, exact only together with the rotation about the
    # registered centroid -- so the fit is exact in rotation and within that residual in position
    assert np.allclose(aligned[:, :2, :2], orig[:, :2, :2], atol=1e-12)
    c = moved[:, :2, 3].mean(axis=0)
    Rz = T[:2, :2]
    expect = (moved[:, :2, 3] @ Rz.T) + (orig[:, :2, 3].mean(axis=0) - c)
    assert np.allclose(aligned[:, :2, 3], expect, atol=1e-12)
    pure_shift = orig.copy()
    pure_shift[:, :2, 3] += [2.0, -1.0]
    assert np.allclose(align_poses(orig, pure_shift), orig, atol=1e-12)
    noisy = orig.copy()
    noisy[:, :2, 3] += rng.normal(0.0, 0.01, (F, 2))
    noisy[6:, 0, 3] += 2.0
    e = registration_errors(orig, noisy, [0] * 6 + [1] * 6)
    assert list(e) == [0, 1] and not e[0]["bad"] and e[1]["bad"] and e[1]["max_end_point_error"] > 1.0 and e[0]["mean_error"] < 0.05
    assert e[0]["mean_heading_error"] < 1e-9


def test_config_defaults():
    from mtgs_amd.registration import KissConfig
    c = KissConfig(max_range=200.0)
    assert (c.min_range, c.voxel_size, c.max_points_per_voxel, c.max_num_iterations, c.convergence_criterion, c.initial_threshold,
            c.min_motion_th, c.max_distance) == (5.0, 2.0, 20, 500, 1e-4, 2.0, 0.1, 400.0)
    with pytest.raises(ValueError, match="max_points_per_voxel"):
        KissConfig(max_range=100.0, max_points_per_voxel=33)
    with pytest.raises(ValueError, match="max_range"):
        KissConfig(max_range=4.0)


def test_header_group_and_build_flags(hip_lib):
    """mtgs_icp.h is one of the header groups (declared, bound, exported: tests/test_abi.py) and icp.hip rounds every operation"""
    import mtgs_amd
    from mtgs_amd import _abi, _lib, build, registration
    assert sorted(_lib.GROUPS["mtgs_icp.h"]) == NAMES and "mtgs_icp.h" in _abi.included_headers()
    assert build.PER_FILE_FLAGS["icp.hip"] == ["-ffp-contract=off"]
    k = _abi.header_abi("mtgs_icp.h").constants
    assert (k["MTGS_ICP_MAX_POINTS"], k["MTGS_ICP_BLOCK"], k["MTGS_ICP_RECORD"], k["MTGS_ICP_SUMS"]) == (32, R.BLOCK, 64, 28)
    assert (registration.CONVERGED, registration.DEGENERATE, registration.EMPTY_MAP) == (R.CONVERGED, R.DEGENERATE, R.EMPTY_MAP)
    assert {"KissConfig", "VoxelMap", "LidarOdometry", "register_traversals", "align_points_to_map", "align_poses",
            "registration_errors"} <= set(mtgs_amd.__all__)


def test_host_side_argument_validation(hip_lib):
    """every call below fails a check on the host: nothing is launched"""
    n = C.c_size_t(0)
    assert hip_lib.mtgs_icp_downsample_workspace_bytes(-1, C.byref(n)) == 1 and b"mtgs_icp_downsample_workspace_bytes" in hip_lib.mtgs_rast_last_error()
    assert hip_lib.mtgs_icp_downsample_workspace_bytes(35000, C.byref(n)) == 0 and n.value > 35000 * 40
    assert hip_lib.mtgs_icp_map_bytes(1000, 33, C.byref(n)) == 1 and b"max_points" in hip_lib.mtgs_rast_last_error()
    assert hip_lib.mtgs_icp_map_bytes(0, 20, C.byref(n)) == 1 and b"capacity" in hip_lib.mtgs_rast_last_error()
    assert hip_lib.mtgs_icp_map_bytes(1000, 20, C.byref(n)) == 0 and n.value >= 1000 * (20 * 24 + 28)
    assert hip_lib.mtgs_icp_downsample(5, None, 0, 3, 5.0, 100.0, 1.0, None, None, None, None, None, None, None, 0, None) == 1
    assert b"points" in hip_lib.mtgs_rast_last_error()
    assert hip_lib.mtgs_icp_map_insert(None, 10, 20, 1.0, 0, None, 1, 3, None, None, None, 0, None) == 1 and b"map" in hip_lib.mtgs_rast_last_error()
    assert hip_lib.mtgs_icp_align_iterate(None, 10, 20, 1.0, 5, None, 1.0, 1.0, 1e-4, 8, None, None, 0, None) == 1
    assert hip_lib.mtgs_icp_map_prune(None, 10, 20, None, 1.0, None) == 1


def test_python_layer_refuses_bad_inputs_before_the_device():
    import torch
    from mtgs_amd import registration as G
    c = G.KissConfig(max_range=100.0)
    with pytest.raises(ValueError, match=r"points must be \[N, 3\]"):
        G.downsample(torch.zeros(4, 4), c)
    with pytest.raises(TypeError, match="float32 or float64"):
        G.downsample(torch.zeros(4, 3, dtype=torch.int32), c)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        G.downsample(torch.zeros(4, 3), c)
    with pytest.raises(ValueError, match="capacity"):
        G.VoxelMap(1.0, 20, capacity=0)
    with pytest.raises(TypeError, match="VoxelMap"):
        G.align_points_to_map(torch.zeros(4, 3), None, np.eye(4), 1.0, 1.0)
