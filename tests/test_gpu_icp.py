"""mtgs_amd.registration on the device (csrc/icp.hip): the down-sampling, the map, one association and its sums are compared BIT FOR BIT
with the NumPy restatement tests/icp_refs.py (up to the sign of a zero); a whole alignment and the recorded traversals within bounds
that come from the number format and from the fixture's own sensitivity d, never from the code under test.  kiss-icp itself cannot be
built here: nothing is compared with its binary."""
import numpy as np
import pytest
import torch

from tests import icp_refs as R

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps


def bits(a):
    """the bit patterns of float64 values, -0.0 folded onto 0.0"""
    return (np.ascontiguousarray(a, dtype=np.float64) + 0.0).view(np.int64)


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


@pytest.fixture(scope="module")
def G(hip_lib):
    from mtgs_amd import registration
    return registration


@pytest.fixture(scope="module")
def gold():
    return R.golden()


# ---- down-sampling -----------------------------------------------------------------------------------------------------------------------
def ds_cloud(N, seed=0):
    """N points in a 60 m cube: a third on the 0.5 m lattice (exactly on voxel faces of both levels at voxel_size 1), close pairs,
    negative coordinates, -0.0, a duplicate"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-30.0, 30.0, (N, 3))
    p[::3] = np.round(p[::3] * 2.0) / 2.0
    p[1::2] = p[0:N - 1:2] + rng.uniform(-0.4, 0.4, (N // 2, 3))          # pairs that mostly share a coarse voxel
    if N > 8:
        p[3] = [-0.0, 6.0, -0.0]
        p[7] = p[2]
    return p


def check_downsample(G, points, config, p64=None):
    p64 = np.asarray(points, dtype=np.float64) if p64 is None else p64
    frame, source, fi, si, status = R.downsample(p64, config.min_range, config.max_range, config.voxel_size)
    out = G.downsample(points if isinstance(points, torch.Tensor) else dev(points), config)
    n1, n2 = out.counts.cpu().tolist()
    assert (n1, n2) == (len(fi), len(si)) and int(out.status.item()) == status
    assert np.array_equal(out.frame_index[:n1].cpu().numpy(), fi) and np.array_equal(out.source_index[:n2].cpu().numpy(), si)
    assert np.array_equal(bits(out.frame[:n1].cpu().numpy()), bits(frame)) and np.array_equal(bits(out.source[:n2].cpu().numpy()), bits(source))
    return n1, n2


@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 255, 256, 257, 1025, 2049])
def test_downsample_sizes(G, N):
    """one above the sort's 1024-row and the scan's 2048-row tiles among them"""
    n1, n2 = check_downsample(G, ds_cloud(N, N), G.KissConfig(max_range=40.0, min_range=5.0, voxel_size=1.0))
    assert n2 <= n1 <= N and (N < 60 or 0 < n2 < n1)


def test_downsample_one_voxel_and_own_voxels(G):
    c = G.KissConfig(max_range=100.0, min_range=1.0, voxel_size=1.0)
    rng = np.random.default_rng(1)
    assert check_downsample(G, 10.0 + rng.uniform(0.0, 0.5, (300, 3)) * [1.0, 1.0, 0.999], c) == (1, 1)
    g = np.stack(np.meshgrid(*[np.arange(-3, 4) * 2.0] * 3, indexing="ij"), axis=-1).reshape(-1, 3) + 0.25
    own = g[np.linalg.norm(g, axis=1) > 1.0]
    assert check_downsample(G, own, c) == (len(own), len(own))


def test_downsample_range_limits_are_excluded(G):
    c = G.KissConfig(max_range=10.0, min_range=5.0, voxel_size=1.0)
    p = np.array([[3.0, 4.0, 0.0], [0.0, 0.0, -5.0], [6.0, 8.0, 0.0], [0.0, -10.0, 0.0], [3.0, 4.0, 1e-3], [6.0, 8.0 - 1e-3, 0.0],
                  [np.nextafter(5.0, 6.0), 0.0, 0.0], [np.nextafter(10.0, 0.0), 0.0, 0.0], [20.0, 0.0, 0.0], [1.0, 1.0, 1.0]])
    check_downsample(G, p, c)
    out = G.downsample(dev(p), c)
    assert out.frame_index[:int(out.counts[0])].cpu().tolist() == [4, 5, 6, 7]


def test_downsample_float32_and_strided(G):
    c = G.KissConfig(max_range=40.0, min_range=5.0, voxel_size=1.0)
    p = ds_cloud(700, 9).astype(np.float32)
    check_downsample(G, dev(p), c, p.astype(np.float64))
    wide = torch.zeros((700, 5), dtype=torch.float32, device="cuda")
    wide[:, 1:4] = dev(p)
    check_downsample(G, wide[:, 1:4], c, p.astype(np.float64))
    wide64 = torch.full((700, 4), 7.0, dtype=torch.float64, device="cuda")
    wide64[:, :3] = dev(p.astype(np.float64))
    check_downsample(G, wide64[:, :3], c, p.astype(np.float64))


def test_downsample_grid_guard(G):
    """level one's voxels are 0.5 wide: 2^19 is voxel 2^20, outside; -2^19 is voxel -2^20, inside"""
    c = G.KissConfig(max_range=1e7, min_range=1.0, voxel_size=1.0)
    p = np.array([[10.0, 0.0, 0.0], [524288.0, 0.0, 0.0], [-524288.0, 0.0, 0.0], [524287.75, 3.0, 0.0], [0.0, np.nan, 20.0], [0.0, 0.0, 9e6]])
    check_downsample(G, p, c)
    out = G.downsample(dev(p), c)
    assert int(out.status.item()) == G.OUT_OF_GRID and out.frame_index[:int(out.counts[0])].cpu().tolist() == [0, 2, 3]
    with pytest.raises(ValueError, match="outside the voxel grid"):
        out.trimmed()
    assert int(G.downsample(dev(p[[0, 2, 3]]), c).status.item()) == 0


# ---- the map -----------------------------------------------------------------------------------------------------------------------------
def both_maps(G, voxel_size, maxp, capacity=64):
    return G.VoxelMap(voxel_size, maxp, capacity), R.RefMap(voxel_size, maxp, capacity)


def same_map(m, ref, strict=True):
    got, want = m.point_cloud(strict).cpu().numpy(), ref.point_cloud()
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want))
    voxels, status, live = m.status()
    assert voxels == len(ref.lists) and live == sum(1 for v in ref.lists.values() if v) and status == ref.status
    assert m.empty() == ref.empty() if strict else True
    return got


def test_map_twentieth_point_accepted_twenty_first_refused(G):
    m, ref = both_maps(G, 1.0, 20)
    lattice = np.stack(np.meshgrid(*[0.05 + 0.3 * np.arange(3)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)      # 27 points 0.3 apart > 0.2236
    for mm in (m, ref):
        mm.insert(dev(lattice[:19]) if mm is m else lattice[:19])
    assert len(same_map(m, ref)) == 19
    for mm in (m, ref):
        mm.insert(dev(lattice[19:]) if mm is m else lattice[19:])
    got = same_map(m, ref)
    assert len(got) == 20 and np.array_equal(got, lattice[:20])


def test_map_resolution_boundary_and_duplicates(G):
    """max_points 4 at voxel_size 1: map_resolution = sqrt(1 / 4) = 0.5 exactly"""
    m, ref = both_maps(G, 1.0, 4)
    below = np.nextafter(0.5, 0.0)
    p = np.array([[0.0, 0.25, 0.25], [below, 0.25, 0.25], [0.5, 0.25, 0.25], [0.0, 0.25, 0.25], [0.5, 0.25, 0.25],
                  [3.0, 0.25, 0.25], [3.0, 0.25 + below, 0.25], [3.0, 0.75, 0.25]])
    m.insert(dev(p)), ref.insert(p)
    got = same_map(m, ref)
    assert np.array_equal(got, p[[0, 2, 5, 7]])
    q = np.array([[0.25, 0.25, 0.875], [3.0, 0.5, 0.75], [-0.0, -0.0, -0.0], [-1e-9, 0.0, 0.0]])      # a second insert into the same voxels
    m.insert(dev(q)), ref.insert(q)
    assert len(same_map(m, ref)) == 7


def test_map_insert_through_a_pose_float32_strided_and_counted(G):
    m, ref = both_maps(G, 2.0, 5, 4096)
    rng = np.random.default_rng(4)
    p = rng.uniform(-12.0, 12.0, (1500, 3)).astype(np.float32)
    pose = R.yaw_pose(1.5, -0.7, 0.2, 0.3)
    wide = torch.zeros((1500, 4), dtype=torch.float32, device="cuda")
    wide[:, :3] = dev(p)
    m.insert(wide[:, :3], pose), ref.insert(p.astype(np.float64), pose)
    same_map(m, ref)
    more = rng.uniform(-14.0, 14.0, (1300, 3))
    count = torch.tensor([1025], dtype=torch.int64, device="cuda")
    m.insert(dev(more), torch.from_numpy(pose[:3].reshape(12)).cuda(), count), ref.insert(more[:1025], pose)
    got = same_map(m, ref)
    assert len(got) > 1500 and max(len(v) for v in ref.lists.values()) >= 3


def test_map_prune_boundary_and_reinsertion(G):
    m, ref = both_maps(G, 1.0, 4)
    p = np.array([[3.0, 4.0, 0.0], [3.5, 4.5, 0.5], [0.5, 0.5, 0.5], [-3.0, -4.0, 0.0], [0.0, 0.0, 12.5]])
    m.insert(dev(p)), ref.insert(p)
    inside = float(np.nextafter(5.0, 6.0))
    m.prune([0.0, 0.0, 0.0], inside), ref.prune([0.0, 0.0, 0.0], inside)           # 25 < inside^2: (3, 4, 0) and (-3, -4, 0) stay
    assert len(same_map(m, ref)) == 4
    m.prune(torch.zeros(3, dtype=torch.float64, device="cuda"), 5.0), ref.prune([0.0, 0.0, 0.0], 5.0)      # 25 >= 25: both voxels emptied
    got = same_map(m, ref)
    assert np.array_equal(got, p[[2]]) and m.status()[0] == 4
    back = np.array([[3.25, 4.25, 0.25], [3.75, 4.75, 0.75]])
    m.insert(dev(back)), ref.insert(back)                                      # the emptied voxel fills again from empty
    assert np.array_equal(same_map(m, ref), np.concatenate([p[[2]], back]))
    m.prune([50.0, 0.0, 0.0], 1.0), ref.prune([50.0, 0.0, 0.0], 1.0)
    assert len(same_map(m, ref)) == 0 and m.empty()


def test_map_capacity_guard(G):
    m, ref = both_maps(G, 1.0, 4, capacity=4)
    p = np.array([[0.5, 0.5, 0.5], [2.5, 0.5, 0.5], [4.5, 0.5, 0.5]])
    m.insert(dev(p)), ref.insert(p)
    before = same_map(m, ref)
    q = np.array([[0.25, 0.75, 0.25], [6.5, 0.5, 0.5], [8.5, 0.5, 0.5]])       # one held voxel, two new ones: five voxels in all
    m.insert(dev(q)), ref.insert(q)
    assert m.status() == (3, G.MAP_FULL, 3) and ref.status == G.MAP_FULL
    assert np.array_equal(same_map(m, ref, strict=False), before)
    with pytest.raises(RuntimeError, match="capacity = 4"):
        m.point_cloud()
    fits = G.VoxelMap(1.0, 4, capacity=4)
    fits.insert(dev(p)), fits.insert(dev(q[:2]))
    assert fits.check() == (4, 4) and len(fits.point_cloud()) == 4


# ---- one association -----------------------------------------------------------------------------------------------------------------------
def check_association(G, m, ref, source, max_distance, kernel):
    nn, dist, mask, c = R.associate(source, ref, max_distance, kernel)
    a = G.associate(dev(source), m, max_distance, kernel)
    assert np.array_equal(a.nn_index.cpu().numpy(), nn) and np.array_equal(a.mask.cpu().numpy(), mask)
    assert np.array_equal(bits(a.distance.cpu().numpy()), bits(dist))
    assert np.array_equal(bits(a.sums.cpu().numpy()), bits(R.tree_sums(c, rows=len(source))))
    return nn, dist, mask


@pytest.mark.parametrize("S", [255, 256, 257, 600])
def test_association_and_sums(G, S):
    """source counts straddle one, two and three blocks"""
    m, ref = both_maps(G, 2.0, 20, 8192)
    rng = np.random.default_rng(7)
    cloud = rng.uniform(-15.0, 15.0, (4000, 3))
    m.insert(dev(cloud)), ref.insert(cloud)
    source = np.concatenate([cloud[:S // 2] + rng.normal(0.0, 0.3, (S // 2, 3)), rng.uniform(-20.0, 20.0, (S - S // 2, 3))])
    nn, dist, mask = check_association(G, m, ref, source, 1.0, 0.4)
    assert mask.sum() > S // 4 and (~mask).sum() > S // 8 and (nn < 0).any()


def test_association_boundaries(G):
    """a correspondence at exactly max_distance is excluded (a 3-4-5 triple); of two equidistant neighbours the first in traversal
    order wins, inside a voxel and across voxels; a point without a neighbour"""
    m, ref = both_maps(G, 8.0, 20)
    held = np.array([[1.0, 1.0, 1.0], [7.0, 1.0, 1.0], [-0.5, 1.0, 20.0], [8.5, 1.0, 20.0], [1.0, 1.0, 41.0]])
    m.insert(dev(held)), ref.insert(held)
    source = np.array([[4.0, 5.0, 41.0], [4.0, 1.0, 1.0], [4.0, 1.0, 20.0], [100.0, 100.0, 100.0], [1.0, 1.0, 41.0]])
    nn, dist, mask = check_association(G, m, ref, source, 5.0, 0.5)
    assert dist[0] == 5.0 and not mask[0] and mask[[1, 2, 4]].all()
    assert nn.tolist() == [13 * 32, 13 * 32, 4 * 32, -1, 13 * 32] and dist[3] == np.finfo(np.float64).max and dist[4] == 0.0
    nn, dist, mask = check_association(G, m, ref, source, float(np.nextafter(5.0, 6.0)), 0.5)
    assert mask.tolist() == [True, True, True, False, True]


# ---- a whole alignment ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair(G, gold):
    """sweep 0 as the map, sweep 1's source, a guess 0.3 m and 1 degree off; the restatement's result for every iteration limit used"""
    c = R.Config(**R.SCENE_CONFIG)
    true = gold["true_poses"].copy()
    true[:, :3, 3] -= true[0, :3, 3]
    frame0 = R.downsample(gold["scans"][0], c.min_range, c.max_range, c.voxel_size)[0]
    source = R.downsample(gold["scans"][1], c.min_range, c.max_range, c.voxel_size)[1]
    ref = R.RefMap(c.voxel_size, 20)
    ref.insert(frame0, true[0])
    m = G.VoxelMap(c.voxel_size, 20, 8192)
    m.insert(dev(frame0), true[0])
    guess = R.compose(true[1], R.yaw_pose(0.25, -0.15, 0.05, np.deg2rad(1.0)))
    full = R.align(source, ref, guess, 6.0, 2.0 / 3.0)
    return m, ref, source, guess, full


def pose_bound(pose, iterations):
    """64 eps (1 + |t|) per step: sin / cos of the device may differ from libm's in the last place, and a step passes that on"""
    return max(iterations, 1) * 64 * EPS * (1.0 + np.linalg.norm(pose[:3, 3]))


def test_align_empty_map(G):
    m = G.VoxelMap(1.0, 20, 64)
    guess = R.yaw_pose(1.0, 2.0, 3.0, 0.1)
    pose, it = G.align_points_to_map(dev(np.ones((5, 3))), m, guess, 1.0, 1.0)
    assert it == 0 and np.array_equal(pose, guess)
    m.insert(dev(np.array([[0.5, 0.5, 0.5]])))
    m.prune([100.0, 0.0, 0.0], 1.0)                       # emptied on the device: found out by the first launch
    pose, it = G.align_points_to_map(dev(np.ones((5, 3))), m, guess, 1.0, 1.0)
    assert it == 0 and np.array_equal(pose, guess)
    assert G.align_record(dev(np.ones((5, 3))), m, guess, 1.0, 1.0).status == G.EMPTY_MAP


def test_align_equals_the_restatement(G, pair):
    m, ref, source, guess, (pose_ref, it_ref, status_ref) = pair
    assert status_ref == R.CONVERGED and it_ref > G.GROUP_SIZE + 1
    pose, it = G.align_points_to_map(dev(source), m, guess, 6.0, 2.0 / 3.0)
    diff = float(np.abs(pose - pose_ref).max())
    print(f"alignment: {it} iterations, largest pose difference {diff:.3g}, bound {pose_bound(pose_ref, it_ref):.3g}")
    assert it == it_ref and diff <= pose_bound(pose_ref, it_ref)
    again, it2 = G.align_points_to_map(dev(source), m, guess, 6.0, 2.0 / 3.0)
    assert it2 == it and np.array_equal(bits(again), bits(pose))


@pytest.mark.parametrize("limit", ["1", "2", "group - 1", "group", "group + 1"])
def test_align_iteration_limits(G, pair, limit):
    """never more launches than max_num_iterations, whatever the group size"""
    m, ref, source, guess, (_, it_ref, _) = pair
    n = eval(limit, {"group": G.GROUP_SIZE})
    assert n < it_ref
    pose_ref, its, status = R.align(source, ref, guess, 6.0, 2.0 / 3.0, max_num_iterations=n)
    r = G.align_record(dev(source), m, guess, 6.0, 2.0 / 3.0, max_num_iterations=n)
    pose, it = G.align_points_to_map(dev(source), m, guess, 6.0, 2.0 / 3.0, max_num_iterations=n)
    assert it == its == n == r.iterations and r.status == status == 0
    assert np.abs(pose - pose_ref).max() <= pose_bound(pose_ref, n)


def test_align_converges_on_the_last_step_of_a_group(G, pair):
    m, ref, source, guess, (pose_ref, it_ref, _) = pair
    for group in (it_ref, it_ref - 1, it_ref + 1, 1):
        pose, it = G.align_points_to_map(dev(source), m, guess, 6.0, 2.0 / 3.0, group_size=group)
        assert it == it_ref and np.abs(pose - pose_ref).max() <= pose_bound(pose_ref, it_ref)
    r = G.align_record(dev(source), m, guess, 6.0, 2.0 / 3.0, group_size=it_ref)
    assert r.status == G.CONVERGED and r.iterations == it_ref and r.dx_norm < 1e-4 and r.correspondences > 100


def test_align_degenerate(G, pair):
    """no correspondence at all: the status is set, one iteration ran, the pose is the guess"""
    m, ref, source, guess, _ = pair
    far = R.compose(R.yaw_pose(500.0, 0.0, 0.0, 0.0), guess)
    r = G.align_record(dev(source), m, far, 6.0, 2.0 / 3.0)
    pose_ref, its, status = R.align(source, ref, far, 6.0, 2.0 / 3.0)
    assert (r.status, r.iterations, r.correspondences) == (G.DEGENERATE, 1, 0) and (status, its) == (R.DEGENERATE, 1)
    pose, it = G.align_points_to_map(dev(source), m, far, 6.0, 2.0 / 3.0)
    assert it == 1 and np.array_equal(pose, pose_ref) and np.array_equal(pose, far)


# ---- the recorded traversals ---------------------------------------------------------------------------------------------------------------
def test_recorded_traversals_end_to_end(G, gold):
    """2 traversals x 5 frames: the iteration counts are the restatement's and every pose entry is within 64 d of the recorded
    poses, d the fixture's own sensitivity to rounding; a second run repeats every bit"""
    config = G.KissConfig(**R.SCENE_CONFIG)
    scans = [dev(s) for s in gold["scans"]]
    poses, its = G.register_traversals(scans, gold["log_poses"], gold["traj_ids"], config, capacity=1 << 16)
    d = float(gold["d"])
    diff = float(np.abs(poses - gold["poses"]).max())
    line = f"recorded traversals: largest pose difference {diff:.3g} against 64 d = {64 * d:.3g} (d = {d:.3g}); iterations {its.tolist()}"
    print(line)                     # scripts/icp_bench.py writes the same figure into profiles/icp.txt
    assert np.array_equal(its, gold["iterations"])
    assert diff <= 64 * d
    poses2, its2 = G.register_traversals(scans, gold["log_poses"], gold["traj_ids"], config, capacity=1 << 16)
    assert np.array_equal(its2, its) and np.array_equal(bits(poses2), bits(poses))
    err = lambda p: float(np.linalg.norm(p[:, :3, 3] - gold["true_poses"][:, :3, 3], axis=1).mean())
    assert err(poses) <= 0.5 * err(gold["log_poses"])
