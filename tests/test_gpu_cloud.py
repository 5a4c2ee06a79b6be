"""mtgs_amd.pointcloud on the device against tests/cloud_oracle.py (open3d's two operators written out in NumPy and SciPy, fp64).

Bounds.  A squared distance is a three-term sum of squares of rounded differences in fp32, at most about 4 units of 2^-24
relative, halved by the square root; everything after it (the square root, the sum of up to 31 terms, the division) is fp64
here and in the oracle, and a mis-ranked near-tie moves a term by no more than that: rtol = 1e-6 (atol = 0) for the averages, as
the neighbour tests hold for the distances, and for cloud_mean, std and the threshold, which are sums of them.  A point whose
average lies within 1e-5 (relative) of the threshold may fall on either side; elsewhere the masks are equal.  The voxel grid has
no tolerance: keys, counts and fp64 means are the oracle's bit for bit."""
import functools

import numpy as np
import pytest
import torch

from mtgs_amd import pointcloud, seed
from tests import cloud_oracle as orc

pytestmark = pytest.mark.gpu
RTOL = 1e-6
BAND = 1e-5
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def street(n):
    x = orc.street_cloud(n, 0)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def street_avg(n, nb):
    a = orc.avg_distances(street(n), nb)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def street_rgb(n):
    c = np.random.default_rng(100 + n).integers(0, 256, (n, 3), dtype=np.uint8)
    c.setflags(write=False)
    return c


def gpu(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def run_outlier(x, nb=20, ratio=0.5):
    keep, avg, stats = pointcloud.statistical_outlier_removal(gpu(x) if isinstance(x, np.ndarray) else x, nb, ratio, return_stats=True)
    assert keep.dtype == torch.bool and avg.dtype == torch.float64 and stats.dtype == torch.float64 and tuple(stats.shape) == (4,)
    return keep.cpu().numpy(), avg.cpu().numpy(), stats.cpu().numpy()


def check_outlier(x, nb, ratio, name, want_avg=None):
    """averages, statistics and the mask against the oracle; returns (keep, avg, stats, oracle's near-threshold count)"""
    keep, avg, stats = run_outlier(x, nb, ratio)
    want_avg = orc.avg_distances(x, nb) if want_avg is None else want_avg
    mean, std, thr, valid = orc.outlier_stats(want_avg, ratio)
    assert np.array_equal(avg == 0, want_avg == 0), f"{name}: the exact zeros differ"
    nz = want_avg != 0
    err = float((np.abs(avg - want_avg)[nz] / want_avg[nz]).max()) if nz.any() else 0.0
    print(f"{name}: avg max rel err {err:.3e}; cloud_mean {stats[0]:.9g} / {mean:.9g}, std {stats[1]:.9g} / {std:.9g}, "
          f"threshold {stats[2]:.9g} / {thr:.9g}, kept {keep.mean():.4f}")
    assert np.allclose(avg, want_avg, rtol=RTOL, atol=0), f"{name}: avg max relative error {err:.3e}"
    assert stats[3] == valid == x.shape[0]
    assert np.allclose(stats[:3], [mean, std, thr], rtol=RTOL, atol=0, equal_nan=True), (name, stats, mean, std, thr)
    with np.errstate(invalid="ignore"):
        want_keep = (want_avg > 0) & (want_avg < thr)
        near = np.abs(want_avg - thr) <= BAND * thr
    assert np.array_equal(keep[~near], want_keep[~near]), f"{name}: the mask differs away from the threshold"
    return keep, avg, stats, int(near.sum()), want_keep


@pytest.mark.parametrize("n", [4096, 20000])
def test_outlier_averages_statistics_and_mask(n):
    x = street(n)
    keep, avg, stats, near, want_keep = check_outlier(x, 20, 0.5, f"street_{n}", street_avg(n, 20))
    assert near == 0, "the oracle has a point within 1e-5 of the threshold: choose another cloud"
    assert np.array_equal(keep, want_keep)
    assert 0.6 < keep.mean() < 0.9


@pytest.mark.parametrize("nb", [2, 20, 32])
@pytest.mark.parametrize("ratio", [0.5, 2.0])
def test_outlier_parameters(nb, ratio):
    check_outlier(street(4096), nb, ratio, f"street_4096_nb{nb}_r{ratio}", street_avg(4096, nb))


@pytest.mark.parametrize("n", [1, 5, 19, 20, 21])
def test_outlier_small_clouds(n):
    """k = min(nb_neighbors, N); N = 1: avg 0, a NaN threshold, nothing kept"""
    x = street(4096)[1000:1000 + n]
    keep, avg, stats, _, want_keep = check_outlier(x, 20, 0.5, f"n{n}")
    assert np.array_equal(keep, want_keep)
    if n == 1:
        assert avg.tolist() == [0.0] and stats[0] == 0.0 and np.isnan(stats[1]) and np.isnan(stats[2]) and not keep.any()
    assert tuple(pointcloud.statistical_outlier_removal(torch.zeros(0, 3, device=DEV)).shape) == (0,)


def test_outlier_duplicates():
    x = street(4096).copy()
    dup = np.random.default_rng(5).choice(4096, 25, replace=False)
    x[dup] = x[dup[0]]
    keep, avg, stats, _, _ = check_outlier(x, 20, 0.5, "dup25")
    assert (avg[dup] == 0.0).all() and not keep[dup].any() and int((avg == 0).sum()) == 25
    pos = avg > 0
    assert stats[3] == 4096 and np.isclose(stats[0], avg[pos].sum() / 4096, rtol=1e-12, atol=0)     # left out of the sum, counted in valid
    same = np.full((64, 3), 2.5, np.float32)                           # every point identical: every avg 0, nothing kept
    keep, avg, stats = run_outlier(same)
    assert not avg.any() and not keep.any() and stats.tolist() == [0.0, 0.0, 0.0, 64.0]


def test_outlier_offset_and_strided():
    x = (street(4096).astype(np.float64) + 1e4).astype(np.float32)
    check_outlier(x, 20, 0.5, "offset_1e4")
    p = gpu(street(4096))
    wide = torch.cat([p, torch.full((4096, 1), float("nan"), device=DEV)], dim=1)            # [N, 4]: the view skips the NaN column
    view = wide[:, :3]
    assert not view.is_contiguous()
    a, b = run_outlier(p), run_outlier(view)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))


def test_non_finite_input_is_refused():
    for bad in (float("nan"), float("inf")):
        p = gpu(street(4096))
        p[17, 1] = bad
        with pytest.raises(ValueError, match="NaN or infinity"):
            pointcloud.statistical_outlier_removal(p)
        with pytest.raises(ValueError, match="NaN or infinity"):
            pointcloud.voxel_down_sample(p, gpu(street_rgb(4096)), 0.15)
    with pytest.raises(ValueError, match="nb_neighbors"):
        pointcloud.statistical_outlier_removal(gpu(street(4096)), 33)


def test_outlier_is_deterministic_and_order_independent():
    x = street(20000)
    k0, a0, s0 = run_outlier(x)
    k1, a1, s1 = run_outlier(x)
    assert np.array_equal(a0.view(np.uint64), a1.view(np.uint64)) and np.array_equal(k0, k1) and np.array_equal(s0.view(np.uint64), s1.view(np.uint64))
    perm = np.random.default_rng(8).permutation(20000)
    _, ap, _ = run_outlier(x[perm])
    assert np.array_equal(ap.view(np.uint64), a0[perm].view(np.uint64))


def test_knn_distances_are_unchanged():
    """seed.knn_distances shares its front with the filter now: its distances are still, bit for bit, the fp32 brute force
    ((dx dx + dy dy) + dz dz), sqrt, over all pairs, as at the parent commit"""
    x = gpu(street(20000))
    got = seed.knn_distances(x, 3)
    want = []
    for s in range(0, 20000, 1000):
        q = x[s:s + 1000]
        d = [q[:, None, a] - x[None, :, a] for a in range(3)]
        d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        d2[torch.arange(q.shape[0], device=DEV), torch.arange(s, s + q.shape[0], device=DEV)] = float("inf")
        want.append(torch.topk(d2, 3, dim=1, largest=False).values)
    want = np.sqrt(torch.cat(want).cpu().numpy().astype(np.float64)).astype(np.float32)     # the correctly rounded fp32 square root
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    with pytest.raises(ValueError):
        seed.knn_distances(x, 9)


def run_voxel(x, c, vs):
    xyz, rgb, counts, keys = pointcloud.voxel_down_sample(gpu(x), gpu(c), vs, return_keys=True)
    assert xyz.dtype == torch.float64 and rgb.dtype == torch.float64 and counts.dtype == torch.int32 and keys.dtype == torch.int64
    return keys.cpu().numpy(), xyz.cpu().numpy(), rgb.cpu().numpy(), counts.cpu().numpy()


def check_voxel(x, c, vs, name):
    got, want = run_voxel(x, c, vs), orc.voxel_down_sample(x, c, vs)
    print(f"{name}: {x.shape[0]} points -> {want[0].shape[0]} voxels, largest {int(want[3].max())}")
    for g, w, what in zip(got, want, ("keys", "xyz", "rgb", "counts")):
        assert g.shape == w.shape and g.dtype == w.dtype, (name, what, g.shape, w.shape)
        assert np.array_equal(g, w), f"{name}: {what} differ"
    assert (np.diff(got[0]) > 0).all() and int(got[3].sum()) == x.shape[0]
    return got


@pytest.mark.parametrize("n", [4096, 20000])
@pytest.mark.parametrize("vs", [0.15, 1.0])
def test_voxel_grid_is_the_oracle_bit_for_bit(n, vs):
    got = check_voxel(street(n), street_rgb(n), vs, f"street_{n}_{vs}")
    if vs == 1.0 and n == 20000:
        assert got[3].max() >= 10                              # tens of points in a voxel
    again = run_voxel(street(n), street_rgb(n), vs)
    assert all(np.array_equal(a, b) for a, b in zip(got, again))


def test_voxel_grid_boundaries_float_colours_and_corners():
    r = np.random.default_rng(11)
    vs = 0.25
    x = (r.integers(-20, 21, (3000, 3)) * (vs / 2)).astype(np.float32)          # exact multiples of voxel_size / 2: points on voxel faces
    check_voxel(x, street_rgb(4096)[:3000], vs, "boundaries")
    check_voxel(x, r.random((3000, 3)).astype(np.float32), vs, "float_colours")
    one = check_voxel(street(4096), street_rgb(4096), 1000.0, "single_voxel")
    assert one[3].tolist() == [4096]
    pt = check_voxel(street(4096)[7:8], street_rgb(4096)[7:8], 0.15, "one_point")
    assert pt[3].tolist() == [1] and np.array_equal(pt[1][0], street(4096)[7].astype(np.float64))
    heavy = np.concatenate([r.random((10000, 3)) * 0.1 + 0.2, street(4096)[:500].astype(np.float64) + [0, 0, 20]]).astype(np.float32)
    heavy = heavy[r.permutation(heavy.shape[0])]
    got = check_voxel(heavy, r.integers(0, 256, (heavy.shape[0], 3), dtype=np.uint8), 1.0, "heavy_voxel")
    assert got[3].max() >= 10000
    e = [torch.zeros(0, 3, device=DEV), torch.zeros(0, 3, dtype=torch.uint8, device=DEV)]
    assert [tuple(t.shape) for t in pointcloud.voxel_down_sample(*e, 0.15)] == [(0, 3), (0, 3), (0,)]


def test_voxel_grid_reads_a_column_strided_view_of_one_row_as_its_copy():
    """points = wide[:1, ::2]: one row has no row stride to tell the layout by, and the coordinates are two elements apart; read in
    place the voxel's mean would be (x, 50, y).  The backing row holds six elements."""
    wide = torch.full((1, 6), 50.0, device=DEV)
    wide[:, ::2] = torch.tensor([[1.25, -2.5, 3.75]], device=DEV)
    view, colors = wide[:, ::2], torch.tensor([[10, 20, 30]], dtype=torch.uint8, device=DEV)
    assert view.stride(1) == 2 and tuple(view.shape) == (1, 3)
    got, want = (pointcloud.voxel_down_sample(p, colors, 0.15, return_keys=True) for p in (view, view.contiguous()))
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert got[0].tolist() == [[1.25, -2.5, 3.75]] and got[2].tolist() == [1]


def test_voxel_grid_refuses_an_extent_beyond_21_bits():
    x = street(4096).copy()
    x[5, 1] = 4e5                                                 # 4e5 / 0.15 = 2.7e6 voxels along y
    with pytest.raises(ValueError, match="axis y"):
        orc.voxel_down_sample(x, street_rgb(4096), 0.15)
    with pytest.raises(ValueError, match="axis y needs more than 21 bits"):
        pointcloud.voxel_down_sample(gpu(x), gpu(street_rgb(4096)), 0.15)
    x[9, 0] = -5e5
    with pytest.raises(ValueError, match="axis x, y needs"):
        pointcloud.voxel_down_sample(gpu(x), gpu(street_rgb(4096)), 0.15)
    with pytest.raises(ValueError, match="voxel_size"):
        pointcloud.voxel_down_sample(gpu(x), gpu(street_rgb(4096)), 0.0)


def sort_rows(xyz, rgb):
    """by colour, then position: colours are exact, so a position that differs in its last bits cannot change the order"""
    order = np.lexsort((xyz[:, 2], xyz[:, 1], xyz[:, 0], rgb[:, 2], rgb[:, 1], rgb[:, 0]))
    return xyz[order], rgb[order]


def test_prepare_seed_cloud_end_to_end():
    n = 20000
    r = np.random.default_rng(21)
    sfm_xyz = (r.random((500, 3)) * [80, 16, 6] - [40, 8, 0]).astype(np.float32)
    sfm_rgb = r.integers(0, 256, (500, 3), dtype=np.uint8)
    a = 0.3
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], np.float32)
    T[:3, 3] = [150.0, 120.0, 40.0]                               # every transformed coordinate stays well away from zero
    want_xyz, want_rgb = orc.load_3d_points(street(n), street_rgb(n), sfm_xyz, sfm_rgb, T, 0.1)
    out = pointcloud.prepare_seed_cloud(gpu(street(n)), gpu(street_rgb(n)), gpu(sfm_xyz), gpu(sfm_rgb), transform=gpu(T), scale_factor=0.1)
    assert out["xyz"].dtype == torch.float32 and out["rgb"].dtype == torch.uint8 and out["xyz"].is_cuda
    P = want_xyz.shape[0]
    assert tuple(out["xyz"].shape) == (P, 3) and tuple(out["rgb"].shape) == (P, 3) and P > 5000
    # the SfM cloud is appended unfiltered and a voxel with one point keeps its colour: (c / 255.0 * 255) truncates back to c
    assert np.array_equal(out["rgb"][-500:].cpu().numpy(), sfm_rgb)
    got_xyz, got_rgb = sort_rows(out["xyz"].cpu().numpy(), out["rgb"].cpu().numpy())
    want_xyz, want_rgb = sort_rows(want_xyz, want_rgb)
    assert np.array_equal(got_rgb, want_rgb)
    err = float((np.abs(got_xyz - want_xyz) / np.abs(want_xyz)).max())
    print(f"prepare_seed_cloud: {n} + 500 points -> {P}, xyz max rel err {err:.3e}")
    assert np.allclose(got_xyz, want_xyz, rtol=RTOL, atol=0)
    node = seed.seed_gaussians(out, sh_degree=3, generator=torch.Generator(device=DEV).manual_seed(1))
    assert node["means"].shape[0] == P and node["features_rest"].shape == (P, 15, 3) and bool(torch.isfinite(node["scales"]).all())


def test_prepare_seed_cloud_fallback():
    e = torch.zeros(0, 3, device=DEV)
    out = pointcloud.prepare_seed_cloud(e, e.to(torch.uint8), generator=torch.Generator(device=DEV).manual_seed(2))
    assert tuple(out["xyz"].shape) == (200, 3) and out["xyz"].dtype == torch.float32 and bool(out["xyz"].any())
    assert tuple(out["rgb"].shape) == (200, 3) and out["rgb"].dtype == torch.uint8 and not bool(out["rgb"].any())
    same = torch.full((50, 3), 1.5, device=DEV)                    # the filter keeps nothing of a cloud of duplicates
    out = pointcloud.prepare_seed_cloud(same, torch.zeros(50, 3, dtype=torch.uint8, device=DEV))
    assert tuple(out["xyz"].shape) == (200, 3)
