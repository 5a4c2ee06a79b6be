"""mtgs_amd.pointcloud without a GPU: the oracle (tests/cloud_oracle.py) against answers worked out by hand, the library's
refusals by name before any launch, and no CPU fallback in the Python layer."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from mtgs_amd import pointcloud
from tests import cloud_oracle as orc

# three copies of one point (with k = 3 their two nearest others are at distance 0), a point half a unit from them that lands
# exactly on a voxel boundary, and two far ones; every coordinate of the first four is negative
PTS = np.array([[-1, -1, -1], [-1, -1, -1], [-1, -1, -1], [2, -1, -1], [2, 3, -1], [-0.5, -1, -1]], np.float32)
RGB = np.array([[0, 0, 0], [255, 0, 30], [0, 255, 60], [10, 20, 30], [200, 100, 50], [255, 255, 255]], np.uint8)


def test_oracle_outlier_statistics_by_hand():
    keep, avg, (mean, std, thr, valid) = orc.statistical_outlier(PTS, nb_neighbors=3, std_ratio=0.5)
    s = math.sqrt(2.5 ** 2 + 4.0 ** 2)                       # from (2, 3, -1) to (-0.5, -1, -1)
    want = np.array([0.0, 0.0, 0.0, (2.5 + 3.0) / 3, (4.0 + s) / 3, (0.5 + 0.5) / 3])
    assert np.array_equal(avg[:3], [0.0, 0.0, 0.0])           # the duplicate group: exact zeros
    assert np.allclose(avg, want, rtol=1e-15, atol=0)
    assert valid == 6
    m = (want[3] + want[4] + want[5]) / 6                     # the zeros are left out of the sum and counted in the divisor
    sd = math.sqrt(sum((a - m) ** 2 for a in want[3:]) / 5)
    assert math.isclose(mean, m, rel_tol=1e-15) and math.isclose(std, sd, rel_tol=1e-15) and math.isclose(thr, m + 0.5 * sd, rel_tol=1e-15)
    # m = 0.8454, sd = 1.0472, threshold = 1.3690: only the point next to the duplicates stays (avg = 0.3333, 1.8333, 2.9057)
    assert keep.tolist() == [False, False, False, False, False, True]
    assert orc.statistical_outlier(PTS, 3, 1.5)[0].tolist() == [False, False, False, True, False, True]      # threshold 2.4162
    # nb_neighbors above N: k = N
    assert np.allclose(orc.avg_distances(PTS[3:], 20), [(4 + 2.5) / 3, (4 + s) / 3, (2.5 + s) / 3], rtol=1e-15, atol=0)
    keep1, avg1, st1 = orc.statistical_outlier(PTS[:1], 20, 0.5)
    assert avg1.tolist() == [0.0] and math.isnan(st1[2]) and not keep1.any()


def test_oracle_voxel_grid_by_hand():
    keys, xyz, rgb, counts = orc.voxel_down_sample(PTS, RGB, 1.0)
    # voxel_min_bound = (-1.5, -1.5, -1.5): -0.5 maps to exactly 1.0, the lower face of voxel 1
    assert keys.tolist() == [0, 1 << 42, 3 << 42, 3 << 42 | 4 << 21]
    assert counts.tolist() == [3, 1, 1, 1] and counts.dtype == np.int32
    assert np.array_equal(xyz, [[-1, -1, -1], [-0.5, -1, -1], [2, -1, -1], [2, 3, -1]])
    assert np.array_equal(rgb[0], [(0.0 + 255 / 255.0 + 0.0) / 3, (0.0 + 0.0 + 255 / 255.0) / 3, (0.0 + 30 / 255.0 + 60 / 255.0) / 3])
    assert np.array_equal(rgb[1:], RGB[[5, 3, 4]].astype(np.float64) / 255.0)
    f = orc.voxel_down_sample(PTS, RGB.astype(np.float32) / np.float32(255), 1.0)
    assert np.array_equal(f[0], keys) and np.allclose(f[2], rgb, rtol=1e-7, atol=0)
    with pytest.raises(ValueError, match="axis y"):
        orc.voxel_down_sample(np.array([[0, 0, 0], [1, 4e5, 1]], np.float32), RGB[:2], 0.15)
    # (c / 255.0 * 255) truncates back to c: a voxel with one point keeps its colour
    c = np.arange(256, dtype=np.uint8)
    assert np.array_equal((c.astype(np.float64) / 255.0 * 255).astype(np.uint8), c)


def test_street_cloud_has_no_point_near_the_threshold():
    """the clouds of the device mask test: no average within 1e-5 (relative) of the threshold"""
    for n in (4096, 20000):
        keep, avg, (_, _, thr, _) = orc.statistical_outlier(orc.street_cloud(n, 0), 20, 0.5)
        assert int((np.abs(avg - thr) <= 1e-5 * thr).sum()) == 0
        assert 0.6 < keep.mean() < 0.9


def test_library_refuses_bad_arguments_by_name(hip_lib):
    n = C.c_size_t(0)
    one = C.c_void_p(16)                              # a non-null pointer that is never dereferenced: every call below is refused
    err = lambda: hip_lib.mtgs_rast_last_error()
    big = 1 << 40
    # workspace sizes
    assert hip_lib.mtgs_cloud_outlier_workspace_bytes(1000, 20, C.byref(n)) == 0 and n.value >= 1000 * (8 + 8 + 4 + 4 + 16)
    small = n.value
    assert hip_lib.mtgs_cloud_outlier_workspace_bytes(2_000_000, 20, C.byref(n)) == 0 and n.value > small
    assert hip_lib.mtgs_cloud_outlier_workspace_bytes(0, 20, C.byref(n)) == 0
    assert hip_lib.mtgs_cloud_outlier_workspace_bytes(1000, 20, None) == 1 and b"null pointer: bytes" in err()
    assert hip_lib.mtgs_cloud_outlier_workspace_bytes(1 << 31, 20, C.byref(n)) == 1 and b"N outside" in err()
    assert hip_lib.mtgs_cloud_voxel_workspace_bytes(1000, C.byref(n)) == 0 and n.value >= 1000 * (8 + 8 + 4 + 4 + 4)
    assert hip_lib.mtgs_cloud_voxel_workspace_bytes(0, C.byref(n)) == 0
    assert hip_lib.mtgs_cloud_voxel_workspace_bytes(1000, None) == 1 and b"null pointer: bytes" in err()
    assert hip_lib.mtgs_cloud_voxel_workspace_bytes(-1, C.byref(n)) == 1 and b"N outside" in err()
    # the outlier filter
    out = lambda **kw: hip_lib.mtgs_cloud_outlier(*{**dict(N=1000, nb=20, ratio=0.5, points=one, stride=3, avg=one, stats=one, keep=one,
                                                           status=one, ws=one, ws_bytes=big, stream=None), **kw}.values())
    for nb in (1, 33, 0, -3):
        assert out(nb=nb) == 1 and b"nb_neighbors outside [2, 32]" in err()
        assert hip_lib.mtgs_cloud_outlier_workspace_bytes(1000, nb, C.byref(n)) == 1 and b"nb_neighbors outside" in err()
    for N in (-1, 1 << 31):
        assert out(N=N) == 1 and b"N outside" in err()
    assert out(stride=2) == 1 and b"row_stride" in err()
    for name in ("points", "avg", "stats", "keep", "status", "ws"):
        assert out(**{name: None}) == 1 and b"null pointer: " + name.encode() in err()
    assert out(ws=C.c_void_p(1 << 20), ws_bytes=64) != 0 and b"workspace" in err()
    assert hip_lib.mtgs_cloud_outlier(0, 20, 0.5, None, 3, None, None, None, None, None, 0, None) == 0
    # the voxel grid
    vox = lambda **kw: hip_lib.mtgs_cloud_voxel(*{**dict(N=1000, vs=0.15, points=one, stride=3, colors=one, u8=1, out_xyz=one, out_rgb=one,
                                                         counts=one, out_keys=None, n_voxels=one, status=one, ws=one, ws_bytes=big,
                                                         stream=None), **kw}.values())
    for vs in (0.0, -0.15, float("inf"), float("nan")):
        assert vox(vs=vs) == 1 and b"voxel_size" in err()
    for N in (-1, 1 << 31):
        assert vox(N=N) == 1 and b"N outside" in err()
    assert vox(stride=2) == 1 and b"row_stride" in err()
    for name in ("points", "colors", "out_xyz", "out_rgb", "counts", "n_voxels", "status", "ws"):
        assert vox(**{name: None}) == 1 and b"null pointer: " + name.encode() in err()
    assert vox(ws=C.c_void_p(1 << 20), ws_bytes=64) != 0 and b"workspace" in err()
    assert hip_lib.mtgs_cloud_voxel(0, 0.15, None, 3, None, 1, None, None, None, None, None, None, None, 0, None) == 0
    # mtgs_knn keeps its limit
    assert hip_lib.mtgs_knn(1000, 9, one, 3, one, None, one, one, 1 << 30, None) == 1 and b"k outside [1, 8]" in err()


def test_no_cpu_fallback_and_argument_checks():
    x, c = torch.rand(100, 3), torch.zeros(100, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pointcloud.statistical_outlier_removal(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pointcloud.voxel_down_sample(x, c, 0.15)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pointcloud.prepare_seed_cloud(x, c)
    import mtgs_amd
    assert mtgs_amd.prepare_seed_cloud is pointcloud.prepare_seed_cloud
    assert mtgs_amd.statistical_outlier_removal is pointcloud.statistical_outlier_removal
    assert mtgs_amd.voxel_down_sample is pointcloud.voxel_down_sample
