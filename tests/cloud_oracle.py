"""The oracle of mtgs_amd.pointcloud: open3d's remove_statistical_outlier and voxel_down_sample written out in NumPy and SciPy
(fp64), since open3d itself cannot be installed next to this project, and _load_3D_points (nuplan_dataparser.py:460-500) on top.

remove_statistical_outlier (open3d PointCloud.cpp): a k-d tree query for knn = nb_neighbors against the cloud that holds the
query point returns min(knn, N) squared distances, the point itself first at 0;  avg_distances[i] = the mean of their square
roots;  valid = N;  cloud_mean = (sum of avg over avg > 0) / valid;  std = sqrt((sum of (avg - cloud_mean)^2 over avg > 0) /
(valid - 1));  a point stays when avg > 0 and avg < cloud_mean + std_ratio * std.

voxel_down_sample: voxel_min_bound = min_bound - voxel_size * 0.5;  index = floor((p - voxel_min_bound) / voxel_size) per axis;
every voxel averages its points with AccumulatedPoint: point_ += p and color_ += c per point in input order, then one division
by the count.  The rows are returned in ascending order of key = ix << 42 | iy << 21 | iz (open3d's own order is that of a hash map).
"""
import numpy as np
from scipy.spatial import cKDTree

QBITS = 21
QMAX = (1 << QBITS) - 1


def street_cloud(n, seed):
    """a ground plane, two walls and clutter"""
    r = np.random.default_rng(seed)
    n_g, n_w = n // 2, n // 4
    n_c = n - n_g - n_w
    ground = np.stack([r.uniform(-40, 40, n_g), r.uniform(-8, 8, n_g), r.normal(0, 0.02, n_g)], -1)
    walls = np.stack([r.uniform(-40, 40, n_w), np.where(r.random(n_w) < 0.5, -8.0, 8.0) + r.normal(0, 0.03, n_w), r.uniform(0, 6, n_w)], -1)
    clutter = np.stack([r.uniform(-60, 60, n_c), r.uniform(-30, 30, n_c), r.uniform(0, 15, n_c)], -1)
    return np.concatenate([ground, walls, clutter]).astype(np.float32)


def avg_distances(points, nb_neighbors):
    p = np.asarray(points, np.float32).astype(np.float64)
    n = p.shape[0]
    k = min(int(nb_neighbors), n)
    d, _ = cKDTree(p).query(p, k=k, workers=-1)
    return d.reshape(n, k).sum(axis=1) / k


def outlier_stats(avg, std_ratio):
    """cloud_mean, std, threshold, valid"""
    valid = avg.shape[0]
    pos = avg > 0
    cloud_mean = float(np.sum(avg[pos])) / valid
    with np.errstate(invalid="ignore", divide="ignore"):
        std = float(np.sqrt(np.float64(np.sum((avg[pos] - cloud_mean) ** 2)) / np.float64(valid - 1)))
    return cloud_mean, std, cloud_mean + std_ratio * std, valid


def statistical_outlier(points, nb_neighbors=20, std_ratio=0.5):
    """keep [N] bool, avg [N], (cloud_mean, std, threshold, valid)"""
    avg = avg_distances(points, nb_neighbors)
    stats = outlier_stats(avg, std_ratio)
    with np.errstate(invalid="ignore"):
        keep = (avg > 0) & (avg < stats[2])
    return keep, avg, stats


def colors_f64(colors):
    colors = np.asarray(colors)
    return colors.astype(np.float64) / 255.0 if colors.dtype == np.uint8 else colors.astype(np.float32).astype(np.float64)


def voxel_keys(points, voxel_size):
    p = np.asarray(points, np.float32).astype(np.float64)
    voxel_min_bound = p.min(axis=0) - voxel_size * 0.5
    index = np.floor((p - voxel_min_bound) / voxel_size)
    for a in range(3):
        if not (index[:, a] <= QMAX).all():
            raise ValueError(f"the voxel index of axis {'xyz'[a]} needs more than {QBITS} bits")
    index = index.astype(np.int64)
    return index[:, 0] << (2 * QBITS) | index[:, 1] << QBITS | index[:, 2]


def voxel_down_sample(points, colors, voxel_size):
    """keys [M] int64 ascending, xyz [M, 3] f64, rgb [M, 3] f64, counts [M] int32"""
    p = np.asarray(points, np.float32).astype(np.float64)
    c = colors_f64(colors)
    key = voxel_keys(points, voxel_size)
    acc = {}
    for i, kk in enumerate(key.tolist()):                   # AddPoint, in input order
        a = acc.get(kk)
        if a is None:
            a = acc[kk] = [np.zeros(3), np.zeros(3), 0]
        a[0] += p[i]
        a[1] += c[i]
        a[2] += 1
    keys = np.array(sorted(acc), np.int64)
    xyz = np.array([acc[kk][0] / float(acc[kk][2]) for kk in keys.tolist()], np.float64).reshape(-1, 3)
    rgb = np.array([acc[kk][1] / float(acc[kk][2]) for kk in keys.tolist()], np.float64).reshape(-1, 3)
    counts = np.array([acc[kk][2] for kk in keys.tolist()], np.int32)
    return keys, xyz, rgb, counts


def load_3d_points(lidar_xyz, lidar_rgb, sfm_xyz, sfm_rgb, transform, scale_factor, nb_neighbors=20, std_ratio=0.5, voxel_size=0.15):
    """_load_3D_points: xyz float32 [P, 3], rgb uint8 [P, 3]"""
    keep, _, _ = statistical_outlier(lidar_xyz, nb_neighbors, std_ratio)
    _, xyz, rgb, _ = voxel_down_sample(lidar_xyz[keep], lidar_rgb[keep], voxel_size)
    if sfm_xyz is not None:
        xyz = np.concatenate([xyz, np.asarray(sfm_xyz, np.float64)])
        rgb = np.concatenate([rgb, colors_f64(sfm_rgb)])
    x = xyz.astype(np.float32)
    t = np.asarray(transform, np.float32)
    x = x @ t[:3, :3].T + t[:3, 3]
    x = x * np.float32(scale_factor)
    return x, (rgb * 255).astype(np.uint8)
