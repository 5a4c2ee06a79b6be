"""mtgs_amd.seed without a GPU: the fixture is pinned by an fp64 brute force, the library refuses bad arguments by name before
any launch, and the Python layer has no CPU fallback."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

from mtgs_amd import seed

GOLD = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def ref():
    return np.load(GOLD / "seed_ref.npz")


def cloud_of(ref, name):
    key = f"{name}_xyz"
    return ref[key] if key in ref.files else ref[str(ref[f"{name}_xyz_from"]) + "_xyz"]


def brute_force(x, k):
    """the k smallest distances to the other points in fp64 from the float32 coordinates"""
    x = x.astype(np.float64)
    d = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1))
    np.fill_diagonal(d, np.inf)
    return np.sort(d, axis=1)[:, :k]


def test_fixture_distances_are_the_fp64_brute_force(ref):
    """sklearn computes in fp64 from the float32 input and the fixture stores the result as float32: an fp64 brute force rounded
    the same way agrees to one float32 rounding (sklearn's tree may sum the squares in another order)."""
    for name in ref["knn_cases"]:
        x, k = cloud_of(ref, name), int(ref[f"{name}_k"])
        want, got = brute_force(x, k), ref[f"{name}_dist"]
        assert got.shape == (x.shape[0], k) and got.dtype == np.float32
        assert np.array_equal(got == 0, want == 0), name
        assert np.allclose(got, want, rtol=1.2e-7, atol=0), name
    d = ref["duplicates_dist"]
    assert (d == 0).all(axis=1).sum() >= 4          # the point present four times
    want = brute_force(ref["seed_xyz"], 3)
    assert np.allclose(ref["seed_dist"], want, rtol=1.2e-7, atol=0)
    assert np.isneginf(ref["seed_scales"]).all(axis=1).sum() == 4


def test_library_refuses_bad_arguments_by_name(hip_lib):
    n = C.c_size_t(0)
    one = C.c_void_p(16)                              # a non-null pointer that is never dereferenced: every call below is refused
    err = lambda: hip_lib.mtgs_rast_last_error()
    assert hip_lib.mtgs_knn_workspace_bytes(1000, 3, C.byref(n)) == 0 and n.value >= 1000 * (8 + 8 + 4 + 4 + 16)
    small = n.value
    assert hip_lib.mtgs_knn_workspace_bytes(2_000_000, 3, C.byref(n)) == 0 and n.value > small
    assert hip_lib.mtgs_knn_workspace_bytes(0, 3, C.byref(n)) == 0
    assert hip_lib.mtgs_knn_workspace_bytes(1000, 3, None) == 1 and b"bytes" in err()
    assert hip_lib.mtgs_knn_workspace_bytes(1 << 31, 3, C.byref(n)) == 1 and b"N outside" in err()
    for k in (0, 9):
        assert hip_lib.mtgs_knn_workspace_bytes(1000, k, C.byref(n)) == 1 and b"k outside" in err()
        assert hip_lib.mtgs_knn(1000, k, one, 3, one, None, one, one, 1 << 30, None) == 1 and b"k outside" in err()
        assert hip_lib.mtgs_seed_fwd(10, k, one, one, None, 3, 3, one, one, one, 3, one, None) == 1 and b"k outside" in err()
    for N in (1, 3):
        assert hip_lib.mtgs_knn(N, 3, one, 3, one, None, one, one, 1 << 30, None) == 1 and b"N must exceed k" in err()
    assert hip_lib.mtgs_knn(0, 3, None, 3, None, None, None, None, 0, None) == 0
    assert hip_lib.mtgs_seed_fwd(0, 3, None, None, None, 3, 3, None, None, None, 3, None, None) == 0
    for i, name in ((2, b"points"), (4, b"dist"), (6, b"status"), (7, b"ws")):
        args = [1000, 3, one, 3, one, None, one, one, 1 << 30, None]
        args[i] = None
        assert hip_lib.mtgs_knn(*args) == 1 and b"null pointer: " + name in err()
    assert hip_lib.mtgs_knn(1000, 3, one, 3, one, None, one, C.c_void_p(1 << 20), 64, None) != 0 and b"workspace" in err()
    assert hip_lib.mtgs_knn(1000, 3, one, 2, one, None, one, one, 1 << 30, None) == 1 and b"row_stride" in err()
    for i, name in ((2, b"knn_dist"), (3, b"rgb"), (7, b"scales"), (9, b"features_dc"), (11, b"opacities")):
        args = [10, 3, one, one, None, 3, 3, one, one, one, 3, one, None]
        args[i] = None
        assert hip_lib.mtgs_seed_fwd(*args) == 1 and b"null pointer: " + name in err()
    assert hip_lib.mtgs_seed_fwd(10, 3, one, one, one, 3, 3, one, None, one, 3, one, None) == 1 and b"quats" in err()
    assert hip_lib.mtgs_seed_fwd(10, 3, one, one, None, 3, 2, one, one, one, 3, one, None) == 1 and b"scale_dim" in err()
    assert hip_lib.mtgs_seed_fwd(10, 3, one, one, None, 5, 3, one, one, one, 3, one, None) == 1 and b"sh_degree" in err()


def test_no_cpu_fallback():
    x = torch.rand(100, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        seed.knn_distances(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        seed.seed_gaussians({"xyz": x, "rgb": torch.zeros(100, 3)}, 3)
    with pytest.raises(ValueError):
        seed.seed_gaussians({"xyz": x, "rgb": torch.zeros(100, 3)}, 3, scale_dim=2)
    with pytest.raises(ValueError):
        seed.seed_gaussians({"xyz": x, "rgb": torch.zeros(100, 3)}, 3, features_dc_dim=1)


def test_empty_node_shapes():
    """_skip_current_model: __empty_gaussians(0, dim_sh) (vanilla_gaussian_splatting.py:198-217)"""
    from mtgs_amd.checkpoint import GAUSS_PARAM_NAMES
    e = {"xyz": torch.zeros(0, 3), "rgb": torch.zeros(0, 3)}
    out = seed.seed_gaussians(e, 3)
    assert {k: tuple(v.shape) for k, v in out.items()} == {"means": (0, 3), "scales": (0, 3), "quats": (0, 4), "features_dc": (0, 3),
                                                           "features_rest": (0, 15, 3), "opacities": (0, 1)}
    assert set(out) <= set(GAUSS_PARAM_NAMES) and all(v.dtype == torch.float32 for v in out.values())
    assert tuple(seed.seed_gaussians(e, 0, scale_dim=1)["scales"].shape) == (0, 1)
    assert tuple(seed.seed_gaussians(e, 0)["features_rest"].shape) == (0, 0, 3)
    assert tuple(seed.seed_gaussians(e, 2, features_dc_dim=5)["features_dc"].shape) == (0, 5, 3)


def test_fixture_conventions(ref):
    h = np.load(GOLD / "ref_helpers.npz")
    c0 = float(ref["C0"])
    assert np.allclose((h["rgb"] - 0.5) / c0, h["rgb2sh"], rtol=1e-6, atol=1e-7)
    assert np.allclose(h["rgb2sh"] * c0 + 0.5, h["rgb"], rtol=1e-6, atol=1e-7)
    assert [seed.num_sh_bases(int(d)) for d in h["degrees"]] == [int(n) for n in h["num_sh_bases"]]
    rgb = ref["seed_rgb"].astype(np.float32)
    assert np.array_equal((rgb / np.float32(255) - np.float32(0.5)) / np.float32(c0), ref["seed_dc_sh"])
    # the special normals: +z -> identity, -z -> the reference's non-unit (0, -0, -0, sqrt(2) / 2), zero -> NaN
    q = ref["seed_quats32"]
    assert np.array_equal(q[0], [1, 0, 0, 0]) and np.array_equal(q[1], np.array([0, -0.0, -0.0, np.sqrt(0.5)], np.float32))
    assert np.signbit(q[1][1:3]).all() and np.isnan(q[6]).all() and int(ref["seed_special_rows"]) == 7


def test_sky_radius_rule_and_sampling_on_a_cpu_generator():
    """skybox_gaussian_splatting.py:51-91"""
    import math
    assert seed.sky_radius(1000.0, 50.0) == 1000.0          # at least ten scene extents away: kept
    assert seed.sky_radius(1000.0, 150.0) == 1000.0         # closer than ten extents, but beyond two
    assert seed.sky_radius(1000.0, 700.0) == 1400.0         # pushed out to two extents
    for kind in ("spheric", "volumetric", "hemispheric"):
        p = seed.sky_points(500, 1000.0, 150.0, kind, generator=torch.Generator().manual_seed(5), device="cpu")
        q = seed.sky_points(500, 1000.0, 150.0, kind, generator=torch.Generator().manual_seed(5), device="cpu")
        assert torch.equal(p["xyz"], q["xyz"]) and bool((p["rgb"] == 255).all()) and tuple(p["xyz"].shape) == (500, 3)
        r = p["xyz"].norm(dim=1)
        lo, hi = {"spheric": (1000.0, 1000.0), "volumetric": (0.0, 1000.0), "hemispheric": (150.0, 1000.0)}[kind]
        assert bool((r >= lo * (1 - 1e-5)).all() and (r <= hi * (1 + 1e-5)).all())
        cos_phi = p["xyz"][:, 2] / r
        assert bool((cos_phi >= -1e-6).all() and (cos_phi <= math.cos(math.pi / 4) + 1e-6).all())
