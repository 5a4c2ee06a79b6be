"""The oriented crop box on the GPU (mtgs_amd/crop.py, csrc/crop.hip): mtgs_crop_select against the NumPy fp32 formula of
tests/crop_refs.py and mtgs_crop_gather against torch indexing, both bit for bit -- there is no tolerance anywhere in this file --
at the wave, block and scan-tile edges (scan.hpp: 2048 rows per workgroup); `crop_gaussians` through the two collectors; and the
render of a cropped set against the render of the torch-indexed one."""
import numpy as np
import pytest
import torch

from mtgs_amd import crop
from mtgs_amd._inputs import point_rows
from mtgs_amd.crop import OrientedBox, crop_gaussians
from tests import crop_refs as R
from tests.util import small_scene

pytestmark = pytest.mark.gpu
DEV = "cuda"
TILE = 2048
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097, 100_003]


@pytest.fixture(scope="module")
def lib(hip_lib):
    assert torch.cuda.is_available()
    return hip_lib


def unit_box():
    return OrientedBox(np.eye(3), np.zeros(3), np.full(3, 2.0))


def select(points, box):
    """(kept indices [count], count, mask [N]) of mtgs_crop_select as NumPy arrays"""
    keep_ids, count, mask = crop._select(points, box, want_mask=True)
    n = int(count.item())
    assert keep_ids.dtype == torch.int32 and count.dtype == torch.int64 and mask.dtype == torch.uint8
    assert 0 <= n <= points.shape[0]
    return keep_ids[:n].cpu().numpy(), n, mask.cpu().numpy()


def check_select(points_np, box, name):
    want = R.within_np(points_np, box.box)
    ids, n, mask = select(torch.tensor(points_np, device=DEV), box)
    assert n == int(want.sum()), (name, n, int(want.sum()))
    assert np.array_equal(ids, np.nonzero(want)[0]), name
    assert np.array_equal(mask, want.astype(np.uint8)), name
    return want


@pytest.mark.parametrize("N", SIZES)
def test_select_equals_the_fp32_formula(lib, N):
    """keep-all, keep-none, exactly one kept row at the first and at the last row of a scan tile (and of the array), the random box"""
    inside, outside = np.zeros((N, 3), dtype=np.float32), np.full((N, 3), 5.0, dtype=np.float32)
    assert check_select(inside, unit_box(), "keep-all").all()
    assert not check_select(outside, unit_box(), "keep-none").any()
    last_tile = (N - 1) // TILE * TILE if N else 0
    for row in sorted({0, N - 1, last_tile, last_tile - 1, TILE - 1} & set(range(N))):
        pts = outside.copy()
        pts[row] = 0.0
        want = check_select(pts, unit_box(), f"only row {row}")
        assert want.sum() == 1 and want[row]
    box = R.random_box()
    pts = R.random_points(N, seed=N)
    want = check_select(pts, box, "random box")
    if N >= 2047:
        assert 0.01 * N < want.sum() < 0.1 * N
    # the within() of the box is the same decision
    assert np.array_equal(box.within(torch.tensor(pts, device=DEV)).cpu().numpy(), want)


@pytest.mark.parametrize("N", [1, 65, 2049, 100_003])
def test_select_reads_a_strided_view_in_place(lib, N):
    box, pts = R.random_box(), R.random_points(N, seed=N)
    wide = torch.full((N, 4), float("nan"), device=DEV)
    wide[:, :3] = torch.tensor(pts, device=DEV)
    view = wide[:, :3]
    assert N == 1 or point_rows(view).data_ptr() == wide.data_ptr() and point_rows(view).stride(0) == 4
    a, b = select(view, box), select(view.contiguous(), box)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert np.array_equal(a[2], R.within_np(pts, box.box).astype(np.uint8))


def test_within_reads_any_layout_of_a_single_row_and_of_columns(lib):
    """a [1, 3] view with a column stride (N = 1 has no row stride to check) and a [N, 3] view of every other column"""
    box = unit_box()
    wide = torch.tensor([[0.5, 9.0, 0.5, 9.0, 0.5, 9.0], [9.0, 0.0, 9.0, 0.0, 9.0, 0.0], [0.1, 0.2, 0.3, 0.4, 9.0, 0.6]], device=DEV)
    for rows in (wide[:1, ::2], wide[1:2, ::2], wide[:, ::2], wide[:, 1::2]):
        assert rows.stride(1) == 2
        assert torch.equal(box.within(rows).cpu(), box.within(rows.cpu())) and torch.equal(box.within(rows), box.within(rows.contiguous()))
    assert box.within(wide[:, ::2]).tolist() == [True, False, False] and box.within(wide[:, 1::2]).tolist() == [False, True, True]


def test_select_drops_nan_and_inf_rows(lib):
    pts = np.zeros((300, 3), dtype=np.float32)
    for i, bad in enumerate((np.nan, np.inf, -np.inf)):
        for axis in range(3):
            pts[10 + 3 * i + axis, axis] = bad
    pts[100, 0] = 1.0                                   # on a face: out
    pts[101, 0] = np.nextafter(np.float32(1.0), np.float32(0.0))
    want = check_select(pts, unit_box(), "non-finite rows")
    assert want.sum() == 300 - 10 and not want[10:19].any() and not want[100] and want[101]


# ---- gather --------------------------------------------------------------------------------------------------------------------
def table(N, n_tensors, seed):
    """n_tensors tensors with N rows each: float rows of 1, 3, 4, 45 and 48 floats ([N], [N, 1], [N, 15, 3], ... shapes), an int64
    model_id, int32 and float64 rows, repeated in that order"""
    g = torch.Generator().manual_seed(seed)
    kinds = [lambda: torch.randn(N, generator=g), lambda: torch.randn(N, 3, generator=g), lambda: torch.randn(N, 4, generator=g),
             lambda: torch.randn(N, 15, 3, generator=g), lambda: torch.randn(N, 48, generator=g),
             lambda: torch.randint(-2 ** 40, 2 ** 40, (N,), generator=g, dtype=torch.int64),
             lambda: torch.randn(N, 1, generator=g), lambda: torch.randint(0, 1000, (N, 5), generator=g, dtype=torch.int32),
             lambda: torch.randn(N, 2, generator=g, dtype=torch.float64)]
    return [kinds[i % len(kinds)]().to(DEV) for i in range(n_tensors)]


@pytest.mark.parametrize("N, n_tensors", [(1, 6), (300, 6), (5000, 9), (5000, 16), (2049, 17)])
def test_gather_equals_torch_indexing(lib, N, n_tensors):
    """every tensor bit-equal to v[ids.long()]; 16 tensors are one launch, 17 are two"""
    tensors = table(N, n_tensors, seed=N + n_tensors)
    g = torch.Generator().manual_seed(5)
    for share in (0.5, 0.03, 1.0):
        keep = torch.rand(N, generator=g) < share
        keep[N - 1] = True
        ids = torch.nonzero(keep).flatten().to(torch.int32).to(DEV)
        got = crop.gather_rows(tensors, ids, ids.numel())
        assert len(got) == n_tensors
        for v, o in zip(tensors, got):
            want = v[ids.long()]
            assert o.dtype == v.dtype and o.shape == want.shape and o.is_contiguous()
            assert torch.equal(o.view(torch.int32) if o.dtype.is_floating_point and o.element_size() == 4 else o,
                               want.view(torch.int32) if o.dtype.is_floating_point and o.element_size() == 4 else want)


def test_gather_of_nothing_keeps_shapes_and_dtypes(lib):
    tensors = table(100, 9, seed=1)
    got = crop.gather_rows(tensors, torch.empty(0, dtype=torch.int32, device=DEV), 0)
    for v, o in zip(tensors, got):
        assert o.shape == (0,) + tuple(v.shape[1:]) and o.dtype == v.dtype and o.device == v.device


def test_gather_takes_non_contiguous_sources_and_refuses_odd_rows(lib):
    wide = torch.randn(500, 8, device=DEV)
    ids = torch.arange(0, 500, 7, dtype=torch.int32, device=DEV)
    got, = crop.gather_rows([wide[:, 1:6]], ids, ids.numel())
    assert torch.equal(got, wide[:, 1:6][ids.long()])
    with pytest.raises(TypeError, match="4-byte words"):
        crop.gather_rows([torch.zeros(500, 3, dtype=torch.uint8, device=DEV)], ids, ids.numel())


# ---- crop_gaussians ------------------------------------------------------------------------------------------------------------
def node_params(N, seed, centre=(0.0, 0.0, 0.0)):
    g = torch.Generator().manual_seed(seed)
    P = {"means": torch.randn(N, 3, generator=g) * 5 + torch.tensor(centre), "scales": torch.randn(N, 3, generator=g) - 2,
         "quats": torch.randn(N, 4, generator=g), "opacities": torch.randn(N, 1, generator=g),
         "features_dc": torch.randn(N, 3, generator=g) * 0.7, "features_rest": torch.randn(N, 15, 3, generator=g) * 0.2}
    return {k: v.to(DEV) for k, v in P.items()}


def assert_same_dict(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if a[k] is None:
            assert b[k] is None, k
        else:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and not a[k].requires_grad, k
            assert torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                               b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k]), k


def test_crop_through_the_collector_equals_crop_of_the_collected(lib):
    """A three-node scene, the second node rigid and posed far outside the box: the kept rows jump across a node boundary and one
    node ends up empty.  crop_gaussians(collect(...)) == collect(..., crop_box=) == the reference's torch indexing, bitwise,
    and a second run gives the same bits."""
    from mtgs_amd.nodes import collect_gaussians
    nodes = [node_params(700, 1), node_params(300, 2), node_params(2500, 3, centre=(4.0, 0.0, -3.0))]
    nodes[1]["instance_quat"] = torch.tensor([0.9, 0.1, -0.3, 0.2], device=DEV)
    nodes[1]["instance_trans"] = torch.tensor([100.0, 0.0, 0.0], device=DEV)
    c2w = torch.eye(4, device=DEV)[None, :3].clone()
    c2w[0, :3, 3] = torch.tensor([0.4, -1.1, 2.3])
    box = OrientedBox.from_params((1.0, 0.5, -1.0), R.RPY, (9.0, 12.0, 7.0))
    with torch.no_grad():
        full = collect_gaussians(nodes, c2w, 3, 3)
        a = crop_gaussians(full, box)
        b = collect_gaussians(nodes, c2w, 3, 3, crop_box=box)
        again = crop_gaussians(full, box)
    keep = box.within(full["means"])
    assert keep.dtype == torch.bool and np.array_equal(keep.cpu().numpy(), R.within_np(full["means"].cpu().numpy(), box.box))
    want = {k: (v[keep] if v is not None else None) for k, v in full.items() if k != "node_table"}
    assert "node_table" in full and "node_table" not in a and set(a) >= {"means", "scales", "quats", "opacities", "rgbs", "model_id"}
    assert_same_dict(a, want)
    assert_same_dict(b, want)
    assert_same_dict(again, a)
    per_node = [int((a["model_id"] == i).sum()) for i in range(3)]
    print(f"kept per node {per_node} of [700, 300, 2500]")
    assert per_node[1] == 0 and 0 < per_node[0] < 700 and 0 < per_node[2] < 2500 and a["model_id"].dtype == full["model_id"].dtype
    # with grad enabled the collected tensors carry a graph: refused, and so through the collector
    for nd in nodes:
        nd["means"].requires_grad_(True)
    with pytest.raises(ValueError, match="evaluation"):
        collect_gaussians(nodes, c2w, 3, 3, crop_box=box)


def test_crop_through_the_checkpoint_collector(lib):
    """mtgs_amd.checkpoint.collect_gaussians(..., crop_box=) == crop_gaussians of its uncropped result == torch indexing, bitwise:
    two vanilla nodes and a rigid one with a static pose that puts it outside the box"""
    from mtgs_amd import checkpoint as ck
    cpu = lambda d: {k: v.cpu() for k, v in d.items()}
    nodes = {"background": cpu(node_params(900, 11)), "object_vehicle_3": cpu(node_params(200, 12)), "road": cpu(node_params(1300, 13))}
    nodes["object_vehicle_3"]["instance_quats"] = torch.tensor([0.9, 0.1, -0.3, 0.2])
    nodes["object_vehicle_3"]["instance_trans"] = torch.tensor([0.0, 80.0, 0.0])
    c2w = torch.eye(4)[None, :3].clone()
    box = OrientedBox.from_params((1.0, 0.5, -1.0), R.RPY, (9.0, 12.0, 7.0))
    with torch.no_grad():
        full = ck.collect_gaussians(nodes, c2w, 3)
        got = ck.collect_gaussians(nodes, c2w, 3, crop_box=box)
        want = crop_gaussians(full, box)
    keep = box.within(full["means"])
    assert_same_dict(got, want)
    assert_same_dict(got, {k: (v[keep] if v is not None else None) for k, v in full.items() if k != "node_table"})
    per_node = [int((got["model_id"] == i).sum()) for i in range(3)]
    assert per_node[1] == 0 and 0 < per_node[0] < 900 and 0 < per_node[2] < 1300, per_node


def test_crop_of_the_parameter_dictionary_and_of_an_empty_result(lib):
    """the get_gaussian_params shape (features_dc / features_rest, int64 model_id), None entries, a box that keeps nothing, N = 0"""
    P = node_params(4097, 7)
    P["model_id"] = torch.arange(4097, device=DEV) // 1000
    P["rgbs"], P["sh_degree"] = None, 3
    box = OrientedBox.from_params((0.0, 0.0, 0.0), (0.0, 0.0, 0.4), (8.0, 8.0, 8.0))
    got = crop_gaussians(P, box)
    keep = torch.tensor(R.within_np(P["means"].cpu().numpy(), box.box), device=DEV)
    assert 100 < int(keep.sum()) < 4000 and got["rgbs"] is None and got["sh_degree"] == 3
    assert_same_dict({k: v for k, v in got.items() if k != "sh_degree"},
                     {k: (v[keep] if v is not None else None) for k, v in P.items() if k != "sh_degree"})
    nothing = crop_gaussians(P, OrientedBox.from_params((500.0, 0.0, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)))
    empty = crop_gaussians({k: (v[:0] if isinstance(v, torch.Tensor) else v) for k, v in P.items()}, box)
    for out in (nothing, empty):
        for k, v in P.items():
            if isinstance(v, torch.Tensor):
                assert out[k].shape == (0,) + tuple(v.shape[1:]) and out[k].dtype == v.dtype, k


@pytest.mark.parametrize("cell", ["3DGS.py", "MTGS.py"])
def test_render_of_the_cropped_set_is_the_render_of_the_indexed_set(lib, cell):
    """100x70 (partial tiles), the two shipped option cells: RGB + expected depth, classic (3DGS.py); RGB + normals + expected depth,
    antialiased (MTGS.py).  The compacted tensors are the torch-indexed ones bit for bit and in the same order, so render, alpha
    and radii are torch.equal."""
    import mtgs_amd
    mtgs = cell == "MTGS.py"
    W, H, D = 100, 70, (6 if mtgs else 3)
    sc, vm, K = small_scene(N=3000, W=W, H=H, D=D)
    gs = {k: v.to(DEV) for k, v in sc.items()}
    box = OrientedBox.from_params((0.5, 0.0, 3.0), R.RPY, (5.0, 3.0, 3.0))
    keep = box.within(gs["means"])
    assert 300 < int(keep.sum()) < 2700

    def render(d):
        with torch.no_grad():
            r, a, info = mtgs_amd.rasterization(d["means"], d["quats"], d["scales"], d["opacities"], d["colors"], vm.to(DEV), K.to(DEV),
                                                W, H, packed=False, render_mode="RGB+ED", absgrad=mtgs,
                                                rasterize_mode="antialiased" if mtgs else "classic")
        return r, a, info["radii"]
    cropped = crop_gaussians(gs, box)
    assert cropped["means"].shape[0] == int(keep.sum())
    got, want = render(cropped), render({k: v[keep] for k, v in gs.items()})
    assert int((want[2] > 0).sum()) > 20 and float(want[1].max()) > 0.0        # something is on screen
    for g, w, name in zip(got, want, ("render", "alpha", "radii")):
        assert torch.equal(g, w), name
    again = render(crop_gaussians(gs, box))
    for g, w in zip(again, got):
        assert torch.equal(g, w)
