"""The shared input normalisation (mtgs_amd/_inputs.py) without a GPU: which layouts of point rows are read in place and which are
copied, the dtypes, and the refusals."""
import pytest
import torch

from mtgs_amd._inputs import point_rows, row_stride, shape_of

FLOATS = (torch.float32, torch.float64)


@pytest.mark.parametrize("N", [0, 1, 2])
def test_a_row_stride_is_kept(N):
    """[N, 4][:, :3]: the coordinates are adjacent, the rows four elements apart"""
    wide = torch.arange(4.0 * N).reshape(N, 4)
    p = point_rows(wide[:, :3])
    assert p.data_ptr() == wide.data_ptr() and tuple(p.shape) == (N, 3) and p.stride(1) == 1
    assert row_stride(p) == (4 if N == 2 else 3)
    assert N < 2 or p.stride(0) == 4


@pytest.mark.parametrize("N", [1, 2])
def test_a_column_stride_is_copied_whatever_the_row_count(N):
    """[N, 6][:, ::2]: one row has no row stride to tell the layout by, and is copied like two"""
    wide = torch.arange(6.0 * N).reshape(N, 6)
    view = wide[:, ::2]
    assert view.stride(1) == 2
    p = point_rows(view)
    assert p.data_ptr() != wide.data_ptr() and p.is_contiguous() and torch.equal(p, view) and row_stride(p) == 3
    assert p[0].tolist() == [0.0, 2.0, 4.0]


def test_overlapping_rows_are_copied():
    row = torch.tensor([[1.0, 2.0, 3.0]])
    view = row.expand(4, 3)
    assert view.stride(0) == 0
    p = point_rows(view)
    assert p.is_contiguous() and p.data_ptr() != row.data_ptr() and torch.equal(p, view) and row_stride(p) == 3


def test_dtypes():
    x64 = (torch.arange(8.0, dtype=torch.float64).reshape(2, 4) + 1e-9)[:, :3]
    p = point_rows(x64)                                         # seed, crop, pointcloud: float32 rows
    assert p.dtype == torch.float32 and torch.equal(p, x64.to(torch.float32)) and p.is_contiguous()
    q = point_rows(x64, FLOATS, convert=False)                  # lidar: float32 or float64, as they come
    assert q.dtype == torch.float64 and q.data_ptr() == x64.data_ptr() and q.stride(0) == 4
    r = point_rows(x64.to(torch.float32), FLOATS, convert=False)
    assert r.dtype == torch.float32
    strided = torch.arange(12.0, dtype=torch.float64).reshape(2, 6)[:1, ::2]
    assert point_rows(strided, FLOATS, convert=False).dtype == torch.float64 and point_rows(strided, FLOATS, convert=False).is_contiguous()
    assert not point_rows(torch.zeros(2, 3, requires_grad=True)).requires_grad
    with pytest.raises(TypeError, match=r"points must be float32 or float64, got torch\.float16"):
        point_rows(torch.zeros(2, 3, dtype=torch.float16), FLOATS, convert=False)
    with pytest.raises(TypeError, match=r"points must be float32 or float64, got torch\.int64"):
        point_rows(torch.zeros(2, 3, dtype=torch.int64), FLOATS, convert=False)


@pytest.mark.parametrize("bad, got", [(torch.zeros(3), r"\(3,\)"), (torch.zeros(2, 4), r"\(2, 4\)"), (torch.zeros(1, 2, 3), r"\(1, 2, 3\)"),
                                      ([[0.0, 0.0, 0.0]], "list"), (None, "NoneType")])
def test_shapes_are_refused(bad, got):
    with pytest.raises(ValueError, match=r"points must be \[N, 3\], got " + got):
        point_rows(bad)
    with pytest.raises(ValueError, match=r"points must be \[N, 3\], got " + got):
        point_rows(bad, FLOATS, convert=False)


def test_the_operators_take_the_shared_rows():
    """seed, pointcloud, crop and lidar have no copies of their own"""
    from mtgs_amd import crop, lidar, pointcloud, seed
    for module in (crop, lidar, pointcloud, seed):
        assert module.point_rows is point_rows and not hasattr(module, "_points")
    with pytest.raises(ValueError, match=r"points must be \[N, 3\], got \(2, 4\)"):
        lidar.depth_image(torch.zeros(2, 4), torch.eye(4), torch.eye(3), 4, 4)
    with pytest.raises(TypeError, match="points must be float32 or float64, got torch.float16"):
        lidar.depth_image(torch.zeros(2, 3, dtype=torch.float16), torch.eye(4), torch.eye(3), 4, 4)
    assert shape_of(torch.zeros(2, 3)) == "(2, 3)" and shape_of(3) == "int"
