"""The oriented crop box (mtgs_amd/crop.py, csrc/crop.hip) without a GPU: how the box is built, the decision of
`OrientedBox.within` on the host at its edges and against the stated fp32 formula, the recalled nerfstudio semantics, the C
entry points and their host-side argument checks, and what `crop_gaussians` refuses.

nerfstudio 1.1.5 (OrientedBox.within, OrientedBox.from_params) is not part of the reference tree: the two facts recalled from it
are isolated in mtgs_amd.crop._inside (strict comparisons against +-S / 2 in box coordinates) and mtgs_amd.crop._rpy_matrix
(R = Rz(yaw) Ry(pitch) Rx(roll)), and each has one test here: test_within_agrees_with_the_nerfstudio_shaped_evaluation and
test_from_params_is_rz_ry_rx."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from mtgs_amd.crop import OrientedBox, crop_gaussians
from tests import crop_refs as R

N_RANDOM = 100_000
FACE_BAND = 1e-4        # decisions may differ from the fp32-inverse evaluation only this close to a face (fp64 box coordinates)
MAX_IN_BAND = 1e-4      # and at most this share of the points may be that close


# ---- from_params ------------------------------------------------------------------------------------------------------------
def closed_form_rz_ry_rx(roll, pitch, yaw):
    """Rz(yaw) Ry(pitch) Rx(roll) multiplied out by hand, fp64"""
    cr, sr, cp, sp, cy, sy = math.cos(roll), math.sin(roll), math.cos(pitch), math.sin(pitch), math.cos(yaw), math.sin(yaw)
    return np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                     [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                     [-sp, cp * sr, cp * cr]])


@pytest.mark.parametrize("rpy, images", [
    ((math.pi / 2, 0.0, 0.0), ([1, 0, 0], [0, 0, 1], [0, -1, 0])),     # roll about x: y -> z, z -> -y
    ((0.0, math.pi / 2, 0.0), ([0, 0, -1], [0, 1, 0], [1, 0, 0])),     # pitch about y: x -> -z, z -> x
    ((0.0, 0.0, math.pi / 2), ([0, 1, 0], [-1, 0, 0], [0, 0, 1])),     # yaw about z: x -> y, y -> -x
])
def test_from_params_moves_the_unit_axes(rpy, images):
    box = OrientedBox.from_params((0.0, 0.0, 0.0), rpy, (1.0, 1.0, 1.0))
    assert box.R.dtype == np.float64
    for axis, image in enumerate(images):
        assert np.allclose(box.R[:, axis], image, rtol=0, atol=1e-15), (rpy, axis, box.R[:, axis])


def test_from_params_is_rz_ry_rx():
    """[NS-RECALL] the rpy order.  A general triple: the three rotations do not commute, so any other order fails."""
    for rpy in (R.RPY, (-2.4, 1.3, 0.7), (0.1, -1.5, 3.0)):
        box = OrientedBox.from_params(R.POS, rpy, R.SIZE)
        want = closed_form_rz_ry_rx(*rpy)
        assert np.allclose(box.R, want, rtol=0, atol=1e-15), rpy
        assert not np.allclose(box.R, closed_form_rz_ry_rx(*rpy[::-1]), atol=1e-3)
    assert np.array_equal(box.T, np.array(R.POS)) and np.array_equal(box.S, np.array(R.SIZE))


def test_box_accepts_any_float_dtype_and_holds_fp32_for_the_kernel():
    a = OrientedBox(torch.eye(3, dtype=torch.float16), torch.zeros(3, dtype=torch.float64), np.array([2.0, 3.0, 0.75], dtype=np.float32))
    assert a.box.dtype == np.float32 and a.box.shape == (15,)
    assert np.array_equal(a.box, np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1.0, 1.5, 0.375], dtype=np.float32))
    with pytest.raises(ValueError, match="R must be"):
        OrientedBox(torch.eye(4), torch.zeros(3), torch.ones(3))
    # a general inverse, not the transpose: a sheared "rotation" is inverted as nerfstudio inverts H
    shear = np.array([[1.0, 0.5, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    b = OrientedBox(shear, np.array([1.0, 2.0, 3.0]), np.ones(3))
    H = np.eye(4)
    H[:3, :3], H[:3, 3] = shear, [1.0, 2.0, 3.0]
    assert np.array_equal(b.world_to_box, np.linalg.inv(H)[:3].astype(np.float32))
    assert not np.allclose(b.world_to_box[:, :3], shear.T)


# ---- within on the host: the edges ---------------------------------------------------------------------------------------------
SIDES = np.array([2.0, 3.0, 0.75], dtype=np.float32)


def axis_box(sides=SIDES):
    return OrientedBox(np.eye(3), np.zeros(3), sides)


def test_within_is_strict_on_every_face():
    """R = I, T = 0: the box coordinate is the coordinate itself, exactly.  A point on a face is out, its fp32 neighbour towards the
    centre is in."""
    box, half = axis_box(), SIDES / np.float32(2)
    assert bool(box.within(torch.zeros(1, 3))[0])
    for axis in range(3):
        for sign in (1.0, -1.0):
            on = np.zeros((1, 3), dtype=np.float32)
            on[0, axis] = np.float32(sign) * half[axis]
            just_in = on.copy()
            just_in[0, axis] = np.nextafter(on[0, axis], np.float32(0.0))
            just_out = on.copy()
            just_out[0, axis] = np.nextafter(on[0, axis], np.float32(sign * np.inf))
            assert not bool(box.within(torch.from_numpy(on))[0]), (axis, sign)
            assert bool(box.within(torch.from_numpy(just_in))[0]), (axis, sign)
            assert not bool(box.within(torch.from_numpy(just_out))[0]), (axis, sign)
            assert not R.within_np(on, box.box)[0] and R.within_np(just_in, box.box)[0]


def test_within_drops_nan_and_inf_and_an_empty_box_keeps_nothing():
    box = axis_box()
    bad = torch.zeros(9, 3)
    for axis in range(3):
        bad[3 * axis, axis], bad[3 * axis + 1, axis], bad[3 * axis + 2, axis] = float("nan"), float("inf"), float("-inf")
    got = box.within(bad)
    assert got.dtype == torch.bool and got.shape == (9,) and not bool(got.any())
    assert not R.within_np(bad.numpy(), box.box).any()
    pts = torch.from_numpy(np.concatenate([np.zeros((1, 3), dtype=np.float32), R.random_points(1000)]).copy())
    assert not bool(axis_box(np.zeros(3, dtype=np.float32)).within(pts).any())
    flat = axis_box(np.array([2.0, 0.0, 2.0], dtype=np.float32))                  # one zero side is enough
    assert not bool(flat.within(pts).any())
    assert box.within(torch.zeros(0, 3)).shape == (0,)
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        box.within(torch.zeros(5, 4))


# ---- within on the host: the formula and the recalled semantics -----------------------------------------------------------------
def test_within_equals_the_numpy_fp32_formula_exactly():
    box, pts = R.random_box(), R.random_points(N_RANDOM)
    got = box.within(torch.tensor(pts)).numpy()
    want = R.within_np(pts, box.box)
    kept = int(want.sum())
    print(f"kept {kept} of {N_RANDOM}")
    assert 0.01 * N_RANDOM < kept < 0.5 * N_RANDOM
    assert np.array_equal(got, want)
    # a [N, 4][:, :3] view and a float64 tensor of the same values give the same decisions
    wide = torch.zeros(N_RANDOM, 4)
    wide[:, :3] = torch.tensor(pts)
    assert np.array_equal(box.within(wide[:, :3]).numpy(), want)
    assert np.array_equal(box.within(torch.tensor(pts).double()).numpy(), want)


def nerfstudio_within(R_, T_, S_, pts):
    """[NS-RECALL] OrientedBox.within as nerfstudio 1.1.5 evaluates it, written out: H = [[R, T], [0, 1]] and its inverse in
    fp32, homogeneous points through it, strict comparisons against -S / 2 and S / 2."""
    Rm, T, S = (torch.as_tensor(a, dtype=torch.float32) for a in (R_, T_, S_))
    H = torch.eye(4)
    H[:3, :3], H[:3, 3] = Rm, T
    H_world2bbox = torch.inverse(H)
    p = torch.cat((pts, torch.ones_like(pts[..., :1])), dim=-1)
    p = torch.matmul(H_world2bbox, p.T).T[..., :3]
    comp_l, comp_m = -S / 2, S / 2
    return torch.all(torch.cat([p > comp_l, p < comp_m], dim=-1), dim=-1)


def test_within_agrees_with_the_nerfstudio_shaped_evaluation():
    """[NS-RECALL] the strict comparisons against +-S / 2 in box coordinates.  The two evaluations round differently (an fp32
    inverse and a matmul there, an fp64 inverse rounded once and a fixed order here), so they may differ at points within
    FACE_BAND of a face in exact (fp64) box coordinates; nowhere else, and that band holds at most MAX_IN_BAND of the points."""
    box, pts = R.random_box(), R.random_points(N_RANDOM)
    ours = box.within(torch.tensor(pts)).numpy()
    theirs = nerfstudio_within(box.R, box.T, box.S, torch.tensor(pts)).numpy()
    H = np.eye(4)
    H[:3, :3], H[:3, 3] = box.R, box.T
    inv = np.linalg.inv(H)
    q64 = pts.astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]
    near = (np.abs(np.abs(q64) - box.S / 2) <= FACE_BAND).any(axis=1)
    m, h = box.box[:12].reshape(3, 4), box.box[12:]
    q32 = ((m[:, 0] * pts[:, 0:1] + m[:, 1] * pts[:, 1:2]) + m[:, 2] * pts[:, 2:3]) + m[:, 3]
    differ = ours != theirs
    print(f"fp32 coordinate error {np.abs(q32 - q64).max():.2e}; {int(near.sum())} of {N_RANDOM} points within {FACE_BAND} of a face; "
          f"{int(differ.sum())} decisions differ, {int((differ & ~near).sum())} of them outside the band")
    assert np.array_equal(h.astype(np.float64), box.S / 2)
    assert near.mean() <= MAX_IN_BAND
    assert not (differ & ~near).any()
    assert np.array_equal(ours[~near], ((q64 > -box.S / 2) & (q64 < box.S / 2)).all(axis=1)[~near])     # and both are the exact answer there


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_and_bound():
    """The crop block is include/mtgs_crop.h, a group of its own (tests/test_abi.py checks every group against its header, its
    reviewed record tests/golden/abi_signatures_crop.txt and the library): these are its entry points."""
    from mtgs_amd import _lib
    assert sorted(_lib.GROUPS["mtgs_crop.h"]) == ["mtgs_crop_gather", "mtgs_crop_select", "mtgs_crop_workspace_bytes"]


def test_host_side_argument_checks(hip_lib):
    """Every refusal happens before a launch and names the argument (nothing here needs a device: the pointers are never followed)."""
    err = lambda: hip_lib.mtgs_rast_last_error().decode()
    n = C.c_size_t(0)
    assert hip_lib.mtgs_crop_workspace_bytes(1 << 20, C.byref(n)) == 0 and n.value == 8 * ((1 << 20) // 2048 + 1)
    assert hip_lib.mtgs_crop_workspace_bytes(0, C.byref(n)) == 0 and n.value == 8
    assert hip_lib.mtgs_crop_workspace_bytes(1 << 31, C.byref(n)) == 1 and "N outside" in err()
    assert hip_lib.mtgs_crop_workspace_bytes(5, None) == 1 and "bytes" in err()
    buf = (C.c_int64 * 64)()
    a = C.addressof(buf)                                   # a non-null, 8-byte aligned address
    box = (C.c_float * 15)()
    select = lambda N=100, means=a, stride=3, bx=box, ids=a, count=a, mask=None, ws=a, ws_bytes=1 << 20: \
        hip_lib.mtgs_crop_select(N, means, stride, bx, ids, count, mask, ws, ws_bytes, None)
    for kw, word in (({"means": None}, "means"), ({"bx": None}, "box"), ({"ids": None}, "keep_ids"), ({"count": None}, "count"),
                     ({"ws": None}, "ws")):
        assert select(**kw) == 1 and f"null pointer: {word}" in err(), kw
    assert select(stride=2) == 1 and "row_stride < 3" in err()
    assert select(N=-1) == 1 and "N outside" in err()
    assert select(N=5000, ws_bytes=31) == 3 and "workspace 31 < 32 bytes" in err()
    assert select(count=a + 4) == 1 and "count must be 8-byte aligned" in err()
    src, dst, rb = (C.c_uint64 * 17)(*([a] * 17)), (C.c_uint64 * 17)(*([a] * 17)), (C.c_int64 * 17)(*([12] * 17))
    gather = lambda n_keep=10, n_rows=100, ids=a, n=1, s=src, d=dst, r=rb: hip_lib.mtgs_crop_gather(n_keep, n_rows, ids, n, s, d, r, None)
    assert gather(n=0) == 1 and "n_tensors outside [1, 16] (0)" in err()
    assert gather(n=17) == 1 and "n_tensors outside [1, 16] (17)" in err()
    for kw, word in (({"s": None}, "src"), ({"d": None}, "dst"), ({"r": None}, "row_bytes"), ({"ids": None}, "keep_ids")):
        assert gather(**kw) == 1 and f"null pointer: {word}" in err(), kw
    for bad in (6, 0, -4):
        rb[2] = bad
        assert gather(n=3) == 1 and f"row_bytes[2] must be a multiple of 4 in [4, 2^30] ({bad})" in err()
    rb[2] = 12
    assert gather(n_keep=101) == 1 and "n_keep 101 > n_rows 100" in err()
    src[1] = 0
    assert gather(n=2) == 1 and "null pointer: src[1]" in err()
    src[1], dst[0] = a, a + 2
    assert gather(n=2) == 1 and "4-byte aligned" in err()
    assert gather(n_keep=0, ids=None) == 0                  # nothing kept: a no-op, whatever the table points to


# ---- crop_gaussians: what it refuses (before it touches a device) ---------------------------------------------------------------
def test_crop_gaussians_refuses_deferred_colours_and_graphs():
    box = R.random_box()
    gs = {"means": torch.zeros(4, 3), "scales": torch.ones(4, 3), "rgbs": None, "color_source": object()}
    with pytest.raises(NotImplementedError, match="deferred_colors"):
        crop_gaussians(gs, box)
    gs = {"means": torch.zeros(4, 3), "scales": torch.ones(4, 3, requires_grad=True)}
    with pytest.raises(ValueError, match=r"\['scales'\] require grad.*evaluation"):
        crop_gaussians(gs, box)
    with torch.no_grad(), pytest.raises(RuntimeError, match="HIP device"):     # past the two refusals: only the device is missing
        crop_gaussians(gs, box)


def test_collectors_refuse_a_crop_with_deferred_colours_before_anything_runs():
    from mtgs_amd.nodes import collect_gaussians
    with pytest.raises(NotImplementedError, match="deferred_colors"):
        collect_gaussians([], torch.eye(4)[None, :3], 3, deferred_colors=True, crop_box=R.random_box())
