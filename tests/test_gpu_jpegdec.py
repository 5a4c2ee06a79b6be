"""mtgs_amd.jpegdec on the device (csrc/jpegdec.hip): every pixel is compared EXACTLY with tests/jpegdec_refs.py, the NumPy decoder
that tests/test_jpegdec_host.py pins to Pillow, and with Pillow's own pixels in tests/golden/jpegdec_pillow.npz."""
import numpy as np
import pytest
import torch

import mtgs_amd
from mtgs_amd import jpegdec as J
from tests import jpeg_refs as R
from tests import jpegdec_refs as D

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = D.golden()


def check(data, want=None, what="", **kw):
    """decodes `data` on the device; the pixels equal the model's (and `want`), the status is clean and complete.  Returns the status."""
    model = D.decode(data)
    got, status = mtgs_amd.decode_jpeg(data, return_status=True, **kw)
    status = status.cpu().tolist()
    got = got.cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == model.shape, what
    if not np.array_equal(got, model):
        bad = np.argwhere(got != model)
        raise AssertionError(f"{what}: {len(bad)} values differ from the model, the first at {tuple(bad[0])}: {got[tuple(bad[0])]} against "
                             f"{model[tuple(bad[0])]}; status {status}")
    assert want is None or np.array_equal(got, want), f"{what}: differs from Pillow's pixels"
    f = D.read(data)
    assert status[0] == 0 and status[1] == status[2] == f.n_blocks, (what, status)
    return status


# ---- the shape and option grid ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h, w", D.SIZES, ids=lambda v: str(v))
def test_the_grid_equals_the_model_and_pillows_pixels(h, w):
    """every size in 4:4:4 / 4:2:2 / 4:2:0 at qualities 1, 75 and 100 over the five image kinds: Pillow's files and pixels of the
    fixture; and where the NumPy encoder writes the file (it has no 4:2:2), its bytes are Pillow's and decode alike"""
    cells = {f"grid/{kind}/{h}x{w}/{q}/{s}" for kind in D.KINDS for q in D.QUALITIES for s in ("444", "422", "420")}
    assert len(cells) == 45 and cells <= set(GOLDEN)
    for name in sorted(cells):
        check(*GOLDEN[name], what=name)
    for kind in D.KINDS:
        for q in D.QUALITIES:
            for s in R.SUBSAMPLINGS:
                assert R.encode(D.image_of(kind, h, w), q, s) == GOLDEN[f"grid/{kind}/{h}x{w}/{q}/{s.replace(':', '')}"][0]


@pytest.mark.parametrize("h, w", D.NARROW, ids=lambda v: str(v))
def test_chroma_one_or_two_samples_wide_is_replicated(h, w):
    """libjpeg interpolates only a component wider than two samples: at these sizes Pillow's pixels are NOT what the fancy rule
    gives for 4:2:2 and 4:2:0, and the device equals Pillow"""
    names = [n for n in GOLDEN if n.startswith("narrow/") and n.split("/")[2] == f"{h}x{w}"]
    assert len(names) == 12
    differ = 0
    for name in names:
        data, want = GOLDEN[name]
        check(data, want, name)
        f = D.read(data)
        if f.hs == 2:
            coef = D.coefficients(f)
            fancy = D.pixels(f, coef, replicate_narrow=False)
            differ += int(not np.array_equal(fancy, want))
    for kind in ("noise", "ramp"):
        check(R.encode(D.image_of(kind, h, w), 75, "4:2:0"), GOLDEN[f"narrow/{kind}/{h}x{w}/75/420"][1], f"encoder's {kind} {h}x{w}")
    assert differ, "the fancy rule gives the same pixels here: the case decides nothing"


def test_a_flat_image_completes_many_blocks_in_one_subsequence():
    for name in ("grid/constant/48x65/75/444", "grid/constant/48x65/75/420", "grid/constant/31x50/75/422"):
        data, want = GOLDEN[name]
        check(data, want, name)
        check(data, want, name, subsequence_bits=1024)
    f = D.read(GOLDEN["grid/constant/48x65/75/444"][0])
    begin, end, _ = D.subsequences(f, 1024)[0]
    assert D.run(f, (begin, 0, 0), end)[1] > 100                # six bits per block


def test_optimised_tables_restart_markers_and_stuffed_bytes():
    names = [n for n in GOLDEN if n.startswith("opt/")]
    assert len(names) == 12
    for name in names:
        for bits in (None, 64):
            check(*GOLDEN[name], what=name, subsequence_bits=bits)
    for name, intervals in (("opt/rmb1/31x50/75/444", 28), ("opt/rmb1/48x65/75/420", 15), ("opt/rmb3/31x50/75/444", 10)):
        f = D.read(GOLDEN[name][0])
        assert f.n_int == intervals > 8                          # the marker number wraps
        assert sorted(set(f.scan[k + 1] for k in range(len(f.scan) - 1) if f.scan[k] == 0xFF and f.scan[k + 1] != 0)) == list(range(0xD0, 0xD8))
    stuffed = GOLDEN["grid/noise/48x65/100/444"][0]
    assert D.read(stuffed).scan.count(b"\xff\x00") > 20
    check(*GOLDEN["grid/noise/48x65/100/444"], what="noise at quality 100", subsequence_bits=32)


# ---- synchronisation ----------------------------------------------------------------------------------------------------------------
def test_the_serial_worst_case_and_a_stream_of_several_workgroups():
    data, want = GOLDEN["worst"]
    f = D.read(data)
    for bits in (256, 1024):
        assert D.steps(f, bits) == len(D.subsequences(f, bits))             # it never synchronises
        status = check(data, want, f"worst {bits}", subsequence_bits=bits)
        assert status[3] == 1                                               # one workgroup: one launch did all the work
    image = R.images("noise", 264, 200, seed=7)
    big = R.encode(image, 75, "4:4:4")
    assert len(big) > 60_000
    launches = {}
    for bits in (None, 256, 32):
        launches[bits] = check(big, what=f"264 x 200 noise {bits}", subsequence_bits=bits)[3]
    n_sub = len(D.subsequences(D.read(big), 256))
    assert n_sub > 4 * J.RUN                                                # several workgroup runs
    # a launch after the first changed something: the second level did real work
    assert launches[256] >= 2 and launches[32] >= 2, launches


# ---- both input forms, and the plumbing -----------------------------------------------------------------------------------------------
def test_every_input_form_gives_the_same_pixels():
    data, want = GOLDEN["grid/noise/31x50/75/420"]
    jpeg = mtgs_amd.upload_jpeg(data)
    assert isinstance(jpeg, J.DeviceJpeg) and jpeg.scan.is_cuda and jpeg.tables.is_cuda and jpeg.info.scan_length == jpeg.scan.numel()
    array = np.frombuffer(data, dtype=np.uint8)
    for source in (data, bytearray(data), array, torch.from_numpy(array.copy()), jpeg, jpeg):
        assert np.array_equal(mtgs_amd.decode_jpeg(source).cpu().numpy(), want)


def test_out_with_strides_and_image_float():
    data, want = GOLDEN["grid/noise/31x50/75/422"]
    h, w = want.shape[:2]
    big = torch.full((h + 3, 2 * w + 5, 4), 77, dtype=torch.uint8, device=DEV)
    view = big[2:2 + h, 1:1 + 2 * w:2, 1:4]
    assert mtgs_amd.decode_jpeg(data, out=view) is view and not view.is_contiguous()
    assert np.array_equal(view.cpu().numpy(), want)
    view.fill_(77)
    assert bool((big == 77).all())                                          # nothing beside the view was written
    as_float = mtgs_amd.decode_jpeg(data, image_float=True)
    assert as_float.dtype == torch.float32
    expect = want.astype(np.float32) / np.float32(255)                      # one correctly rounded division
    assert np.array_equal(as_float.cpu().numpy().view(np.uint32), expect.view(np.uint32))
    planes = torch.empty((3, h, w), dtype=torch.float32, device=DEV).permute(1, 2, 0)
    mtgs_amd.decode_jpeg(data, image_float=True, out=planes)
    assert np.array_equal(planes.cpu().numpy().view(np.uint32), expect.view(np.uint32))
    with pytest.raises(ValueError, match="out must be"):
        mtgs_amd.decode_jpeg(data, out=torch.empty((h, w, 3), dtype=torch.float32, device=DEV))


def test_a_second_smaller_file_in_the_same_buffers_and_no_host_read():
    first, second = GOLDEN["grid/noise/48x65/100/444"], GOLDEN["grid/ramp/48x65/1/444"]
    assert len(second[0]) < len(first[0]) // 4
    a, b = mtgs_amd.upload_jpeg(first[0]), mtgs_amd.upload_jpeg(second[0])
    workspace = torch.empty(max(J.sizes(a.info), J.sizes(b.info)), dtype=torch.uint8, device=DEV)
    out = torch.empty((48, 65, 3), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    allocations = lambda: torch.cuda.memory_stats()["allocation.all.allocated"]
    before = allocations()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = []
        for jpeg in (a, b, a):
            assert mtgs_amd.decode_jpeg(jpeg, out=out, workspace=workspace) is out
            got.append(out.clone() if jpeg is not a else None)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert allocations() == before + 1                                      # the one clone, nothing for the decodes
    assert np.array_equal(got[1].cpu().numpy(), second[1]) and np.array_equal(out.cpu().numpy(), first[1])
    _, status = mtgs_amd.decode_jpeg(b, out=out, workspace=workspace, return_status=True)
    assert status.data_ptr() == workspace.data_ptr() and status.cpu().tolist()[:3] == [0, 54 * 3, 54 * 3]
    assert np.array_equal(out.cpu().numpy(), second[1])
    with pytest.raises(RuntimeError, match="workspace"):
        mtgs_amd.decode_jpeg(a, workspace=workspace[:1024])


# ---- round trip -----------------------------------------------------------------------------------------------------------------------
def test_decoding_what_the_device_encoder_wrote():
    for kind, s, q in (("noise", "4:2:0", 75), ("ramp", "4:4:4", 95), ("blocks", "4:2:0", 40)):
        image = torch.from_numpy(R.images(kind, 40, 57, seed=3)).to(DEV)
        data = mtgs_amd.encode_jpeg(image, q, s).tobytes()
        assert np.array_equal(mtgs_amd.decode_jpeg(data).cpu().numpy(), D.decode(data)), (kind, s, q)


def test_live_pillow_decodes_the_same_pixels(tmp_path):
    Image = pytest.importorskip("PIL.Image", reason="Pillow is not installed")
    image = R.images("noise", 100, 131, seed=12)
    for kw in (dict(quality=75), dict(quality=95, subsampling=0), dict(quality=85, subsampling=1, optimize=True),
               dict(quality=60, restart_marker_rows=1)):
        Image.fromarray(image).save(tmp_path / "x.jpg", "JPEG", **kw)
        data = (tmp_path / "x.jpg").read_bytes()
        assert np.array_equal(mtgs_amd.decode_jpeg(data).cpu().numpy(), np.array(Image.open(tmp_path / "x.jpg"))), kw
