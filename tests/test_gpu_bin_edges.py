"""The stages of the depth-ordered binning (csrc/bin.hip, isect.hip, scan.hpp, radix_sort.hpp, tile_schedule_kernel of blend.hip)
called directly through the C ABI at the sizes where they branch, against the numpy references of tests/bin_refs.py.  Integer and
bit-pattern work only: every comparison is np.array_equal / torch.equal, there is no tolerance in this file.

The canary rule holds for every call: every output is allocated with slack behind it and pre-filled with one bit pattern; a
test asserts what was written AND that everything else still holds the pattern.  Workspaces are scratch: only the bytes behind
the size the library asks for are checked.

Where the code branches (and which test goes there):
  * mtgs_scan::spine_kernel takes a second round above 256 blocks x 2048 elements      -> n = 524 288 / 524 289 / 526 337
  * mtgs_bin_compact: 16-byte loads when radii and tiles_per_gauss are 16-byte aligned, the generic scan otherwise
                                                                                         -> `[1:]` views (the only misaligned inputs here)
  * mtgs_bin_compact packs n_vis << 32 | M into one int64                               -> tile counts summing to 2^32 - 1
  * bin_emit_kernel: 256-ary search (step rounding at n_vis = 256, 65 536), a 2048-entry window that is exactly full when
    every Gaussian owns one tile, cum[pos] <= s0 at a block boundary on a Gaussian boundary, and the global-memory search for
    slots behind 2048 or more entries WITHOUT a tile                                    -> the scenes of bin_refs.SCENES
  * mtgs_bin_sort_tiles: 1, 2 or 3 passes as C * n_tiles crosses 256 and 65 536, the ping-pong parity with it, the id epilogue
    in the last pass only, bit_length(n_tiles) tile bits                                -> SORT_TILES_GRIDS
  * isect_offsets_kernel: one thread fills every empty tile between two entries, the last one the tail
  * tile_schedule_kernel: never visible in a render."""
import numpy as np
import pytest
import torch

from tests import bin_refs as R

pytestmark = pytest.mark.gpu

CAN = 0x5AC0DE5A                                         # every int32 word of every output before the call
CAN64 = (CAN << 32) | CAN
SL = 5                                                   # slack elements behind every output
WS_FILL, WS_SLACK = 0xA5, 64


# ---- device helpers ---------------------------------------------------------------------------------------------------------------
def _call(name, *a):
    from mtgs_amd import _lib
    _lib.call(name, *a)


def _st():
    return torch.cuda.current_stream().cuda_stream


def can(n):
    return torch.full((int(n),), CAN, dtype=torch.int32, device="cuda")


def can64(n):
    return can(2 * int(n)).view(torch.int64)


def up(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def host(t):
    return t.detach().cpu().numpy()


def shifted(a, by):
    """The array on the device, `by` 4-byte elements behind a 16-byte boundary (a `[by:]` view)."""
    a = np.ascontiguousarray(a)
    t = up(np.concatenate([np.zeros(by, dtype=a.dtype), a]))[by:]
    assert t.data_ptr() % 16 == 4 * by and t.numel() == a.size
    return t


class Ws:
    """A workspace of the size the library asks for, with WS_SLACK bytes behind it that must survive."""

    def __init__(self, query, *dims):
        from mtgs_amd import _lib
        self.size = _lib.size_query(query, *dims)
        self.buf = torch.full((self.size + WS_SLACK,), WS_FILL, dtype=torch.uint8, device="cuda")
        self.ptr = self.buf.data_ptr()

    def intact(self):
        return bool((self.buf[self.size:] == WS_FILL).all())


def written(t, n, want):
    """t[:n] equals want and everything behind is canary."""
    h = host(t)
    fill = CAN64 if h.dtype == np.int64 else CAN
    want = np.asarray(want)
    if want.dtype == np.uint32:
        want = want.view(np.int32)
    return h[:n].dtype == want.dtype and np.array_equal(h[:n], want) and bool((h[n:] == fill).all()) and h.size > n


def untouched(t):
    h = host(t)
    return bool((h == (CAN64 if h.dtype == np.int64 else CAN)).all())


def scene_ids(keys):
    return ["-".join(str(v) for v in k) for k in keys]


# ---- mtgs_isect_scan ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.SCAN_N)
def test_isect_scan(hip_lib, n):
    """Inclusive int64 sums at one element, around the 8 elements of a thread, around the 2048 of a block and around the 256
    blocks of one spine round; a value set whose total passes 2^32; the total pointer null and non-null."""
    for big in (False, True):
        v = R.scan_values(n, big)
        want = R.scan_inclusive(v)
        assert not (big and n >= 7) or int(want[-1]) > 1 << 32
        dv = up(v)
        for with_total in (True, False):
            cum, tot, w = can64(n + SL), can64(1 + SL), Ws("mtgs_scan_workspace_bytes", n)
            _call("mtgs_isect_scan", n, dv.data_ptr(), cum.data_ptr(), tot.data_ptr() if with_total else None, w.ptr, w.size, _st())
            assert written(cum, n, want), (n, big)
            assert written(tot, 1, want[-1:]) if with_total else untouched(tot), (n, big)
            assert w.intact() and np.array_equal(host(dv), v)


def test_isect_scan_of_nothing(hip_lib):
    cum, tot = can64(SL), can64(1 + SL)
    _call("mtgs_isect_scan", 0, None, cum.data_ptr(), tot.data_ptr(), None, 0, _st())
    _call("mtgs_isect_scan", 0, None, cum.data_ptr(), None, None, 0, _st())
    assert untouched(cum) and written(tot, 1, np.zeros(1, dtype=np.int64))


# ---- mtgs_bin_compact ---------------------------------------------------------------------------------------------------------------
# C * N = every n of the scan test as (1, n) and (n, 1); three cameras: N = n / 3 rounded down and up where that is no power of two
COMPACT_SHAPES = [(1, n) for n in R.SCAN_N] + [(3, N) for N in (3, 682, 683, 174762, 174763, 175445, 175446)] + [(n, 1) for n in R.SCAN_N if n > 1]


def run_compact(C, N, radii, depths, tpg, by, tag, rank=True, mailbox=True):
    n = C * N
    keys, ids, rk, packed = R.compact(radii, depths, tpg, N)
    n_vis = ids.size
    d_r, d_t, d_d = shifted(radii, by), shifted(tpg, by), up(depths)
    assert d_r.data_ptr() % 16 == d_t.data_ptr() % 16 == 4 * by
    vk, vi, vr, tot = can64(n + SL), can(n + SL), can(n + SL), can64(1 + SL)
    mb = torch.full((2 + SL,), CAN64, dtype=torch.int64).pin_memory()
    w = Ws("mtgs_scan_workspace_bytes", n)
    _call("mtgs_bin_compact", C, N, d_r.data_ptr(), d_d.data_ptr(), d_t.data_ptr(), vk.data_ptr(), vi.data_ptr(),
          vr.data_ptr() if rank else None, tot.data_ptr(), mb.data_ptr() if mailbox else None, tag, w.ptr, w.size, _st())
    torch.cuda.current_stream().synchronize()
    m = mb.numpy()
    what = (C, N, by, tag)
    if mailbox:
        assert int(m[0]) == packed and int(m[1]) == tag and (m[2:] == CAN64).all(), what
    else:
        assert (m == CAN64).all(), what
    assert written(tot, 1, np.array([packed], dtype=np.int64)), what
    assert written(vk, n_vis, keys) and written(vi, n_vis, ids), what
    assert written(vr, n, np.where(rk >= 0, rk, CAN).astype(np.int32)) if rank else untouched(vr), what
    assert w.intact() and np.array_equal(host(d_r), radii) and np.array_equal(host(d_t), tpg), what
    return n_vis, packed


@pytest.mark.parametrize("C,N", COMPACT_SHAPES)
def test_bin_compact(hip_lib, C, N):
    """(C, N) with C * N at the scan's edges, N no power of two where the camera is a division; no pair visible, all, the first,
    the last, runs of eight (a thread's eight pairs all visible or none); radii and tiles_per_gauss 16-byte aligned (two 16-byte
    loads per array and thread) and one element behind (the generic scan).  Keys, ids and ranks bit for bit, the canary at every
    rank of an invisible pair and behind n_vis, the device totals, and {totals, tag} in pinned host memory after a stream
    synchronise."""
    n = C * N
    k = COMPACT_SHAPES.index((C, N))
    patterns = R.VIS_PATTERNS if n < 100_000 else (R.VIS_PATTERNS[k % 5], R.VIS_PATTERNS[(k + 2) % 5])
    for j, pattern in enumerate(patterns):
        radii, depths, tpg = R.compact_input(C, N, pattern)
        for by in (0, 1):
            n_vis, _ = run_compact(C, N, radii, depths, tpg, by, tag=1000 * k + 10 * j + by)
            assert n_vis == int(R.vis_pattern(pattern, n).sum())
    radii, depths, tpg = R.compact_input(C, N, "runs8")
    run_compact(C, N, radii, depths, tpg, 0, tag=7, rank=False, mailbox=False)
    run_compact(C, N, radii, depths, tpg, 1, tag=8, rank=False, mailbox=True)


def test_bin_compact_low_word_full(hip_lib):
    """Tile counts that sum to exactly 2^32 - 1: the low word of the packed totals is full and nothing is carried into n_vis.
    (mtgs_bin_compact alone: nothing downstream accepts such an M.)"""
    top = (1 << 31) - 1
    for by in (0, 1):
        radii = np.array([3, 0, 1, -2, 1, 0, 0, 0, 0, 1], dtype=np.int32)
        tpg = np.array([top, 0, top, 0, 1, 0, 0, 0, 0, 0], dtype=np.int32)
        depths = np.linspace(1.0, 2.0, 10).astype(np.float32)
        n_vis, packed = run_compact(1, 10, radii, depths, tpg, by, tag=99)
        assert n_vis == 4 and packed == (4 << 32) | 0xFFFFFFFF


@pytest.mark.parametrize("C,N", [(0, 5), (3, 0), (0, 0)])
def test_bin_compact_of_nothing(hip_lib, C, N):
    x, tot = can(64), can64(1 + SL)
    mb = torch.full((2 + SL,), CAN64, dtype=torch.int64).pin_memory()
    p = x.data_ptr()
    _call("mtgs_bin_compact", C, N, p, p, p, p, p, p, tot.data_ptr(), mb.data_ptr(), 41, p, 0, _st())
    torch.cuda.current_stream().synchronize()
    m = mb.numpy()
    assert int(m[0]) == 0 and int(m[1]) == 41 and (m[2:] == CAN64).all()
    assert written(tot, 1, np.zeros(1, dtype=np.int64)) and untouched(x)
    tot = can64(1 + SL)
    _call("mtgs_bin_compact", C, N, None, None, None, None, None, None, tot.data_ptr(), None, 0, None, 0, _st())
    assert written(tot, 1, np.zeros(1, dtype=np.int64))


# ---- mtgs_bin_scan ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_vis", [1, 2047, 2048, 2049, 524289])
def test_bin_scan(hip_lib, n_vis):
    """The gathered scan: tiles_per_gauss read through a random permutation (n_vis of n_vis + 7 pairs)."""
    rng = np.random.default_rng(n_vis)
    tpg = rng.integers(0, 10, n_vis + 7).astype(np.int32)
    ids = rng.permutation(n_vis + 7)[:n_vis].astype(np.int32)
    cum, w = can64(n_vis + SL), Ws("mtgs_scan_workspace_bytes", n_vis)
    d_ids, d_tpg = up(ids), up(tpg)
    _call("mtgs_bin_scan", n_vis, d_ids.data_ptr(), d_tpg.data_ptr(), cum.data_ptr(), w.ptr, w.size, _st())
    assert written(cum, n_vis, R.scan_inclusive(tpg[ids])) and w.intact()
    _call("mtgs_bin_scan", 0, None, None, cum.data_ptr(), None, 0, _st())
    assert written(cum, n_vis, R.scan_inclusive(tpg[ids]))


# ---- mtgs_bin_emit ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", R.SCENES, ids=scene_ids(R.SCENES))
def test_bin_emit(hip_lib, key):
    """onetile-n: n one-tile Gaussians fill the 2048-entry window exactly (n at the 256-ary search's step roundings and at the
    window's size); cover-tw-th: a grid-covering Gaussian of 2047 / 2048 / 2049 / 4096 tiles first puts a block boundary just
    before, on and just behind a Gaussian boundary; mix: one-tile, 3 x 3 and grid-covering rectangles, one camera (no division)
    and three (idx / N); cams-3-1: N = 1; zerotile: 3000 entries without a tile between, before and behind the ones that own
    tiles -- the slots behind them are not in the window ("blocks": the window of the second block of slots).  tile_keys and
    gids bit for bit, every key inside the grid."""
    sc, ref = R.scene(*key), R.reference(*key)
    M, n_vis = ref["M"], ref["n_vis"]
    tk, g = can(M + SL), can(M + SL)
    ids, cum = up(ref["ids_sorted"].astype(np.int32)), up(ref["cum"])
    means, radii = up(sc["means2d"]), up(sc["radii"])
    _call("mtgs_bin_emit", M, n_vis, ids.data_ptr(), sc["N"], means.data_ptr(), radii.data_ptr(), cum.data_ptr(), R.TS, sc["tw"],
          sc["th"], tk.data_ptr(), g.data_ptr(), _st())
    got = host(tk)[:M].view(np.uint32)
    assert int(got.max()) < sc["C"] * sc["tw"] * sc["th"]
    assert written(g, M, ref["gids"]) and written(tk, M, ref["tile_keys"])
    if key[0] == "zerotile":
        off_screen = np.flatnonzero((sc["radii"].reshape(-1) > 0) & (ref["tpg"].reshape(-1) == 0))
        assert off_screen.size == 3000 and not np.isin(off_screen, host(g)[:M]).any()


def test_bin_emit_of_nothing(hip_lib):
    x = can(16)
    p = x.data_ptr()
    _call("mtgs_bin_emit", 0, 5, p, 5, p, p, p, 16, 4, 4, p, p, _st())
    _call("mtgs_bin_emit", 0, 0, None, 0, None, None, None, 16, 4, 4, None, None, _st())
    assert untouched(x)


# ---- mtgs_bin_sort_tiles / mtgs_bin_finalize ----------------------------------------------------------------------------------------
# (C, tile_w, tile_h): C * n_tiles = 1, 2, 255, 256, 257, 768, 65 535, 65 536, 65 537 -> key bits 1, 1, 8, 8, 9, 10, 16, 16, 17
SORT_TILES_GRIDS = [(1, 1, 1), (1, 2, 1), (3, 5, 17), (1, 16, 16), (1, 257, 1), (3, 16, 16), (3, 5, 4369), (1, 256, 256), (1, 65537, 1)]
BIG_M = (1 << 20) + 1
SORT_TILES_CASES = [(g, M) for g in SORT_TILES_GRIDS for M in (1, 1025, BIG_M)]


@pytest.mark.parametrize("grid,M", SORT_TILES_CASES, ids=[f"{c}x{tw}x{th}-{M}" for (c, tw, th), M in SORT_TILES_CASES])
def test_bin_sort_tiles_and_finalize(hip_lib, grid, M):
    """One, two and three passes (the ping-pong starts on the other side with every pass more), power-of-two tile counts
    (bit_length is log2 + 1) and others, one camera and three, 1024-key tiles and (M > 2^20) 4096-key tiles: flatten_ids and
    isect_ids against a stable argsort; the inputs are only read; mtgs_bin_finalize on mtgs_sort_pairs_u32's output gives the
    same isect_ids."""
    C, tw, th = grid
    total = C * tw * th
    keys, gids, depths = R.sort_tiles_input(C, tw, th, M)
    flat, isect = R.sort_tiles(keys, gids, depths, C, tw, th)
    d_k, d_g, d_d = up(keys), up(gids), up(depths)
    scratch, d_flat, d_isect = can(M + SL), can(M + SL), can64(M + SL)
    w = Ws("mtgs_sort_u32_workspace_bytes", M)
    _call("mtgs_bin_sort_tiles", M, C, tw, th, d_k.data_ptr(), d_g.data_ptr(), d_d.data_ptr(), scratch.data_ptr(), d_flat.data_ptr(),
          d_isect.data_ptr(), w.ptr, w.size, _st())
    assert written(d_flat, M, flat) and written(d_isect, M, isect), (grid, M)
    assert bool((host(scratch)[M:] == CAN).all()) and w.intact()
    assert np.array_equal(host(d_k).view(np.uint32), keys) and np.array_equal(host(d_g), gids)
    # the same through the plain sort and the separate id kernel
    key_bits = max(R.bit_length(total - 1), 1)
    ko, vo, isect2 = can(M + SL), can(M + SL), can64(M + SL)
    _call("mtgs_sort_pairs_u32", M, key_bits, d_k.data_ptr(), d_g.data_ptr(), ko.data_ptr(), vo.data_ptr(), w.ptr, w.size, _st())
    _call("mtgs_bin_finalize", M, ko.data_ptr(), vo.data_ptr(), d_d.data_ptr(), C, tw, th, isect2.data_ptr(), _st())
    assert written(ko, M, np.sort(keys, kind="stable")) and written(vo, M, flat) and written(isect2, M, isect), (grid, M)
    assert w.intact()


# ---- mtgs_isect_offsets -------------------------------------------------------------------------------------------------------------
def test_isect_offsets(hip_lib):
    """No entry; one entry in the first / the last tile; a thousand entries in one tile at the start, in the middle and at the
    end; three cameras with only the middle one populated; gaps of thousands of empty tiles in front of the last entry of the
    list's first 256-thread block and the first of its second; 1, 6, 256 and 4097 tiles per camera."""
    for name, C, tw, th, slots in R.offsets_cases():
        n_tiles, M = tw * th, slots.size
        rng = np.random.default_rng(M + n_tiles)
        ids = R.isect_ids_of(slots // n_tiles, slots % n_tiles, rng.integers(0, 1 << 32, M, dtype=np.uint64).astype(np.uint32), n_tiles)
        want = R.offsets(ids, C, tw, th).reshape(-1)
        off, d_ids = can(C * n_tiles + SL), up(ids)
        _call("mtgs_isect_offsets", M, d_ids.data_ptr() if M else None, C, tw, th, off.data_ptr(), _st())
        assert written(off, C * n_tiles, want), (name, C, tw, th)
    off = can(SL)
    _call("mtgs_isect_offsets", 0, None, 0, 4, 4, off.data_ptr(), _st())
    assert untouched(off)


# ---- mtgs_tile_schedule -------------------------------------------------------------------------------------------------------------
def check_schedule(order, offs, M):
    total = offs.size
    assert np.array_equal(np.sort(order), np.arange(total, dtype=np.int32)), "not a permutation"
    b = R.schedule_bucket(offs, M)[order]
    assert (np.diff(b) <= 0).all(), "bucket rises along the order"


@pytest.mark.parametrize("last", [0, 3, 4092, 100_000])
@pytest.mark.parametrize("total", list(R.SCHEDULE_GRIDS))
def test_tile_schedule(hip_lib, total, last):
    """1 tile, one per thread of the single workgroup, one more and one less, several per thread; list lengths 0, 3, 4 (the
    bucket width), 4091, 4092 (the last bucket) and 100 000.  The order is a permutation and min(length >> 2, 1023) never rises
    along it; the LAST tile's length is M - offsets[last]: `last` moves that tile between the first and the last bucket."""
    C, tw, th = R.SCHEDULE_GRIDS[total]
    offs, M = R.schedule_input(total, last)
    order, d_offs = can(total + SL), up(offs)
    _call("mtgs_tile_schedule", C, tw, th, d_offs.data_ptr(), M, order.data_ptr(), _st())
    got = host(order)
    assert bool((got[total:] == CAN).all())
    check_schedule(got[:total], offs, M)
    b = R.schedule_bucket(offs, M)
    assert b[-1] == min(last >> 2, 1023)
    where = int(np.flatnonzero(got[:total] == total - 1)[0])
    assert (b > b[-1]).sum() <= where < (b >= b[-1]).sum()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", R.SCENES, ids=scene_ids(R.SCENES))
def test_three_formulations_agree(hip_lib, key):
    """isect_tiles(sort=True) (the depth-ordered binning, with the offsets and the tile order that ride on its outputs),
    isect_tiles(sort=False) + mtgs_sort_pairs + mtgs_isect_offsets, and the numpy reference, on the scenes of the emit test --
    the zero-tile scenes among them."""
    import mtgs_amd as gs
    sc, ref = R.scene(*key), R.reference(*key)
    C, tw, th, M = sc["C"], sc["tw"], sc["th"], ref["M"]
    means, radii, depths = up(sc["means2d"]), up(sc["radii"]), up(sc["depths"])
    tpg, ids, flat = gs.isect_tiles(means, radii, depths, R.TS, tw, th)
    off = gs.isect_offset_encode(ids, C, tw, th)
    assert off is ids._mtgs_offsets
    assert np.array_equal(host(tpg), ref["tpg"])
    assert np.array_equal(host(ids), ref["isect_ids"]) and np.array_equal(host(flat), ref["flatten_ids"])
    assert np.array_equal(host(off), ref["offsets"])
    check_schedule(host(off._mtgs_tile_order), ref["offsets"].reshape(-1), M)
    tpg2, u_ids, u_flat = gs.isect_tiles(means, radii, depths, R.TS, tw, th, sort=False)
    assert np.array_equal(host(tpg2), ref["tpg"]) and u_ids.numel() == M
    ko, vo, w = can64(M + SL), can(M + SL), Ws("mtgs_sort_workspace_bytes", M)
    bits = 32 + R.bit_length(tw * th) + R.bit_length(C - 1)
    _call("mtgs_sort_pairs", M, bits, u_ids.data_ptr(), u_flat.data_ptr(), ko.data_ptr(), vo.data_ptr(), w.ptr, w.size, _st())
    assert written(ko, M, ref["isect_ids"]) and written(vo, M, ref["flatten_ids"]) and w.intact()
    off2 = can(C * tw * th + SL)
    _call("mtgs_isect_offsets", M, ko.data_ptr(), C, tw, th, off2.data_ptr(), _st())
    assert written(off2, C * tw * th, ref["offsets"].reshape(-1))
    if key[0] == "zerotile":
        off_screen = np.flatnonzero((sc["radii"].reshape(-1) > 0) & (ref["tpg"].reshape(-1) == 0))
        assert not np.isin(off_screen, host(flat)).any()
