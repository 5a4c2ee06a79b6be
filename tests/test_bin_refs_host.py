"""tests/bin_refs.py without a GPU: (1) the composed numpy reference of the depth-ordered binning equals the project's C oracle
(oracle.isect_tiles(sort=True) and isect_offset_encode) on every scene of tests/test_gpu_bin_edges.py; (2) the scenes are what
that file says they are; (3) emit_window_model, the literal restatement of bin_emit_kernel's two searches, agrees with the
reference wherever every visible pair owns a tile, and WITHOUT the global-memory fallback resolves slots of the zero-tile scene
to the wrong Gaussian -- the record of the defect the fallback closes; (4) the small references against loops."""
import numpy as np
import pytest

from tests import bin_refs as R


# ---- (1) the composition against the C oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", R.SCENES, ids=lambda k: "-".join(str(v) for v in k))
def test_composed_reference_equals_the_oracle(oracle, key):
    sc, ref = R.scene(*key), R.reference(*key)
    tpg, ids, flat = oracle.isect_tiles(sc["means2d"], sc["radii"], sc["depths"], R.TS, sc["tw"], sc["th"], sort=True)
    off = oracle.isect_offset_encode(ids, sc["C"], sc["tw"], sc["th"])
    assert ref["M"] == ids.shape[0] > 0
    assert np.array_equal(ref["tpg"], tpg)
    assert np.array_equal(ref["isect_ids"], ids) and ref["isect_ids"].dtype == ids.dtype
    assert np.array_equal(ref["flatten_ids"], flat)
    assert np.array_equal(ref["offsets"], off) and ref["offsets"].shape == off.shape
    # the unsorted emission of the oracle holds the same pairs
    _, u_ids, u_flat = oracle.isect_tiles(sc["means2d"], sc["radii"], sc["depths"], R.TS, sc["tw"], sc["th"], sort=False)
    tb = R.bit_length(sc["tw"] * sc["th"])
    want = R.isect_ids_of(ref["tile_keys"].astype(np.int64) // (sc["tw"] * sc["th"]), ref["tile_keys"].astype(np.int64) % (sc["tw"] * sc["th"]),
                          R.depth_bits(sc["depths"])[ref["gids"]], sc["tw"] * sc["th"])
    a, b = np.lexsort((u_flat, u_ids)), np.lexsort((ref["gids"], want))
    assert np.array_equal(u_ids[a], want[b]) and np.array_equal(u_flat[a], ref["gids"][b]) and tb >= 1


# ---- (2) the scenes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", R.SCENES, ids=lambda k: "-".join(str(v) for v in k))
def test_scenes_are_what_they_claim(key):
    sc, ref = R.scene(*key), R.reference(*key)
    d, r = sc["depths"].reshape(-1), sc["radii"].reshape(-1)
    assert (d > 0).all() and not np.isnan(d).any()
    if d.size >= 2:
        assert (d == R.DENORMAL).any() and np.isinf(d).any() and 0 < float(R.DENORMAL) < np.finfo(np.float32).tiny
    if d.size >= 8:
        assert np.unique(d[r > 0]).size < (r > 0).sum()                  # exact ties among the visible
    assert ((sc["means2d"] - 8) % 16 == 0).all()
    vis_tpg = ref["tpg"].reshape(-1)[r > 0]
    n_tiles = sc["tw"] * sc["th"]
    if key[0] == "onetile":
        assert ref["n_vis"] == key[1] == ref["M"] and (vis_tpg == 1).all()
    elif key[0] == "cams":
        assert (vis_tpg == 1).all() and ref["n_vis"] == sc["C"] * sc["N"]
    elif key[0] == "cover":
        first = ref["ids_sorted"][0]
        assert ref["tpg"].reshape(-1)[first] == n_tiles == ref["cum"][0] and (np.delete(vis_tpg, np.flatnonzero(np.flatnonzero(r > 0) == first)) == 1).all()
        assert n_tiles in (2047, 2048, 2049, 4096) and ref["M"] > n_tiles + R.EMIT_WINDOW
    elif key[0] == "mix":
        assert {1, 9, n_tiles} <= set(vis_tpg.tolist()) and (r <= 0).any() and (vis_tpg > 0).all()
    else:
        cnt = ref["tpg"].reshape(-1)[ref["ids_sorted"]]
        zero = np.flatnonzero(cnt == 0)
        assert zero.size == 3000 and np.array_equal(zero, np.arange(zero[0], zero[0] + 3000)) and ref["n_vis"] == sc["N"]
        assert zero[0] == {"middle": 1, "first": 0, "last": 101, "blocks": 2100}[key[1]]
        assert not np.isin(ref["ids_sorted"][zero], ref["flatten_ids"]).any()
        assert ref["M"] == (2100 if key[1] == "blocks" else n_tiles) + 100 and (cnt[cnt > 0] == 1).sum() == ref["n_vis"] - 3000 - (key[1] != "blocks")
    if key in R.CONTRACT_SCENES:
        assert (vis_tpg >= 1).all()
    assert int(ref["tile_keys"].max()) < sc["C"] * n_tiles


# ---- (3) the window model -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", R.SCENES, ids=lambda k: "-".join(str(v) for v in k))
def test_emit_window_model(key):
    ref = R.reference(*key)
    cum, M = ref["cum"], ref["M"]
    owner = np.searchsorted(cum, np.arange(M), side="right")             # first r with cum[r] > i
    assert np.array_equal(ref["ids_sorted"][owner], ref["gids"])
    fixed = R.emit_window_model(cum, M, fallback=True)
    assert np.array_equal(fixed, owner)
    was = R.emit_window_model(cum, M, fallback=False)
    if key not in (("zerotile", "middle"), ("zerotile", "blocks")):
        # the contract scenes; and the off-screen block first (r0 lands behind it) or last (no slot behind it)
        assert np.array_equal(was, owner)
    else:
        wrong = np.flatnonzero(was != owner)
        cnt = np.diff(cum, prepend=0)
        assert wrong.size == 100 and (cnt[was[wrong]] == 0).all()        # every slot behind the block: an off-screen Gaussian's
        r0 = 0 if key[1] == "middle" else R.EMIT_WINDOW                  # ("blocks": they lie in the second block of slots)
        assert np.array_equal(was[wrong], np.full(100, r0 + R.EMIT_WINDOW - 1)) and wrong[0] >= r0


def test_emit_window_model_at_other_window_sizes():
    """The same model with a small window: plateaus longer than the window in front of, inside and behind a block."""
    rng = np.random.default_rng(3)
    for window, block in ((8, 4), (16, 4), (64, 8)):
        for _ in range(20):
            n = int(rng.integers(1, 400))
            cnt = np.where(rng.random(n) < 0.5, 0, rng.integers(1, 3 * window, n))
            lo = int(rng.integers(0, n))
            cnt[lo:lo + int(rng.integers(0, 3 * window))] = 0
            if not cnt.any():
                cnt[int(rng.integers(0, n))] = 5
            cum = np.cumsum(cnt)
            M = int(cum[-1])
            owner = np.searchsorted(cum, np.arange(M), side="right")
            assert np.array_equal(R.emit_window_model(cum, M, window=window, fallback=True, block=block), owner)


# ---- (4) the small references against loops -----------------------------------------------------------------------------------------
def test_tile_rect_and_emit_against_loops():
    sc, ref = R.scene("mix", 3, 1000), R.reference("mix", 3, 1000)
    x0, y0, x1, y1 = R.tile_rect(sc["means2d"], sc["radii"], R.TS, sc["tw"], sc["th"])
    keys, gids = [], []
    n_tiles = sc["tw"] * sc["th"]
    for g in ref["ids_sorted"]:
        for y in range(y0[g], y1[g]):
            for x in range(x0[g], x1[g]):
                keys.append((g // sc["N"]) * n_tiles + y * sc["tw"] + x)
                gids.append(g)
    assert np.array_equal(ref["tile_keys"], keys) and np.array_equal(ref["gids"], gids)
    assert R.tile_rect([[8.0, 8.0]], [1], 16, 4, 4) == tuple(np.array([v], dtype=np.int32) for v in (0, 0, 1, 1))
    assert [int(v[0]) for v in R.tile_rect([[-72.0, 8.0]], [1], 16, 4, 4)] == [0, 0, 0, 1]      # left of the grid: no tile
    assert [int(v[0]) for v in R.tile_rect([[24.0, 24.0]], [16], 16, 4, 4)] == [0, 0, 3, 3]
    assert R.tiles_per_gauss([[24.0, 24.0], [24.0, 24.0]], [16, 0], 16, 4, 4).tolist() == [9, 0]


def test_compact_packed_totals_and_rank():
    radii = np.array([3, 0, 1, -2, 1], dtype=np.int32)
    depths = np.array([1.0, 2.0, R.DENORMAL, 4.0, np.inf], dtype=np.float32)
    tpg = np.array([(1 << 31) - 1, 0, (1 << 31) - 1, 0, 1], dtype=np.int32)
    keys, ids, rank, packed = R.compact(radii.reshape(5, 1), depths, tpg, 1)
    assert ids.tolist() == [0, 2, 4] and rank.tolist() == [0, -1, 1, -1, 2]
    assert packed == (3 << 32) | 0xFFFFFFFF                              # the low word full, no carry
    assert keys.tolist() == [(0 << 32) | 0x3F800000, (2 << 32) | int(R.depth_bits([R.DENORMAL])[0]), (4 << 32) | 0x7F800000]


def test_single_stage_inputs_are_what_they_claim():
    for n in R.SCAN_N:
        small, big = R.scan_values(n, False), R.scan_values(n, True)
        assert small.dtype == big.dtype == np.int32 and (small >= 0).all() and (big > 0).all()
        assert n < 7 or int(R.scan_inclusive(big)[-1]) > 1 << 32
    assert R.SCAN_N[7] == 256 * 2048                     # one full round of the spine, then one element and one block more
    for pattern, count in zip(R.VIS_PATTERNS, (0, 2049, 1, 1, 1025)):
        radii, depths, tpg = R.compact_input(3, 683, pattern)
        keys, ids, rank, packed = R.compact(radii, depths, tpg, 683)
        assert ids.size == count == packed >> 32 and (packed & 0xFFFFFFFF) == int(tpg.sum()) and (tpg[radii <= 0] == 0).all()
        assert keys.dtype == np.int64 and ids.dtype == rank.dtype == np.int32 and (count == 0 or int(keys.max()) >> 32 == ids[-1] // 683)
        assert np.array_equal(np.flatnonzero(rank >= 0), ids) and np.array_equal(rank[ids], np.arange(count))
    for C, tw, th, M in ((1, 1, 1, 1), (3, 5, 17, 1025), (1, 65537, 1, 1025), (3, 5, 4369, (1 << 20) + 1)):
        keys, gids, depths = R.sort_tiles_input(C, tw, th, M)
        total = C * tw * th
        assert keys.dtype == np.uint32 and keys.size == gids.size == M and int(keys.max()) == total - 1 and int(gids.max()) < depths.size
        assert M < 1000 or total == 1 or 8 * np.count_nonzero(np.diff(keys.astype(np.int64))) < M         # long runs of equal tiles
        flat, isect = R.sort_tiles(keys, gids, depths, C, tw, th)
        n_tiles = tw * th
        tb = R.bit_length(n_tiles)
        assert flat.dtype == np.int32 and isect.dtype == np.int64 and (np.diff(isect >> 32) >= 0).all()
        assert int(isect[-1] >> (32 + tb)) == C - 1 and int((isect[-1] >> 32) & ((1 << tb) - 1)) == n_tiles - 1
        assert np.array_equal((isect & 0xFFFFFFFF).astype(np.uint32), R.depth_bits(depths)[flat])
    assert R.bit_length(256) == 9 and R.bit_length(255) == 8
    for total, (C, tw, th) in R.SCHEDULE_GRIDS.items():
        assert C * tw * th == total
        for last in (0, 3, 4092, 100_000):
            offs, M = R.schedule_input(total, last)
            length = np.diff(np.append(offs.astype(np.int64), M))
            assert offs.dtype == np.int32 and length[-1] == last and (length >= 0).all()
            assert total < 9 or {0, 3, 4, 4091, 4092, 100_000} <= set(length.tolist())
    assert all(tw * th == n for n, (tw, th) in R.OFFSET_GRIDS.items())


def test_offsets_and_schedule_bucket_against_loops():
    for name, C, tw, th, slots in R.offsets_cases():
        n_tiles = tw * th
        ids = R.isect_ids_of(slots // n_tiles, slots % n_tiles, np.arange(slots.size) % 7, n_tiles)
        want, nxt = np.empty(C * n_tiles, dtype=np.int32), 0
        for i, s in enumerate(slots):
            while nxt <= s:
                want[nxt] = i
                nxt += 1
        want[nxt:] = slots.size
        assert np.array_equal(R.offsets(ids, C, tw, th).reshape(-1), want), name
    offs, M = R.schedule_input(1025, 4092)
    b = R.schedule_bucket(offs, M)
    assert b[-1] == 1023 and set(b.tolist()) >= {0, 1, 2, 25, 1022, 1023}
    assert R.schedule_bucket([0, 3, 7, 4098], 4098 + 4091).tolist() == [0, 1, 1022, 1022]
