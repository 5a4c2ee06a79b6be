"""Plain numpy references of the depth-ordered binning (csrc/bin.hip, isect.hip, scan.hpp, radix_sort.hpp, tile_schedule_kernel of
blend.hip), stage by stage, and the input builders of tests/test_gpu_bin_edges.py.  Numpy only: tests/test_bin_refs_host.py runs
all of it without a GPU, on exactly the GPU test's inputs.

Everything is integer or bit-pattern work: every reference is exact and no tolerance appears.  The chain is

    tiles_per_gauss -> compact -> stable sort of (vis_keys, vis_ids) -> scan_inclusive -> emit -> sort_tiles -> offsets

Conventions of the builders: 16-pixel tiles; a Gaussian sits at a tile centre (mean = 16 k + 8); radius 1 makes a one-tile
rectangle, radius 16 a 3 x 3 one (clamped at the border), a radius larger than the image covers the whole grid; radii <= 0 is
invisible.  Depths are positive only (gsplat sign-extends the depth word, so negative depths are outside the contract) and
include exact ties, a denormal and +inf.  SCENES is closed: scene() refuses anything else, so the host test covers every input
the GPU test uses."""
import functools

import numpy as np

TS = 16
DENORMAL = np.float32(1e-40)
EMIT_WINDOW = 2048


def bit_length(v):
    return int(v).bit_length()


def depth_bits(depths):
    return np.ascontiguousarray(depths, dtype=np.float32).reshape(-1).view(np.uint32)


# ---- the stages -------------------------------------------------------------------------------------------------------------------
def tile_rect(means2d, radii, ts, tw, th):
    """(x0, y0, x1, y1) int32 arrays over the flattened pairs: csrc/tile_rect.hpp in float32, same operations, same order."""
    f = np.float32
    m = np.ascontiguousarray(means2d, dtype=f).reshape(-1, 2)
    r = np.ascontiguousarray(radii, dtype=np.int32).reshape(-1)
    ts = f(ts)
    tr, tx, ty = r.astype(f) / ts, m[:, 0] / ts, m[:, 1] / ts
    assert tr.dtype == tx.dtype == f

    def clamp(v, hi):
        return np.minimum(np.maximum(v, f(0.0)), f(hi)).astype(np.int32)
    return clamp(np.floor(tx - tr), tw), clamp(np.floor(ty - tr), th), clamp(np.ceil(tx + tr), tw), clamp(np.ceil(ty + tr), th)


def tiles_per_gauss(means2d, radii, ts, tw, th):
    x0, y0, x1, y1 = tile_rect(means2d, radii, ts, tw, th)
    r = np.asarray(radii).reshape(-1)
    return np.where(r > 0, (x1 - x0) * (y1 - y0), 0).astype(np.int32).reshape(np.asarray(radii).shape)


def compact(radii, depths, tpg, N):
    """vis_keys[n_vis] i64, vis_ids[n_vis] i32 in index order, vis_rank[C*N] i32 (-1 where not visible: the kernel leaves those
    alone), and the packed totals n_vis << 32 | M as the kernel sums them: the low word is the sum of EVERY tile count as an
    unsigned word.  Visible is radii > 0, whatever the tile count."""
    r = np.asarray(radii).reshape(-1)
    ids = np.flatnonzero(r > 0)
    cam = ids // max(int(N), 1)
    keys = (cam.astype(np.int64) << 32) | depth_bits(depths)[ids].astype(np.int64)
    rank = np.full(r.size, -1, dtype=np.int32)
    rank[ids] = np.arange(ids.size, dtype=np.int32)
    packed = (int(ids.size) << 32) + int(np.asarray(tpg).reshape(-1).astype(np.uint32).astype(np.uint64).sum())
    return keys, ids.astype(np.int32), rank, packed


def scan_inclusive(v):
    return np.cumsum(np.asarray(v).reshape(-1).astype(np.int64), dtype=np.int64)


def emit(ids_sorted, cum, means2d, radii, N, ts, tw, th):
    """(tile_keys[M] u32 = cam * n_tiles + tile, gids[M] i32): the entries of ids_sorted in order, each one's rectangle row-major.
    An entry without a tile (a plateau of cum) emits nothing."""
    ids_sorted = np.asarray(ids_sorted, dtype=np.int64)
    cum = np.asarray(cum, dtype=np.int64)
    cnt = np.diff(cum, prepend=0)
    x0, y0, x1, y1 = (a[ids_sorted] for a in tile_rect(means2d, radii, ts, tw, th))
    assert np.array_equal(cnt, (x1 - x0) * (y1 - y0)), "cum is not the scan of the rectangles"
    M = int(cum[-1]) if cum.size else 0
    src = np.repeat(np.arange(ids_sorted.size), cnt)
    local = np.arange(M) - (cum - cnt)[src]
    bw = (x1 - x0)[src]
    row = local // bw
    col = local - row * bw
    tile = (y0[src] + row) * tw + x0[src] + col
    cam = ids_sorted[src] // max(int(N), 1)
    return (cam * (tw * th) + tile).astype(np.uint32), ids_sorted[src].astype(np.int32)


def sort_tiles(tile_keys, gids, depths, C, tw, th):
    """(flatten_ids[M] i32, isect_ids[M] i64): a stable sort by tile key; gsplat's id is
    cam << (32 + bit_length(n_tiles)) | tile << 32 | depth bits."""
    tile_keys = np.asarray(tile_keys, dtype=np.uint32)
    gids = np.asarray(gids, dtype=np.int32)
    n_tiles = tw * th
    assert tile_keys.size == 0 or int(tile_keys.max()) < C * n_tiles
    order = np.argsort(tile_keys, kind="stable")
    flat = gids[order]
    k = tile_keys[order].astype(np.int64)
    return flat, isect_ids_of(k // n_tiles, k % n_tiles, depth_bits(depths)[flat], n_tiles)


def isect_ids_of(cam, tile, dbits, n_tiles):
    tb = bit_length(n_tiles)
    return (np.asarray(cam, dtype=np.int64) << (32 + tb)) | (np.asarray(tile, dtype=np.int64) << 32) | np.asarray(dbits).astype(np.int64)


def offsets(isect_ids, C, tw, th):
    """offsets[C, th, tw] i32: the first list position of every tile (M behind the last entry)."""
    n_tiles = tw * th
    tb = bit_length(n_tiles)
    hi = np.asarray(isect_ids, dtype=np.int64) >> 32
    slot = (hi >> tb) * n_tiles + (hi & ((1 << tb) - 1))
    assert (np.diff(slot) >= 0).all()
    return np.searchsorted(slot, np.arange(C * n_tiles), side="left").astype(np.int32).reshape(C, th, tw)


def schedule_bucket(offs, M):
    """The sort key of mtgs_tile_schedule, larger first: min(list length >> 2, 1023); the last tile's list ends at M."""
    o = np.asarray(offs, dtype=np.int64).reshape(-1)
    length = np.diff(np.append(o, np.int64(M)))
    return np.minimum(length >> 2, 1023)


def emit_window_model(cum, M, window=EMIT_WINDOW, fallback=False, block=256):
    """The position in ids_sorted that every output slot resolves to in bin_emit_kernel, by its own two searches restated
    literally: per block of `window` slots a 256-ary search for r0 = first r with cum[r] > s0, then per slot a binary search of
    the window cum[r0 .. r0 + window) held as 32-bit words (0x7fffffff behind n_vis).  fallback = False is the kernel as it was:
    a slot whose entry is not in the window ends at the window's last entry.  fallback = True adds the kernel's search of
    cum[r0 + window .. n_vis) for exactly those slots."""
    cum = np.asarray(cum, dtype=np.int64)
    n_vis = cum.size
    pos = np.empty(M, dtype=np.int64)
    tid = np.arange(block, dtype=np.int64)
    for s0 in range(0, M, window):
        lo, hi = 0, n_vis
        while lo < hi:
            step = (hi - lo + block - 1) // block
            p = lo + tid * step
            below = (p < hi) & (cum[np.minimum(p, n_vis - 1)] <= s0)
            cnt = int(below.sum())
            assert below[:cnt].all()                     # monotone in tid
            if cnt == 0:
                hi = lo
                break
            last_below = lo + (cnt - 1) * step
            hi = min(hi, lo + cnt * step)
            lo = last_below + 1
        r0 = lo
        s_c = np.full(window, 0x7fffffff, dtype=np.int64)
        k = max(min(window, n_vis - r0), 0)
        s_c[:k] = cum[r0:r0 + k].astype(np.int32)
        i = np.arange(s0, min(s0 + window, M), dtype=np.int64)
        l, h = np.zeros(i.size, dtype=np.int64), np.full(i.size, window - 1, dtype=np.int64)
        while (l < h).any():
            mid = (l + h) >> 1
            act, go = l < h, s_c[mid] <= i
            l, h = np.where(act & go, mid + 1, l), np.where(act & ~go, mid, h)
        r = r0 + l
        if fallback:
            for j in np.flatnonzero(s_c[window - 1] <= i):
                a, b = r0 + window, n_vis - 1
                while a < b:
                    mid = (a + b) >> 1
                    if cum[mid] <= i[j]:
                        a = mid + 1
                    else:
                        b = mid
                r[j] = a
        pos[s0:s0 + i.size] = r
    return pos


def binning(sc):
    """Every stage of the chain on a scene, composed."""
    C, N, tw, th = sc["C"], sc["N"], sc["tw"], sc["th"]
    tpg = tiles_per_gauss(sc["means2d"], sc["radii"], TS, tw, th)
    keys, ids, rank, packed = compact(sc["radii"], sc["depths"], tpg, N)
    order = np.argsort(keys, kind="stable")              # (keys are non-negative: signed order is the unsigned one)
    ids_sorted = ids[order]
    cum = scan_inclusive(tpg.reshape(-1)[ids_sorted])
    M = int(cum[-1]) if cum.size else 0
    assert packed == (ids.size << 32) + M
    tile_keys, gids = emit(ids_sorted, cum, sc["means2d"], sc["radii"], N, TS, tw, th)
    flat, isect = sort_tiles(tile_keys, gids, sc["depths"], C, tw, th)
    return {"tpg": tpg, "vis_keys": keys, "vis_ids": ids, "vis_rank": rank, "packed": packed, "n_vis": int(ids.size), "M": M,
            "ids_sorted": ids_sorted, "cum": cum, "tile_keys": tile_keys, "gids": gids, "flatten_ids": flat, "isect_ids": isect,
            "offsets": offsets(isect, C, tw, th)}


# ---- scenes -----------------------------------------------------------------------------------------------------------------------
ONE_TILE_NVIS = (1, 2, 255, 256, 257, 2047, 2048, 2049, 4096, 65535, 65536, 65537)
COVER_GRIDS = ((23, 89), (32, 64), (3, 683), (64, 64))   # 2047, 2048, 2049 and 4096 tiles
ZERO_TILE = ("middle", "first", "last", "blocks")
SCENES = tuple([("onetile", n) for n in ONE_TILE_NVIS] + [("cover",) + g for g in COVER_GRIDS]
               + [("mix", 1, 1000), ("mix", 3, 1000), ("cams", 3, 1)] + [("zerotile", v) for v in ZERO_TILE])
CONTRACT_SCENES = tuple(s for s in SCENES if s[0] != "zerotile")     # every visible pair owns at least one tile


def _depths(rng, n, denormal_at=None):
    """Positive depths with exact ties, one denormal and one +inf (n permitting)."""
    d = rng.uniform(0.1, 100.0, n).astype(np.float32)
    if n >= 8:
        a, b = rng.integers(0, n, n // 4), rng.integers(0, n, n // 4)
        d[a] = d[b]
    if n >= 2:
        i, j = (int(v) for v in rng.choice(n, 2, replace=False))
        if denormal_at is not None:
            j = j if j != denormal_at else i
            i = denormal_at
        d[i], d[j] = DENORMAL, np.float32(np.inf)
    return d


def _centres(tiles, tw):
    t = np.asarray(tiles, dtype=np.int64)
    return np.stack([16 * (t % tw) + 8, 16 * (t // tw) + 8], axis=-1).astype(np.float32)


def _pack(C, N, tw, th, means, radii, depths):
    return {"C": C, "N": N, "tw": tw, "th": th, "means2d": np.ascontiguousarray(means, dtype=np.float32).reshape(C, N, 2),
            "radii": np.ascontiguousarray(radii, dtype=np.int32).reshape(C, N),
            "depths": np.ascontiguousarray(depths, dtype=np.float32).reshape(C, N)}


def _cover_radius(tw, th):
    return 16 * 2 * max(tw, th)


@functools.lru_cache(maxsize=None)
def _scene(key):
    kind = key[0]
    rng = np.random.default_rng(sum((i + 1) * ord(c) for i, c in enumerate(repr(key))))
    if kind == "onetile":                                # n_vis one-tile Gaussians among a quarter more invisible ones
        n_vis, tw, th = key[1], 37, 29
        N = n_vis + n_vis // 4 + 1
        vis = np.zeros(N, dtype=bool)
        vis[rng.choice(N, n_vis, replace=False)] = True
        radii = np.where(vis, 1, -(np.arange(N) % 2))
        return _pack(1, N, tw, th, _centres(rng.integers(0, tw * th, N), tw), radii, _depths(rng, N))
    if kind == "cams":                                   # C cameras of N one-tile Gaussians, all visible
        C, N, tw, th = key[1], key[2], 5, 3
        return _pack(C, N, tw, th, _centres(rng.integers(0, tw * th, C * N), tw), np.ones(C * N), _depths(rng, C * N))
    if kind == "cover":                                  # one grid-covering Gaussian nearest, then one-tile ones
        tw, th = key[1], key[2]
        N = 1 + 2100 + 30
        at = int(rng.integers(1, N))
        radii = np.ones(N, dtype=np.int64)
        radii[rng.choice(np.delete(np.arange(N), at), 30, replace=False)] = 0
        radii[at] = _cover_radius(tw, th)
        return _pack(1, N, tw, th, _centres(rng.integers(0, tw * th, N), tw), radii, _depths(rng, N, denormal_at=at))
    if kind == "mix":                                    # one-tile, 3 x 3, grid-covering and invisible, C cameras
        C, N, tw, th = key[1], key[2], 20, 15
        u = rng.random(C * N)
        radii = np.select([u < 0.55, u < 0.80, u < 0.815, u < 0.9], [1, 16, _cover_radius(tw, th), 0], -3)
        return _pack(C, N, tw, th, _centres(rng.integers(0, tw * th, C * N), tw), radii, _depths(rng, C * N))
    assert kind == "zerotile"
    # one camera, 8 x 6 tiles: one grid-covering Gaussian, 3000 with radii > 0 entirely left of the grid at consecutive depths
    # (no tile), 100 one-tile ones; "middle": cover < off-screen < one-tile in depth; "first" / "last": the off-screen block
    # before / behind the other two; "blocks": 2100 one-tile Gaussians in place of the covering one, so that the slots behind
    # the off-screen block lie in the SECOND 2048-slot block, whose window begins at entry 2048.  Index order is a random
    # permutation of that.
    tw, th, n_off, n_one = 8, 6, 3000, 100
    n_head = 2100 if key[1] == "blocks" else 1
    N = n_head + n_off + n_one
    head = _centres(rng.integers(0, tw * th, n_head), tw)
    means = np.concatenate([head, np.stack([np.full(n_off, -72.0), 16.0 * (np.arange(n_off) % th) + 8.0], -1),
                            _centres(rng.integers(0, tw * th, n_one), tw)])
    radii = np.concatenate([np.full(n_head, 1 if key[1] == "blocks" else _cover_radius(tw, th)), np.ones(n_off), np.ones(n_one)])
    front = 0.5 + np.arange(n_head) / 8192.0
    off = 1.0 + np.arange(n_off) / 4096.0
    one = 10.0 + 0.5 * (np.arange(n_one) // 2)           # pairs of equal depths
    if key[1] in ("middle", "blocks"):
        front[0], one[-1] = DENORMAL, np.inf
    elif key[1] == "first":
        front[0], off[0], one[-1] = 2.0, DENORMAL, np.inf
    else:
        front[0], off = DENORMAL, 1000.0 + np.arange(n_off)
        off[-1] = np.inf
    depths = np.concatenate([front, off, one]).astype(np.float32)
    p = rng.permutation(N)
    return _pack(1, N, tw, th, means[p], radii[p], depths[p])


def scene(*key):
    assert key in SCENES, key
    return _scene(key)


@functools.lru_cache(maxsize=None)
def reference(*key):
    """binning(scene(key)), computed once and shared; treat as read-only."""
    return binning(scene(*key))


# ---- inputs of the single-stage tests -----------------------------------------------------------------------------------------------
SCAN_N = (1, 7, 8, 9, 2047, 2048, 2049, 524288, 524289, 526337)       # 524 288 = 256 blocks of 2048: the spine's second round
VIS_PATTERNS = ("none", "all", "first", "last", "runs8")


def scan_values(n, big):
    """Tile counts; big: large enough that the total passes 2^32 from n = 7 on."""
    rng = np.random.default_rng(n + 17 * big)
    return (rng.integers(1 << 29, (1 << 31) - 1, n) if big else rng.integers(0, 10, n)).astype(np.int32)


def vis_pattern(name, n):
    i = np.arange(n)
    return {"none": i < 0, "all": i >= 0, "first": i == 0, "last": i == n - 1, "runs8": (i // 8) % 2 == 0}[name]


def compact_input(C, N, pattern):
    """radii (> 0, 0 and negative), positive depths, tile counts (0 where invisible; 0 for some visible pairs too)."""
    n = C * N
    rng = np.random.default_rng(n * 5 + len(pattern))
    vis = vis_pattern(pattern, n)
    radii = np.where(vis, rng.integers(1, 50, n), -rng.integers(0, 2, n)).astype(np.int32)
    tpg = np.where(vis, rng.integers(0, 40, n), 0).astype(np.int32)
    return radii, _depths(rng, n), tpg


def sort_tiles_input(C, tw, th, M):
    """Tile keys in range in long runs of equal tiles, indices into a small depth array with many equal depths."""
    total = C * tw * th
    rng = np.random.default_rng(total * 3 + M)
    runs = rng.integers(1, 40, M // 8 + 2)
    assert int(runs.sum()) >= M
    keys = np.repeat(rng.integers(0, total, runs.size), runs)[:M].astype(np.uint32)
    keys[-1] = total - 1                                 # (the largest key is present)
    n_g = min(M, 5000)
    depths = _depths(rng, n_g)
    depths[rng.integers(0, n_g, n_g // 2)] = np.float32(3.5)
    return keys, rng.integers(0, n_g, M).astype(np.int32), depths


OFFSET_GRIDS = {1: (1, 1), 6: (3, 2), 256: (16, 16), 4097: (241, 17)}


def offsets_cases():
    """(name, C, tw, th, slots[M]): slots = cam * n_tiles + tile of every list entry, ascending."""
    out = []
    for n_tiles, (tw, th) in OFFSET_GRIDS.items():
        for C in (1, 3):
            total = C * n_tiles
            z = np.zeros(0, dtype=np.int64)
            out += [("empty", C, tw, th, z), ("one_first", C, tw, th, np.array([0])), ("one_last", C, tw, th, np.array([total - 1]))]
            for where, s in (("start", 0), ("middle", total // 2), ("end", total - 1)):
                out.append(("all_in_" + where, C, tw, th, np.full(1000, s)))
            if C == 3:                                   # whole empty cameras at either end
                rng = np.random.default_rng(n_tiles)
                out.append(("middle_camera", C, tw, th, np.sort(rng.integers(n_tiles, 2 * n_tiles, 700))))
        if n_tiles == 4097:
            # entries 0..254 in the first tiles, entry 255 and entry 256 (the first of the list's second 256-thread block)
            # 3000 and 5000 empty tiles further, the rest behind another gap
            for C in (1, 3):
                total = C * n_tiles
                gap = np.concatenate([np.arange(255) // 3, [100 + 3000], [100 + 3000 + 5000 if C == 3 else 100 + 3000 + 900],
                                      np.full(343, total - 40)])
                out.append(("gaps", C, tw, th, gap))
    return out


SCHEDULE_GRIDS = {1: (1, 1, 1), 1023: (3, 11, 31), 1024: (1, 32, 32), 1025: (1, 41, 25), 5000: (1, 100, 50)}
SCHEDULE_LENGTHS = (0, 3, 4, 5, 7, 8, 100, 4091, 4092, 4095, 4096, 5000)     # (and 100 000, placed by hand)


def schedule_input(total, last):
    """(offsets[total] i32, M): list lengths around the bucket width 4 and the last bucket's threshold 4092, three lists of
    100 000; the LAST tile's list has length `last`."""
    rng = np.random.default_rng(total)
    length = np.asarray(SCHEDULE_LENGTHS)[rng.integers(0, len(SCHEDULE_LENGTHS), total)]
    if total > 8:
        length[:len(SCHEDULE_LENGTHS)] = SCHEDULE_LENGTHS            # (every length is present)
        length[rng.choice(np.arange(len(SCHEDULE_LENGTHS), total - 1), 3, replace=False)] = 100_000
    length[-1] = last
    cum = np.cumsum(length)
    assert cum[-1] < 1 << 31
    return (cum - length).astype(np.int32), int(cum[-1])
