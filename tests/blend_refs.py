"""Float64 numpy reference of the compositing kernels (csrc/blend.hip: blend_fwd_kernel, blend_touch_kernel, blend_bwd_kernel in
gather and packed form) and the scene builders of tests/test_gpu_blend_edges.py.  Numpy only: tests/test_blend_refs_host.py runs
all of it without a GPU, on exactly the GPU test's inputs, checks the backward against finite differences of the forward and
measures the tolerance constants at the end of this file with the fp32 C oracle (oracle/gsplat_oracle.c).

The operation (gsplat's rasterize_to_pixels): per pixel, walk the tile's list front to back; with d = mean - pixel centre,
    sigma = (a dx^2 + c dy^2) / 2 + b dx dy,   alpha = min(0.999, o exp(-sigma)),
skip the entry unless sigma >= 0 and alpha >= 1/255 (a NaN fails both, so a NaN opacity never composites), stop BEFORE the entry
that makes T (1 - alpha) <= 1e-4, otherwise add colour x alpha T, T *= 1 - alpha.  last_ids is the position in the sorted list of
the last composited entry (0 if none).  The three constants are the fp32 values of the oracle and the kernels.

A scene is a tile grid and hand-built lists on at most 16 tiles: no projection, no binning.  Only the tiles with a list are
evaluated (the large grids have thousands of empty ones; what an empty tile must hold is `empty_render`).  SCENES is closed and
seeded: scene() refuses anything else.

Sums of |terms| (the scale of every tolerance; nothing is compared relative to a SUM, which may cancel):
  forward   channel k: sum |c_k alpha T| + |background_k| T_final (expected depth: that and the alpha term, over alpha);
            alpha: sum of the T in front of every composited entry (each product T (1 - alpha) rounds at that magnitude).
  backward  every per-pixel term is a product of geometry and dL/dalpha_i = T_i <c_i, v> - (<behind, v> - T_f (v_a - <bg, v>)) / (1 - alpha_i),
            a difference that cancels: its magnitude is taken leaf by leaf (|c_k v_k| summed, |.| of every accumulated-behind term),
            times kappa_i = sum over the entries j >= i of the pixel of 1 / (1 - alpha_j) -- the backward rebuilds T_i by DIVIDING
            T_final by every (1 - alpha_j) behind i, so a relative error eps of alpha_j arrives as eps alpha_j / (1 - alpha_j) in
            T_i: kappa is that condition number plus one rounding per step.
  The position gradient is measured in the form the kernels evaluate it (tests/util.py::moment_xy_terms):
            v_x = -o (a sum h dx + b sum h dy): terms |a h dx| and |b h dy|, not gsplat's |h (a dx + b dy)|.
"""
import functools

import numpy as np

TS = 16
F = np.float32
ALPHA_MIN = float(F(1.0) / F(255.0))     # oracle/gsplat_oracle.c: ALPHA_MIN, ALPHA_MAX, T_MIN
ALPHA_MAX = float(F(0.999))
T_MIN = float(F(1e-4))
CRIT_REL = 1e-4                          # orc_blend_fwd_ex: a decision within this relative distance of its threshold
CRIT_SIGMA = 1e-6                        # ... and |sigma| <= this with a passing alpha
NO_CLAMP_OPACITY = F(0.9989)             # blend.hip kNoClampOpacity: a batch without a larger opacity runs the clamp-free loop
HALF_LOG2E = 0.5 * np.log2(np.e)         # k: rides on the |h u|, |h w| columns of the packed rows
EPS = 2.0 ** -24
MAX_CRITICAL_PER_TILE = 5                # of 256 pixels (2 %), asserted by tests/test_blend_refs_host.py


# ---- scenes -----------------------------------------------------------------------------------------------------------------------
class Scene:
    """C cameras of W x H pixels; n Gaussians (rows of flat [C * N] arrays, N = n / C); `lists`: tile -> ids, front to back.
    D colour channels plus the depth channel if `depths` is there; `cap_pad` sentinel ids (-1) behind the last tile's list in the
    gather form's flatten_ids (a capacity-sized tensor)."""

    def __init__(self, name, C, W, H, D, depth, ed, bg, seed, cap_pad=0):
        self.name, self.C, self.W, self.H, self.D, self.ed, self.cap_pad = name, C, W, H, D, bool(ed), cap_pad
        self.tw, self.th = (W + TS - 1) // TS, (H + TS - 1) // TS
        self.tiles = C * self.tw * self.th
        self.rng = np.random.RandomState(seed)
        self.has_depth = bool(depth)
        self.DT = D + int(self.has_depth)
        self.bg = self.rng.uniform(0.1, 0.9, (C, D)).astype(F) if bg else None
        self.rows, self.lists, self.marks = [], {}, {}

    # geometry of a tile: camera, pixel origin, valid columns / rows
    def tile_box(self, tile):
        cam, t_in = divmod(tile, self.tw * self.th)
        ty, tx = divmod(t_in, self.tw)
        return cam, tx * TS, ty * TS, min(TS, self.W - tx * TS), min(TS, self.H - ty * TS)

    def tile_at(self, cam, tx, ty):
        return (cam * self.th + ty % self.th) * self.tw + tx % self.tw

    def add(self, tile, mean, conic, opacity):
        """One more Gaussian at the end of `tile`'s list; returns its id."""
        g = len(self.rows)
        col = self.rng.uniform(-0.3, 1.0, self.D)
        self.rows.append((mean[0], mean[1], conic[0], conic[1], conic[2], opacity, self.rng.uniform(1.0, 5.0)) + tuple(col))
        self.lists.setdefault(tile, []).append(g)
        return g

    def finish(self):
        while len(self.rows) % self.C:
            self.rows.append((0.0,) * (7 + self.D))
        r = np.array(self.rows, dtype=np.float64).astype(F).reshape(-1, 7 + self.D)
        self.n = r.shape[0]
        self.means, self.conics, self.opac = np.ascontiguousarray(r[:, 0:2]), np.ascontiguousarray(r[:, 2:5]), np.ascontiguousarray(r[:, 5])
        self.depths = np.ascontiguousarray(r[:, 6]) if self.has_depth else None
        self.colors = np.ascontiguousarray(r[:, 7:])
        self.lists = {t: np.asarray(v, dtype=np.int32) for t, v in sorted(self.lists.items())}
        assert len(self.lists) <= 16 and all(v.size <= 2 * 256 + 1 for v in self.lists.values()), self.name
        del self.rows, self.rng
        return self

    # ---- the two input forms
    def channels(self):
        """[n, DT] float32: colours, then the depth."""
        return self.colors if self.depths is None else np.concatenate([self.colors, self.depths[:, None]], axis=1)

    def starts(self):
        """(start[tiles + 1] int64, ids): the lists laid end to end in tile order."""
        start = np.zeros(self.tiles + 1, dtype=np.int64)
        for t, v in self.lists.items():
            start[t + 1] = v.size
        start = np.cumsum(start)
        ids = np.concatenate([v for v in self.lists.values()] + [np.zeros(0, np.int32)]).astype(np.int32)
        return start, ids

    def gather_form(self):
        """(offsets[C, th, tw] int32, flatten_ids[M] int32): the last tile ends at M = flatten_ids.size, or at the first of the
        cap_pad sentinels."""
        start, ids = self.starts()
        flat = np.concatenate([ids, np.full(self.cap_pad, -1, np.int32)])
        return start[:-1].astype(np.int32).reshape(self.C, self.th, self.tw), flat

    def packed_form(self):
        """(records[n, 16] float32, offsets[tiles + 1] int32, rank_ids int32): csrc/raster_rec.hpp."""
        start, ids = self.starts()
        rec = np.zeros((self.n, 16), dtype=F)
        rec[:, 0:2], rec[:, 2:5], rec[:, 5] = self.means, self.conics, self.opac
        with np.errstate(all="ignore"):
            rec[:, 6] = (2.0 * np.log(self.opac.astype(np.float64) / ALPHA_MIN)).astype(F)      # NaN / -inf / < 0: dropped when staged
        rec[:, 7] = np.full(self.n, 48, np.int32).view(F)                                      # radius: not read by the compositing
        rec[:, 8:8 + self.DT] = self.channels()
        return rec, start.astype(np.int32), ids

    def empty_render(self):
        """[C, DT]: what every pixel of an empty tile holds (alpha 0, last_ids 0)."""
        e = np.zeros((self.C, self.DT), dtype=F)
        if self.bg is not None:
            e[:, :self.D] = self.bg
        return e


def _conic(s_long, s_short, theta):
    cs, sn = np.cos(theta), np.sin(theta)
    il, is_ = 1.0 / s_long ** 2, 1.0 / s_short ** 2
    return cs * cs * il + sn * sn * is_, cs * sn * (il - is_), sn * sn * il + cs * cs * is_


def _blob(sc, tile, lo, hi, olo, ohi, reach=2.0):
    """A Gaussian of scale lo..hi pixels and opacity olo..ohi over the valid part of the tile."""
    _, x0, y0, vw, vh = sc.tile_box(tile)
    r = sc.rng
    s1 = r.uniform(lo, hi)
    con = _conic(s1, r.uniform(0.6 * s1, s1), r.uniform(0.0, np.pi))
    return sc.add(tile, (x0 + r.uniform(-reach, vw + reach), y0 + r.uniform(-reach, vh + reach)), con, r.uniform(olo, ohi))


def faint(sc, tile, n, budget=6.0):
    """Broad and faint: nothing terminates, every batch of the list is consumed (`budget`: about twice the sum of the alphas)."""
    hi = max(0.012, min(0.08, budget / max(n, 1)))
    return [_blob(sc, tile, 10.0, 24.0, 0.006, hi) for _ in range(n)]


def strong(sc, tile, n):
    """Small and opaque: the pixels of a tile finish at different entries."""
    return [_blob(sc, tile, 1.5, 4.0, 0.3, 1.0) for _ in range(n)]


def medium(sc, tile, n, olo=0.03, ohi=0.14):
    return [_blob(sc, tile, 3.0, 8.0, olo, ohi) for _ in range(n)]


def culled(sc, tile, n):
    """Elongated along the anti-diagonal outside the tile's top-left corner: the 3-sigma square covers the tile, the 1/255 ellipse
    does not come near it (every pixel is more than 90 short-axis variances away)."""
    _, x0, y0, _, _ = sc.tile_box(tile)
    r = sc.rng
    out = []
    for _ in range(n):
        con = _conic(r.uniform(10.0, 14.0), r.uniform(0.6, 0.8), -np.pi / 4 + r.uniform(-0.03, 0.03))
        out.append(sc.add(tile, (x0 - r.uniform(4.5, 6.0), y0 - r.uniform(4.5, 6.0)), con, r.uniform(0.5, 0.9)))
    sc.marks.setdefault("culled", []).extend(out)
    return out


def grazing(sc, tile):
    """Four round Gaussians outside the corners of the tile that reach alpha >= 1/255 at the corner pixel alone, with
    s2 = 0.95 s2max there: inside the cull's margin, far from the 1/255 threshold (alpha = 1.27 / 255)."""
    _, x0, y0, vw, vh = sc.tile_box(tile)
    out = []
    for cx, cy, sx, sy in ((0.5, 0.5, -1, -1), (vw - 0.5, 0.5, 1, -1), (0.5, vh - 0.5, -1, 1), (vw - 0.5, vh - 0.5, 1, 1)):
        o, s = 0.5, 3.0
        d = s * np.sqrt(0.95 * 2.0 * np.log(o / ALPHA_MIN) / 2.0)       # per axis, along the diagonal
        out.append(sc.add(tile, (x0 + cx + sx * d, y0 + cy + sy * d), (1 / s ** 2, 0.0, 1 / s ** 2), o))
    sc.marks.setdefault("grazing", []).extend(out)
    return out


_CLAMP_SLOTS = ((0.15, 0.15), (0.85, 0.85), (0.8, 0.2), (0.2, 0.8), (0.5, 0.5))


def clamping(sc, tile, n, opacity=None):
    """Opacity in (0.9989, 1], a few hundredths of a pixel off a pixel centre: alpha binds at 0.999 on that pixel (o exp(-sigma) >=
    0.9994 there, <= 0.98 on its neighbours).  The centres of a tile's clamping Gaussians keep apart, so that none ends the others' pixels."""
    _, x0, y0, vw, vh = sc.tile_box(tile)
    r = sc.rng
    out = []
    for _ in range(n):
        k = sc.marks.setdefault("_slots", {}).get(tile, 0)
        sc.marks["_slots"][tile] = k + 1
        fx, fy = _CLAMP_SLOTS[k % len(_CLAMP_SLOTS)]
        o = r.uniform(0.9998, 1.0) if opacity is None else opacity
        s = r.uniform(3.2, 3.8)
        mean = (x0 + int(fx * vw) + 0.5 + r.uniform(0.02, 0.07), y0 + int(fy * vh) + 0.5 + r.uniform(0.02, 0.07))
        out.append(sc.add(tile, mean, _conic(s, 0.9 * s, r.uniform(0, np.pi)), o))
    return out


def degenerate(sc, tile):
    """Candidates that must never composite or that composite on a part of the plane only, between live ones."""
    _, x0, y0, vw, vh = sc.tile_box(tile)
    cx, cy = x0 + min(vw, 7) + 0.25, y0 + min(vh, 8) + 0.75
    rnd = _conic(5.0, 4.0, 0.7)
    dead = {}
    medium(sc, tile, 3)
    dead["below"] = sc.add(tile, (cx, cy), rnd, np.nextafter(F(1.0) / F(255.0), F(0.0)))
    dead["zero"] = sc.add(tile, (cx, cy), rnd, 0.0)
    medium(sc, tile, 2)
    dead["negative"] = sc.add(tile, (cx, cy), rnd, -0.5)
    dead["nan"] = sc.add(tile, (cx, cy), rnd, np.nan)
    sc.add(tile, (cx, cy), (0.02, 0.05, 0.02), 0.5)                     # indefinite: b^2 > a c, sigma < 0 on two sectors
    sc.add(tile, (cx, cy), (-0.01, 0.0, 0.02), 0.4)                     # a <= 0
    sc.add(tile, (x0 + min(vw - 1, 5) + 0.5, y0 + min(vh - 1, 7) + 0.5), rnd, 0.35)      # exactly on a pixel centre
    medium(sc, tile, 3)
    sc.marks.setdefault("dead", []).extend(dead.values())


LENGTHS = (0, 1, 2, 3, 127, 128, 129, 255, 256, 257, 2 * 128 + 1, 2 * 256 + 1)


def _placement(sc):
    """Tiles worth populating: tile 0, the launch's last tile, the last of camera 0 / first of camera 1, a right-edge, a
    bottom-edge and the corner tile of camera 0, then interior ones."""
    per = sc.tw * sc.th
    want = [0, sc.tiles - 1, per - 1, per % sc.tiles, sc.tile_at(0, sc.tw - 1, 1), sc.tile_at(0, 0, sc.th - 1),
            sc.tile_at(0, sc.tw - 1, sc.th // 2), sc.tile_at(0, 0, sc.th // 3)]
    want += [sc.tile_at(c, tx, 2 + 3 * k) for k in range(8) for c in range(sc.C) for tx in range(sc.tw)]
    seen = []
    for t in want:
        if t not in seen:
            seen.append(t)
    return seen


def _fill_lengths(sc, kind, last_len):
    """One list per length of LENGTHS (the empty one is a tile like every other); the launch's last tile gets `last_len`."""
    tiles = _placement(sc)
    first, last, rest = tiles[0], tiles[1], tiles[2:]
    lens = [n for n in LENGTHS if n not in (0, last_len)]
    assert len(rest) >= len(lens), sc.name
    kind(sc, last, last_len)
    kind(sc, first, lens[-1])
    for t, n in zip(rest, lens[:-1]):
        kind(sc, t, n)
    sc.marks["last_tile_len"] = last_len


def _fill_tail(sc, kind, last_len):
    """A few lists and the launch's last tile, for the sentinels behind it."""
    tiles = _placement(sc)
    kind(sc, tiles[0], 3)
    kind(sc, tiles[1], last_len)
    medium(sc, tiles[2], 40)
    sc.marks["last_tile_len"] = last_len


def _fill_edges(sc, small=False):
    """The cull, the clamp, termination in the second 256-batch, degenerate candidates, a Gaussian shared by four tiles."""
    tiles = _placement(sc)
    t = iter(tiles)
    m = sc.marks
    # termination in the middle of the second batch
    m["second_batch"] = tile = next(t)
    medium(sc, tile, 513)
    # last tile of the launch: degenerate candidates
    degenerate(sc, next(t))
    # clamp in front: the accumulated-behind term flows through a bound alpha
    m["clamp_front"] = tile = next(t)
    clamping(sc, tile, 3)
    medium(sc, tile, 24, 0.1, 0.5)
    # clamp: a batch (of either size) without a clamp candidate, then one with one; 0.9989 and the next fp32 value
    m["clamp"] = tile = next(t)
    faint(sc, tile, 256, budget=3.0)
    clamping(sc, tile, 3)
    clamping(sc, tile, 1, opacity=NO_CLAMP_OPACITY)
    clamping(sc, tile, 1, opacity=np.nextafter(NO_CLAMP_OPACITY, F(1.0)))
    medium(sc, tile, 6)
    if small:
        tile = m["clamp_front"]
    else:
        tile = next(t)
    # a batch culled as a whole between two live ones: forward batches of 256 | backward batches of 256 (counted from the
    # last contributor) | both directions with batches of 128
    if not small:
        faint(sc, tile, 256); culled(sc, tile, 256); faint(sc, tile, 1)
        tile = next(t)
        faint(sc, tile, 1); culled(sc, tile, 256); faint(sc, tile, 256)
        tile = next(t)
        faint(sc, tile, 128); culled(sc, tile, 256); faint(sc, tile, 128)
        # odd and even survivor counts
        tile = next(t)
        for k in range(21):
            medium(sc, tile, 1); culled(sc, tile, 1)
        tile = next(t)
        for k in range(20):
            culled(sc, tile, 1); medium(sc, tile, 1)
        grazing(sc, next(t))
    else:
        for k in range(21):
            medium(sc, tile, 1); culled(sc, tile, 1)
        grazing(sc, tile)
    # one set of Gaussians on four neighbouring tiles, around their common corner
    if sc.tw >= 2 and sc.th >= 2:
        quad = [sc.tile_at(0, tx, ty) for ty in (0, 1) for tx in (1, 2)] if small else \
               [sc.tile_at(sc.C - 1, tx, ty) for ty in (4, 5) for tx in (0, 1)]
        _, x0, y0, _, _ = sc.tile_box(quad[3])
        ids = []
        for _ in range(20):
            s = sc.rng.uniform(3.0, 8.0)
            ids.append(sc.add(quad[0], (x0 + sc.rng.uniform(-5, 5), y0 + sc.rng.uniform(-5, 5)), _conic(s, 0.7 * s, sc.rng.uniform(0, np.pi)),
                              sc.rng.uniform(0.05, 0.5)))
        for q in quad[1:]:
            sc.lists.setdefault(q, []).extend(ids)
        m["shared"] = ids


def _fill_wide(sc):
    """The 16- and 32-channel kernels: one pixel per lane whatever the grid, batches of 256."""
    t = iter(_placement(sc))
    faint(sc, next(t), 257)
    tile = next(t)
    strong(sc, tile, 129)
    tile = next(t)
    sc.marks["clamp"] = tile
    clamping(sc, tile, 2); medium(sc, tile, 30)
    degenerate(sc, next(t))
    tile = next(t)
    faint(sc, tile, 3); culled(sc, tile, 5); medium(sc, tile, 4)


# name: (cameras, width, height, colour channels, depth, ed, backgrounds, content, seed, cap_pad).  The seeds are the first of
# seed + 100 k at which no tile has more than 4 critical pixels (test_blend_refs_host.py asserts the cap of 5).
# Tile counts on both sides of every pick_ppl threshold (forward 3000 / 16000, backward 1536 / 6000); the widths and heights leave a
# right-edge tile of 1 or 8 columns and a bottom-edge tile of 1 or 11 rows.
_SPECS = {
    # 3 x 2 tiles: 8 valid columns, 11 valid rows
    "edges-6t-d3": (1, 40, 27, 3, False, False, False, ("edges", True), 11, 0),
    "wide16-6t": (1, 40, 27, 16, False, False, True, ("wide",), 12, 0),
    "wide32-6t": (1, 33, 17, 31, True, True, False, ("wide",), 13, 0),
    "sentinel-batch-start-6t": (1, 40, 27, 3, False, False, False, ("tail", "faint", 256), 14, 70),
    "sentinel-mid-batch-6t": (1, 40, 27, 4, False, False, True, ("tail", "faint", 200), 15, 70),
    # 1535 = 5 x 307 | 1536 = 4 x 384
    "faint-1535t-d4": (1, 80, 307 * 16, 3, True, True, True, ("faint", 257), 421, 0),
    "strong-1535t-d4": (1, 65, 307 * 16 - 15, 4, False, False, False, ("strong", 129), 22, 0),
    "edges-1536t-d4": (1, 49, 384 * 16 - 5, 3, True, False, True, ("edges", False), 23, 0),
    # 2999 = 1 x 2999 | 3000 = 2 cameras x 3 x 500
    "faint-2999t-d7": (1, 16, 2999 * 16 - 15, 7, False, False, True, ("faint", 513), 24, 0),
    "strong-3000t-d3": (2, 40, 500 * 16 - 5, 2, True, True, False, ("strong", 256), 25, 0),
    # 5999 = 7 cameras x 1 x 857 | 6000 = 2 cameras x 3 x 1000
    "edges-5999t-d5": (7, 8, 857 * 16 - 5, 4, True, True, True, ("edges", False), 26, 0),
    "faint-6000t-d8": (2, 33, 1000 * 16, 7, True, False, False, ("faint", 128), 427, 0),
    # 15999 = 3 x 5333 | 16000 = 4 cameras x 4 x 1000
    "strong-15999t-d1": (1, 48, 5333 * 16 - 15, 1, False, False, True, ("strong", 257), 28, 0),
    "faint-16000t-d4": (4, 64, 1000 * 16, 4, False, False, False, ("faint", 256), 129, 70),
    "strong-16000t-d3": (4, 49, 1000 * 16 - 5, 3, False, False, True, ("strong", 129), 30, 70),
    "edges-16000t-d7": (4, 56, 1000 * 16 - 15, 6, True, True, True, ("edges", False), 31, 0),
}
SCENES = tuple(_SPECS)
# the grids on the two sides of every pick_ppl threshold
THRESHOLD_GRIDS = {1536: ("faint-1535t-d4", "edges-1536t-d4"), 3000: ("faint-2999t-d7", "strong-3000t-d3"),
                   6000: ("edges-5999t-d5", "faint-6000t-d8"), 16000: ("strong-15999t-d1", "faint-16000t-d4")}


@functools.lru_cache(maxsize=None)
def scene(name):
    C, W, H, D, depth, ed, bg, content, seed, cap_pad = _SPECS[name]
    sc = Scene(name, C, W, H, D, depth, ed, bg, seed, cap_pad)
    if content[0] == "edges":
        _fill_edges(sc, small=content[1])
    elif content[0] == "wide":
        _fill_wide(sc)
    elif content[0] == "tail":
        _fill_tail(sc, {"faint": faint, "strong": strong}[content[1]], content[2])
    else:
        _fill_lengths(sc, {"faint": faint, "strong": strong}[content[0]], content[1])
    return sc.finish()


def gradient_check_scene():
    """One tile, 40 Gaussians, no clamp, no termination: the forward is smooth in every input."""
    sc = Scene("fd", 1, 16, 16, 3, True, True, True, 5)
    for _ in range(40):
        _blob(sc, 0, 4.0, 9.0, 0.05, 0.2)
    return sc.finish()


# ---- forward ----------------------------------------------------------------------------------------------------------------------
def _pixels(sc, tile):
    cam, x0, y0, vw, vh = sc.tile_box(tile)
    ys, xs = np.mgrid[y0:y0 + vh, x0:x0 + vw]
    ys, xs = ys.reshape(-1), xs.reshape(-1)
    return cam, (cam * sc.H + ys) * sc.W + xs, xs + 0.5, ys + 0.5


def _entry(sc, g, px, py, params=None):
    p = params or sc
    mx, my = (float(v) for v in p.means[g])
    a, b, c = (float(v) for v in p.conics[g])
    o = float(p.opac[g])
    dx, dy = mx - px, my - py
    with np.errstate(all="ignore"):
        sigma = 0.5 * (a * dx * dx + c * dy * dy) + b * dx * dy
        vis = np.exp(-sigma)
        raw = o * vis
        alpha = np.minimum(ALPHA_MAX, raw)
        ok = (sigma >= 0.0) & (alpha >= ALPHA_MIN)                          # (NaN: False)
    return dx, dy, a, b, c, o, sigma, vis, raw, alpha, ok


def forward(sc, params=None):
    """tile -> dict over the tile's valid pixels (row-major): pix (flat pixel index), render[P, DT], alpha[P], last[P] (sorted
    index, int64), render_terms[P, DT], alpha_terms[P], critical[P], clamped[P] (a composited alpha was bound at 0.999); and the Gaussians that updated a pixel at all /
    a non-critical one (sets of ids).  `params`: float64 stand-ins for the scene's arrays (the finite-difference check)."""
    p = params or sc
    chan = np.asarray(p.channels(), dtype=np.float64)
    start, _ = sc.starts()
    out, hit_any, hit_clear = {}, set(), set()
    for tile, ids in sc.lists.items():
        cam, pix, px, py = _pixels(sc, tile)
        P = pix.size
        T, acc, tabs = np.ones(P), np.zeros((P, sc.DT)), np.zeros((P, sc.DT))
        aterm, last = np.zeros(P), np.zeros(P, dtype=np.int64)
        done, crit, bound = np.zeros(P, bool), np.zeros(P, bool), np.zeros(P, bool)
        upds = []
        for k, g in enumerate(ids):
            if done.all():
                break
            _, _, _, _, _, _, sigma, _, raw, alpha, ok = _entry(sc, g, px, py, params)
            live = ~done
            ok &= live
            with np.errstate(all="ignore"):
                c_alpha = (np.abs(alpha - ALPHA_MIN) <= CRIT_REL * ALPHA_MIN) & (sigma >= -CRIT_SIGMA)
                c_sigma = (np.abs(sigma) <= CRIT_SIGMA) & (alpha >= ALPHA_MIN)
                # (not in the oracle's rule: the backward switches the sigma / opacity gradient off where o exp(-sigma) > 0.999)
                c_clamp = (np.abs(raw - ALPHA_MAX) <= CRIT_REL * ALPHA_MAX) & (sigma >= -CRIT_SIGMA)
            nT = T * (1.0 - alpha)
            c_stop = ok & (np.abs(nT - T_MIN) <= CRIT_REL * T_MIN)
            crit |= (live & (c_alpha | c_sigma | c_clamp)) | c_stop
            stop = ok & (nT <= T_MIN)
            done |= stop
            upd = ok & ~stop
            if upd.any():
                w = np.where(upd, alpha * T, 0.0)
                acc += w[:, None] * chan[g]
                tabs += w[:, None] * np.abs(chan[g])
                aterm += np.where(upd, T, 0.0)
                T = np.where(upd, nT, T)
                last = np.where(upd, start[tile] + k, last)
                bound |= upd & (raw > ALPHA_MAX)
                upds.append((int(g), upd))
        for g, upd in upds:
            hit_any.add(g)
            if (upd & ~crit).any():
                hit_clear.add(g)
        alpha_out = 1.0 - T
        render, terms = acc.copy(), tabs.copy()
        if p.bg is not None:
            bgc = np.asarray(p.bg[cam], dtype=np.float64)
            render[:, :sc.D] += T[:, None] * bgc
            terms[:, :sc.D] += T[:, None] * np.abs(bgc)
        if sc.ed:
            den = np.maximum(alpha_out, 1e-10)
            render[:, -1] = render[:, -1] / den
            terms[:, -1] = (terms[:, -1] + np.abs(render[:, -1]) * aterm) / den
        out[tile] = dict(pix=pix, cam=cam, render=render, alpha=alpha_out, last=last, render_terms=terms, alpha_terms=aterm, critical=crit,
                         clamped=bound)
    return out, hit_any, hit_clear


# ---- backward ---------------------------------------------------------------------------------------------------------------------
ROW_GROUPS = {"xy": (0, 2), "xy_abs": (2, 4), "conic": (4, 7), "opacity": (7, 8)}        # columns of a row; colours: 8 ..


def backward(sc, fwd_in, v_render, v_alpha, params=None, rounded=True):
    """The gradients of sum(render * v_render) + sum(alpha * v_alpha) over the populated tiles, walked back to front from each
    pixel's last_ids as the kernels do.  fwd_in: tile -> dict(alpha[P], last[P], render[P, DT]) -- what the device call is given
    (float32-rounded when `rounded`: T_final is then the FLOAT32 difference 1 - alpha, the one operation every float32
    implementation shares bit for bit); v_render: tile -> [P, DT], v_alpha: tile -> [P].
    Returns dict of [n, .] float64 arrays: `rows` [n, 8 + DT] the packed kernel's raw-moment rows
        sum h dx, sum h dy | k sum |h u|, k sum |h w| | sum h dx^2, sum h dx dy, sum h dy^2 | sum h | channels      (h = vis dL/dalpha)
    `rows_terms` their sums of |terms|; `dense` [n, 8 + DT] gsplat's gradients in the same column order
        v_means2d | |v_means2d| | v_conics | v_opacities | v_colors (v_depths last)
    summed PER PIXEL in gsplat's form, `dense_terms` their sums of |terms| (module docstring)."""
    p = params or sc
    chan = np.asarray(p.channels(), dtype=np.float64)
    start, _ = sc.starts()
    NV = 8 + sc.DT
    rows, rterm, dense, dterm = (np.zeros((sc.n, NV)) for _ in range(4))
    for tile, ids in sc.lists.items():
        cam, pix, px, py = _pixels(sc, tile)
        f = fwd_in[tile]
        a_out = np.asarray(f["alpha"], dtype=np.float64)
        Tf = (F(1.0) - np.asarray(f["alpha"], dtype=F)).astype(np.float64) if rounded else 1.0 - a_out
        last = np.asarray(f["last"], dtype=np.int64)
        vr = np.array(v_render[tile], dtype=np.float64)
        va = np.array(v_alpha[tile], dtype=np.float64)
        va_abs = np.abs(va)
        if sc.ed:
            vE = vr[:, -1].copy()
            vr[:, -1] = vE / np.maximum(a_out, 1e-10)
            extra = np.where(a_out > 1e-10, -vE * np.asarray(f["render"], dtype=np.float64)[:, -1] / np.maximum(a_out, 1e-10), 0.0)
            va = va + extra
            va_abs = va_abs + np.abs(extra)
        bgd, bgabs = 0.0, 0.0
        if p.bg is not None:
            bgc = np.asarray(p.bg[cam], dtype=np.float64)
            bgd, bgabs = vr[:, :sc.D] @ bgc, np.abs(vr[:, :sc.D]) @ np.abs(bgc)
        T = Tf.copy()
        Bq, Babs = -Tf * (va - bgd), Tf * (va_abs + bgabs)
        kappa = np.zeros(pix.size)
        top = int(last.max())
        for pos in range(min(top, start[tile] + ids.size - 1), start[tile] - 1, -1):
            g = int(ids[pos - start[tile]])
            dx, dy, a, b, c, o, sigma, vis, raw, alpha, ok = _entry(sc, g, px, py, params)
            valid = ok & (last >= pos)
            if not valid.any():
                continue
            alpha = np.where(valid, alpha, 0.0)
            vis = np.where(valid, vis, 0.0)
            ra = 1.0 / (1.0 - alpha)
            T = T * ra
            kappa = kappa + np.where(valid, ra, 0.0)
            fac = alpha * T
            A, Aabs = vr @ chan[g], np.abs(vr) @ np.abs(chan[g])
            v_al = A * T - ra * Bq
            mag = kappa * (Aabs * T + ra * Babs)
            Bq = Bq + fac * A
            Babs = Babs + fac * Aabs
            free = valid & (raw <= ALPHA_MAX)                 # alpha bound at 0.999: nothing through sigma or opacity
            h, hm = np.where(free, vis * v_al, 0.0), np.where(free, vis * mag, 0.0)
            u, w = a * dx + b * dy, b * dx + c * dy
            R, RT, Dn, DTm = rows[g], rterm[g], dense[g], dterm[g]
            mom = (h * dx, h * dy, HALF_LOG2E * np.abs(h * u), HALF_LOG2E * np.abs(h * w), h * dx * dx, h * dx * dy, h * dy * dy, h)
            # (u and w are sums that cancel for a slanted conic: their magnitude is |a dx| + |b dy|, not |u|)
            momt = (hm * np.abs(dx), hm * np.abs(dy), HALF_LOG2E * hm * (np.abs(a * dx) + np.abs(b * dy)),
                    HALF_LOG2E * hm * (np.abs(b * dx) + np.abs(c * dy)), hm * dx * dx,
                    hm * np.abs(dx * dy), hm * dy * dy, hm)
            for j in range(8):
                R[j] += mom[j].sum()
                RT[j] += momt[j].sum()
            col, colt = (fac[:, None] * vr).sum(axis=0), ((kappa * fac)[:, None] * np.abs(vr)).sum(axis=0)
            R[8:] += col
            RT[8:] += colt
            vs = -o * h
            Dn[0] += (vs * u).sum(); Dn[1] += (vs * w).sum()
            Dn[2] += np.abs(vs * u).sum(); Dn[3] += np.abs(vs * w).sum()
            Dn[4] += 0.5 * (vs * dx * dx).sum(); Dn[5] += (vs * dx * dy).sum(); Dn[6] += 0.5 * (vs * dy * dy).sum()
            Dn[7] += h.sum()
            Dn[8:] += col
            ao = abs(o)
            sdx, sdy = momt[0].sum(), momt[1].sum()
            DTm[0] += ao * (abs(a) * sdx + abs(b) * sdy); DTm[1] += ao * (abs(b) * sdx + abs(c) * sdy)
            DTm[2] += ao * momt[2].sum() / HALF_LOG2E; DTm[3] += ao * momt[3].sum() / HALF_LOG2E
            DTm[4] += 0.5 * ao * momt[4].sum(); DTm[5] += ao * momt[5].sum(); DTm[6] += 0.5 * ao * momt[6].sum()
            DTm[7] += hm.sum()
            DTm[8:] += colt
    return dict(rows=rows, rows_terms=rterm, dense=dense, dense_terms=dterm)


def rows_to_dense(sc, rows):
    """The identities of project_bwd.hip::rows_to_gradients: raw-moment rows -> gsplat's gradients (same column order)."""
    o = sc.opac.astype(np.float64)
    a, b, c = (sc.conics[:, k].astype(np.float64) for k in range(3))
    d = np.array(rows, dtype=np.float64)
    with np.errstate(all="ignore"):
        d[:, 0] = -o * (a * rows[:, 0] + b * rows[:, 1])
        d[:, 1] = -o * (b * rows[:, 0] + c * rows[:, 1])
        d[:, 2] = o * rows[:, 2] / HALF_LOG2E
        d[:, 3] = o * rows[:, 3] / HALF_LOG2E
        d[:, 4], d[:, 5], d[:, 6] = -0.5 * o * rows[:, 4], -o * rows[:, 5], -0.5 * o * rows[:, 6]
    return np.where((rows == 0.0).all(axis=1)[:, None], 0.0, d)      # (a NaN opacity has an all-zero row)


# ---- shared by the host and the device test -----------------------------------------------------------------------------------------
def rounded_forward(sc, fwd):
    """tile -> the float32 alpha / last_ids / render a backward call is given."""
    return {t: dict(alpha=f["alpha"].astype(F), last=f["last"].astype(np.int32), render=f["render"].astype(F)) for t, f in fwd.items()}


def cotangents(sc, fwd, seed=7):
    """Random float32 v_render / v_alpha per populated tile, ZERO on the critical pixels: those then contribute exactly nothing,
    whichever way their decisions fall."""
    rng = np.random.RandomState(seed)
    vr, va = {}, {}
    for t, f in fwd.items():
        keep = ~f["critical"]
        vr[t] = (rng.standard_normal(f["render"].shape) * keep[:, None]).astype(F)
        va[t] = (rng.standard_normal(f["alpha"].shape) * keep).astype(F)
    return vr, va


@functools.lru_cache(maxsize=None)
def reference(name):
    """(scene, forward per tile, hit_any, hit_clear, rounded forward, v_render, v_alpha, backward): computed once per scene."""
    sc = scene(name)
    fwd, hit_any, hit_clear = forward(sc)
    fin = rounded_forward(sc, fwd)
    vr, va = cotangents(sc, fwd)
    return sc, fwd, hit_any, hit_clear, fin, vr, va, backward(sc, fin, vr, va)


def worst_ratio(got, ref, terms):
    """max |got - ref| / (2^-24 sum |terms|); inf where a value with no term at all is not exactly its reference."""
    got, ref, terms = (np.asarray(v, dtype=np.float64) for v in (got, ref, terms))
    err = np.abs(got - ref)
    with np.errstate(all="ignore"):
        r = np.where(terms > 0.0, err / (EPS * terms), np.where(err == 0.0, 0.0, np.inf))
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


def device_bound(measured):
    """What a HIP kernel may differ by, in units of 2^-24 sum |terms|: four times the oracle's own distance from float64 (v_exp_f32 /
    v_rcp_f32 for libm, contraction, a tree-plus-atomic summation order: ulp-class effects)."""
    return 4.0 * max(measured, 1.0)


# The fp32 C oracle's worst |oracle - reference| / (2^-24 sum |terms|) over every gather-form scene it supports (no expected-depth
# normalisation; a NaN opacity replaced by 0, which gsplat's fminf would composite).  MEASURED by
# tests/test_blend_refs_host.py::test_oracle_within_constants -- never against a HIP kernel -- which also asserts that the oracle
# stays within them.  Measured 2026-10-20, rounded up in the second decimal:
#   forward 26.74 (the serial float32 sum over a 513-entry list) | xy 5.45, |xy| 5.45, conic 6.06, opacity 5.65, channels 9.71
ORACLE_FWD = 26.75
ORACLE_BWD = {"xy": 5.46, "xy_abs": 5.46, "conic": 6.07, "opacity": 5.66, "channels": 9.72}
