"""The gradient exchange kernels (csrc/dp.hip) called directly, in ONE process, at map, tile, capacity and sender-count edges,
against the host references of tests/dp_refs.py.  The W senders are W calls of mtgs_dp_pack_ordered into one buffer with
strides: no process group, no spawn.

What is exact (np.array_equal on bit patterns): visibility / touched / union maps, prefixes, counts and totals, wire rows, the
eleven geometry sums and the three sums of v_rgb (one float32 addition per sender in rank order from +0.0: the reference is the
expectation, not an approximation), row numbers, ids, and every form-against-form comparison (chunked against one call, sparse
against dense write, rows against dense, groups against one call per group).  Only colour against float64 has a bar:
|got - f64| <= (16 + W) * 2^-23 * S[n, c], S = sum |v_rgb| over the senders of the mask, no element excluded -- the float32
restatement alone measures 2.3 (tests/test_dp_refs_host.py keeps it below a quarter of the bar on every input set of this file),
the hardware reciprocal square root adds ~1 ulp to each of x, y, z, which a cubic with |basis| < 1 turns into at most 3, FMA
contraction only removes roundings, and a sequential sum of W terms adds at most (W - 1) / 2.  The largest measured ratio per
entry point goes to the parity report (tests/util.REPORT).

The canary rule holds for every call: every output is allocated with slack behind it and pre-filled with one NaN bit pattern;
a test asserts what was written AND that everything else still holds the pattern.  Map records are laid out with a stride larger
than the words and the prefix, and the gap is canary as well.

Input sets: SCENES lists every (N, W, mix) this file uses; scene() refuses any other, so that the host test covers them all."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import dp_refs as R

pytestmark = pytest.mark.gpu

N_LIST = (1, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 2049, 4099)
W_LIST = (1, 2, 3, 8, 33, 64)
KDEG = ((1, 0), (4, 1), (9, 2), (16, 3), (16, 1))      # (the last: zero coefficients above (degree + 1)^2)
PATTERNS = ("all", "random", "altwords", "block2", "bit63", "none", "bit0", "bit31", "bit32", "bit64", "bitlast")
MIXES = {"mixed": PATTERNS, "full": ("all",), "random": ("random",), "disjoint": ("disjoint",)}
SCENES = tuple([(N, W, "mixed") for W in W_LIST for N in N_LIST]
               + [(N, W, "full") for W in (3, 8, 64) for N in (33, 1025)]          # every sender full in the same tile
               + [(N, 8, "random") for N in (1025, 4099)]
               + [(4099, 8, "disjoint"), (16449, 3, "random")])
CAN = 0x7FC0DEAD                                         # a quiet NaN with a payload nobody computes
SL = 3                                                   # slack rows behind every output
RATIOS = {}                                              # entry point -> largest |got - f64| / (2^-23 S)


# ---- input builders (numpy only: tests/test_dp_refs_host.py imports them) --------------------------------------------------------
def pattern_flags(name, N, rng, r=0, W=1):
    n = np.arange(N)
    if name == "none":
        return np.zeros(N, dtype=bool)
    if name == "all":
        return np.ones(N, dtype=bool)
    if name.startswith("bit"):
        at = N - 1 if name == "bitlast" else min(int(name[3:]), N - 1)
        return n == at
    if name == "altwords":                               # full and empty words alternating
        return (n // 64) % 2 == 0
    if name == "block2":                                 # a full 1024 block behind an empty one
        return (n >= 1024) & (n < 2048)
    if name == "disjoint":
        return n % W == r
    assert name == "random"
    return rng.random(N) < 0.15


@functools.lru_cache(maxsize=None)
def _scene(N, W, mix):
    rng = np.random.default_rng(N * 131 + W * 7 + len(mix))
    f32 = lambda *s: rng.standard_normal(s).astype(np.float32)
    means = rng.uniform(-1.0, 1.0, (N, 3)).astype(np.float32)
    d = rng.standard_normal((W, 3))
    cams = (3.0 * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)      # |mean - cam| >= 3 - sqrt(3)
    pats = MIXES[mix]
    flags = np.stack([pattern_flags(pats[r % len(pats)], N, rng, r, W) for r in range(W)])
    grads = {"v_means": f32(W, N, 3), "v_quats": f32(W, N, 4), "v_scales": f32(W, N, 3), "v_opacities": f32(W, N), "v_rgb": f32(W, N, 3)}
    # radii: > 0 is visible; 0 and negative values are not
    radii = np.where(flags, rng.integers(1, 9, (W, N)), -rng.integers(0, 2, (W, N))).astype(np.int32)
    senders = [(flags[r], R.pack_rows(flags[r], *(grads[k][r] for k in ("v_means", "v_quats", "v_scales", "v_opacities", "v_rgb"))))
               for r in range(W)]
    return {"N": N, "W": W, "means": means, "cams": cams, "flags": flags, "grads": grads, "radii": radii, "senders": senders}


def scene(N, W, mix):
    assert (N, W, mix) in SCENES, (N, W, mix)
    return _scene(N, W, mix)


def touched_input(N, r=0):
    """Wire rows of one sender, most of them without a gradient: zero rows (Gaussian 0 among them), a row of -0.0 only, a row
    whose only non-zero word is the pad, and a row that is NaN in one word and zero elsewhere.  r = 0: the sender sees every
    Gaussian (row j is Gaussian j); r = 2: every other word of Gaussians (row j is NOT Gaussian j behind the first word)."""
    sc = scene(N, 33, "mixed")
    rows = sc["senders"][r][1].copy()
    n = rows.shape[0]
    rng = np.random.default_rng(N + r)
    rows[rng.random(n) < 0.6, :14] = 0.0
    rows[0, :14] = 0.0
    special = {}
    for j, kind in zip((n // 2, n // 3 + 1, n - 1), ("negzero", "pad", "nan")):
        if 0 < j < n and j not in special:
            special[j] = kind
            rows[j, :14] = 0.0
            if kind == "negzero":
                rows[j, :14] = -0.0
            elif kind == "pad":
                rows[j, 14] = 1.0
            else:
                rows[j, 5] = np.nan
    return rows, special


# ---- device helpers ---------------------------------------------------------------------------------------------------------------
def _call(name, *a):
    from mtgs_amd import _lib
    _lib.call(name, *a)


def _st(t):
    from mtgs_amd import _lib
    return _lib.stream_of(t)


def can(n):
    return torch.full((int(n),), CAN, dtype=torch.int32, device="cuda")


def u32(t):
    return t.detach().contiguous().cpu().view(torch.int32).numpy().view(np.uint32).copy()


def fb(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def is_can(a):
    return bool((np.asarray(a) == CAN).all())


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Dev:
    """The W senders of a scene on the device: W calls of mtgs_dp_pack_ordered into one map buffer (record r at r * stride_b:
    words | prefix | canary gap) and one row buffer (sender r at r * row_stride floats)."""

    def __init__(self, sc, pad_rows=0, gap=40):
        N, W = sc["N"], sc["W"]
        self.sc, self.N, self.W, self.nw = sc, N, W, R.n_words(N)
        self.stride_b = -(-(12 * self.nw + gap) // 8) * 8
        self.maps = can(W * self.stride_b // 4 + 8)
        self.n_rows = [rows.shape[0] for _, rows in sc["senders"]]
        self.cap = max(max(self.n_rows), 1) + pad_rows
        self.row_stride = self.cap * 16
        self.rows = can(W * self.row_stride + 64)
        self.counts = can(W + 2)
        self.means, self.cams = up(sc["means"]), up(sc["cams"])
        self.g = {k: up(v) for k, v in sc["grads"].items()}
        self.radii = up(sc["radii"])
        self.blocks = can(N // 1024 + 2)
        for r in range(W):
            self.pack(r, self.words_ptr(r), self.prefix_ptr(r), self.counts.data_ptr() + 4 * r,
                      self.rows.data_ptr() + 4 * r * self.row_stride, self.cap)

    def pack(self, r, words, prefix, count, rows, capacity, rgb=True):
        g = self.g
        _call("mtgs_dp_pack_ordered", self.N, self.radii[r].data_ptr(), g["v_means"][r].data_ptr(), g["v_quats"][r].data_ptr(),
              g["v_scales"][r].data_ptr(), g["v_opacities"][r].data_ptr(), g["v_rgb"][r].data_ptr() if rgb else None, words, prefix,
              count, self.blocks.data_ptr(), rows, capacity, _st(self.rows))

    def words_ptr(self, r):
        return self.maps.data_ptr() + r * self.stride_b

    def prefix_ptr(self, r):
        return self.words_ptr(r) + 8 * self.nw

    def check(self):
        """Maps, counts and rows of every sender against the references; every other word is canary."""
        maps, rows, counts = u32(self.maps), u32(self.rows), u32(self.counts)
        nw, q = self.nw, self.stride_b // 4
        for r, (flags, want) in enumerate(self.sc["senders"]):
            words, prefix, count = R.vis_map(flags)
            rec = maps[r * q:(r + 1) * q]
            assert np.array_equal(rec[:2 * nw].view(np.uint64), words), r
            assert np.array_equal(rec[2 * nw:3 * nw], prefix), r
            assert is_can(rec[3 * nw:]), r
            assert counts[r] == count == want.shape[0], r
            mine = rows[r * self.row_stride:(r + 1) * self.row_stride].reshape(-1, 16)
            assert np.array_equal(mine[:count], fb(want)), r
            assert is_can(mine[count:]), r
        assert is_can(maps[self.W * q:]) and is_can(rows[self.W * self.row_stride:]) and is_can(counts[self.W:])

    def chunk_rows(self, g_begin, pad_rows=0):
        """A row buffer for a range that begins at g_begin: sender r's rows from ITS first row of the range to its last row."""
        first = [int(R.vis_map(f)[1][g_begin // 64]) for f, _ in self.sc["senders"]]
        cap = max(max(n - f for n, f in zip(self.n_rows, first)), 1) + pad_rows
        buf = can(self.W * cap * 16 + 64)
        src = self.rows[:self.W * self.row_stride].view(self.W, self.cap, 16)
        dst = buf[:self.W * cap * 16].view(self.W, cap, 16)
        for r in range(self.W):
            n = self.n_rows[r] - first[r]
            dst[r, :n] = src[r, first[r]:self.n_rows[r]]
        return buf, cap * 16


def run_reduce(D, K, degree, entry="reduce", mask=~0, wg=1, T=1, t=0, row_cap=0, g_begin=0, g_end=-1, rows=None, row_stride=None,
               out=None, W=None):
    N = D.N
    if out is None:
        out = {"vm": can((N + SL) * 3), "vq": can((N + SL) * 4), "vs": can((N + SL) * 3), "vo": can(N + SL), "vc": can((N + SL) * T * K * 3)}
    head = (D.W if W is None else W, N, K, degree, D.means.data_ptr(), D.words_ptr(0), D.prefix_ptr(0), D.stride_b,
            (D.rows if rows is None else rows).data_ptr(), D.row_stride if row_stride is None else row_stride)
    tail = (D.cams.data_ptr(), out["vm"].data_ptr(), out["vq"].data_ptr(), out["vs"].data_ptr(), out["vo"].data_ptr(),
            out["vc"].data_ptr() + 4 * t * K * 3, g_begin, g_end)
    more = (C.c_uint64(mask & (2 ** 64 - 1)), wg, T * K * 3)
    if entry == "reduce":
        assert T == 1 and wg == 1
        _call("mtgs_dp_reduce", *head, *tail, _st(D.rows))
    elif entry == "slices":
        _call("mtgs_dp_reduce_slices", *head, *tail, *more, _st(D.rows))
    else:
        _call("mtgs_dp_reduce_slices_cap", *head, row_cap, *tail, *more, _st(D.rows))
    return out


def host(out, N, T, K):
    return {"vm": u32(out["vm"]).reshape(N + SL, 3), "vq": u32(out["vq"]).reshape(N + SL, 4), "vs": u32(out["vs"]).reshape(N + SL, 3),
            "vo": u32(out["vo"]).reshape(N + SL, 1), "vc": u32(out["vc"]).reshape(N + SL, T, K, 3)}


GEO = (("vm", 0, 3), ("vq", 3, 7), ("vs", 7, 10), ("vo", 10, 11))


def note_ratio(entry, got, want, S, W):
    """The colour bar on every element; remembers the largest error in units of 2^-23 S."""
    err = np.abs(got.astype(np.float64) - want)
    Sb = np.broadcast_to(S[:, None, :], err.shape)
    bar = R.colour_bar(W, Sb)
    ok = err <= bar                                       # (a NaN fails)
    assert ok.all(), (entry, int((~ok).sum()), float((err / np.maximum(bar, 1e-300)).max()))
    if (Sb > 0).any():
        RATIOS[entry] = max(RATIOS.get(entry, 0.0), float((err[Sb > 0] / (R.EPS * Sb[Sb > 0])).max()))


def check_dense(entry, h, sc, K, degree, mask=~0, wg=1, T=1, t=0, row_cap=None, written=None):
    """h: host(outputs).  written[N] bool: the Gaussians this call had to write (default all); the others, the slack and the
    other slices keep the canary."""
    N, W = sc["N"], sc["W"]
    mask &= (1 << W) - 1
    written = np.ones(N, dtype=bool) if written is None else written
    geo = R.reduce_geometry_f32(sc["senders"], N, row_cap)
    for name, a, b in GEO:
        if wg & 1:
            assert np.array_equal(h[name][:N][written], fb(geo[:, a:b])[written]), (entry, name)
            assert is_can(h[name][:N][~written]) and is_can(h[name][N:]), (entry, name)
        else:
            assert is_can(h[name]), (entry, name)
    want, S = R.reduce_colour_f64(sc["senders"], sc["means"], sc["cams"], K, degree, mask, row_cap)
    vc = h["vc"]
    got = vc[:N, t][written].view(np.float32)
    note_ratio(entry, got, want[written], S[written], W)
    nb = (degree + 1) ** 2
    assert (got[:, nb:] == 0).all(), entry
    others = [s for s in range(T) if s != t]
    assert is_can(vc[:N][~written]) and is_can(vc[N:]) and is_can(vc[:N, others]), entry
    return geo


@pytest.fixture(scope="module", autouse=True)
def _report_colour_ratios():
    yield
    from tests.util import REPORT
    for entry, ratio in sorted(RATIOS.items()):
        unit = "" if "share" in entry else ": largest |got - float64| in units of 2^-23 * sum |v_rgb| (bar: 16 + W)"
        REPORT.append({"kind": "dp_colour", "name": entry + unit, "ratio": ratio})


# ---- mtgs_dp_pack_ordered / mtgs_dp_pack --------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", N_LIST)
@pytest.mark.parametrize("pad_rows", [0, 5])
def test_pack_ordered_maps_and_rows(hip_lib, N, pad_rows):
    """Every visibility pattern (33 senders cycle through the eleven of PATTERNS): words, prefix, count and rows bit for bit, the
    gap of the map record, the rows behind the count and the slack untouched; row_stride exact and padded."""
    D = Dev(scene(N, 33, "mixed"), pad_rows=pad_rows)
    torch.cuda.synchronize()
    D.check()


@pytest.mark.parametrize("N", [1, 33, 64, 1025, 4099])
def test_pack_ordered_capacity_and_null_rgb(hip_lib, N):
    """capacity = count, count - 1 and 0: nothing is written past it and the count still gives the total; v_rgb = NULL: zeros."""
    sc = scene(N, 33, "mixed")
    D = Dev(sc)
    nw = D.nw
    for r in (0, 1, 2, 4):                               # all, random, alternating words, one bit
        flags, want = sc["senders"][r]
        words, prefix, count = R.vis_map(flags)
        for capacity, rgb in ((count, False), (count - 1, True), (0, True)):
            if capacity < 0:
                continue
            m, rows, cnt = can(3 * nw + 6), can((count + SL) * 16), can(3)
            D.pack(r, m.data_ptr(), m.data_ptr() + 8 * nw, cnt.data_ptr(), rows.data_ptr(), capacity, rgb=rgb)
            m, rows, cnt = u32(m), u32(rows).reshape(-1, 16), u32(cnt)
            assert np.array_equal(m[:2 * nw].view(np.uint64), words) and np.array_equal(m[2 * nw:3 * nw], prefix) and is_can(m[3 * nw:])
            assert cnt[0] == count and is_can(cnt[1:])
            exp = want.copy()
            if not rgb:
                exp[:, 11:14] = 0.0
            assert np.array_equal(rows[:capacity], fb(exp)[:capacity]) and is_can(rows[capacity:]), (r, capacity)


@pytest.mark.parametrize("N", N_LIST)
def test_pack_unordered_equals_ordered_after_sorting(hip_lib, N):
    sc = scene(N, 33, "mixed")
    D = Dev(sc)
    for r in range(11):
        flags, want = sc["senders"][r]
        count = want.shape[0]
        for capacity in {count, max(count - 1, 0)}:
            rows, cnt = can((count + SL) * 16), can(4)
            g = D.g
            _call("mtgs_dp_pack", N, D.radii[r].data_ptr(), g["v_means"][r].data_ptr(), g["v_quats"][r].data_ptr(),
                  g["v_scales"][r].data_ptr(), g["v_opacities"][r].data_ptr(), g["v_rgb"][r].data_ptr(), rows.data_ptr(), capacity,
                  cnt.data_ptr(), _st(rows))
            rows, cnt = u32(rows).reshape(-1, 16), u32(cnt)
            assert cnt[:2].view(np.int64)[0] == count and is_can(cnt[2:])
            assert is_can(rows[capacity:]), (r, capacity)
            got = rows[:capacity]
            got = got[np.argsort(got[:, 15].view(np.int32), kind="stable")]
            if capacity == count:
                assert np.array_equal(got, fb(want)), r
            else:                                        # count - 1 distinct rows of the sender, each bit for bit
                idx = got[:, 15].view(np.int32)
                assert len(set(idx.tolist())) == capacity and flags[idx].all()
                assert np.array_equal(got, fb(want)[np.searchsorted(np.flatnonzero(flags), idx)]), r


def test_pack_of_nothing(hip_lib):
    cnt, cnt64 = can(3), can(4)
    x = can(64)
    p = x.data_ptr()
    _call("mtgs_dp_pack_ordered", 0, p, p, p, p, p, p, p, p, cnt.data_ptr(), p, p, 4, _st(x))
    _call("mtgs_dp_pack", 0, p, p, p, p, p, p, p, 4, cnt64.data_ptr(), _st(x))
    assert u32(cnt)[0] == 0 and is_can(u32(cnt)[1:]) and not u32(cnt64)[:2].any() and is_can(u32(cnt64)[2:]) and is_can(u32(x))


def test_pack_ordered_second_trip_of_the_block_count_loop(hip_lib):
    """N = 1024 * 1025 + 1: blocks 1025 and 1026 sum more than 1024 block counts in front of them.  One Gaussian in 97 visible."""
    N = 1024 * 1025 + 1
    n = np.arange(N)
    flags = n % 97 == 0
    val = lambda c, k: ((n[:, None] * c + np.arange(c)[None] + k) % 8191).astype(np.float32) - 4000.0
    vm, vq, vs, vo, vr = val(3, 0), val(4, 11), val(3, 23), val(1, 37)[:, 0].copy(), val(3, 41)
    words, prefix, count = R.vis_map(flags)
    want = R.pack_rows(flags, vm, vq, vs, vo, vr)
    nw = R.n_words(N)
    m, rows, cnt, blocks = can(3 * nw + 6), can((count + SL) * 16), can(3), can(N // 1024 + 3)
    dev = [up(a) for a in (flags.astype(np.int32), vm, vq, vs, vo, vr)]
    _call("mtgs_dp_pack_ordered", N, *(a.data_ptr() for a in dev), m.data_ptr(), m.data_ptr() + 8 * nw, cnt.data_ptr(),
          blocks.data_ptr(), rows.data_ptr(), count, _st(rows))
    m, rows, cnt = u32(m), u32(rows).reshape(-1, 16), u32(cnt)
    assert cnt[0] == count and count * 64 < 1 << 20
    assert np.array_equal(m[:2 * nw].view(np.uint64), words) and np.array_equal(m[2 * nw:3 * nw], prefix) and is_can(m[3 * nw:])
    assert np.array_equal(rows[:count], fb(want)) and is_can(rows[count:])


# ---- mtgs_dp_touched_pack / mtgs_dp_touched_pack_chunks -------------------------------------------------------------------------
def run_touched(rows_np, N, n_rows, capacity, chunks=None):
    """chunks: (begin, cap) -> mtgs_dp_touched_pack_chunks.  Returns the host views of everything the call may write."""
    from mtgs_amd import _abi
    nw = R.n_words(N)
    src = up(rows_np) if rows_np.size else can(16).view(torch.float32)
    o = {"words": can(2 * nw + 4), "prefix": can(nw + 3), "count": can(3), "totals": can(4), "overflow": can(3)}
    scratch, blocks = can(2 * nw + 4), can(nw // 256 + 3)
    head = (n_rows, src.data_ptr(), N, scratch.data_ptr(), o["words"].data_ptr(), o["prefix"].data_ptr(), o["count"].data_ptr(),
            o["totals"].data_ptr(), blocks.data_ptr())
    if chunks is None:
        o["rows"] = can((capacity + SL) * 16)
        _call("mtgs_dp_touched_pack", *head, o["rows"].data_ptr(), capacity, _st(src))
    else:
        begin, cap = chunks
        tab = np.zeros(1, dtype=_abi.struct_dtype("mtgs_dp_chunks"))
        tab["n"] = len(cap)
        tab["begin"][0, :len(begin)] = begin
        bufs = [can((max(c, 0) + SL) * 16) for c in cap]
        for c in range(min(len(cap), 16)):
            tab["rows"][0, c], tab["cap"][0, c] = bufs[c].data_ptr(), cap[c]
        _call("mtgs_dp_touched_pack_chunks", *head, tab.ctypes.data, o["overflow"].data_ptr(), _st(src))
        o["chunks"] = bufs
    torch.cuda.synchronize()
    h = {k: u32(v) for k, v in o.items() if k != "chunks"}
    if chunks is not None:
        h["chunks"] = [u32(b).reshape(-1, 16) for b in o["chunks"]]
    return h


def check_touched_map(h, flags, N):
    nw = R.n_words(N)
    words, prefix, count = R.vis_map(flags)
    assert np.array_equal(h["words"][:2 * nw].view(np.uint64), words) and is_can(h["words"][2 * nw:])
    assert np.array_equal(h["prefix"][:nw], prefix) and is_can(h["prefix"][nw:])
    assert h["count"][0] == count and is_can(h["count"][1:])
    assert h["totals"][:2].view(np.int64)[0] == count << 32 and is_can(h["totals"][2:])
    return count


@pytest.mark.parametrize("r", [0, 2])
@pytest.mark.parametrize("N", N_LIST)
def test_touched_pack(hip_lib, N, r):
    """Only the rows that carry a gradient survive, in order, with their own map: the -0.0 row, the pad-only row and the zero row
    of Gaussian 0 are dropped, the NaN row is kept; a capacity cut; n_rows = 0."""
    rows, special = touched_input(N, r)
    n_rows, idx = rows.shape[0], R.row_index(rows)
    kept, flags = R.touched(rows, N)
    for j, kind in special.items():
        assert flags[idx[j]] == (kind == "nan"), (j, kind)
    assert idx[0] == 0 and not flags[0]
    count = kept.shape[0]
    for capacity in {count, max(count - 1, 0), count // 2}:
        h = run_touched(rows, N, n_rows, capacity)
        assert check_touched_map(h, flags, N) == count
        got = h["rows"].reshape(-1, 16)
        assert np.array_equal(got[:capacity], fb(kept)[:capacity]) and is_can(got[capacity:]), capacity
    h = run_touched(rows, N, 0, 4)
    assert check_touched_map(h, np.zeros(N, dtype=bool), N) == 0 and is_can(h["rows"])


def _bounds(N, n):
    nw = R.n_words(N)
    return [0] + [64 * ((c * nw) // n) for c in range(1, n)] + [N]


@pytest.mark.parametrize("n", [1, 4, 16])
@pytest.mark.parametrize("N", [65, 1025, 4099])
def test_touched_pack_chunks(hip_lib, N, n):
    """The same compaction into n chunks of the index range (empty chunks included: N = 65 has two words): the map is the whole
    range's, the concatenated chunks equal the unchunked rows; one chunk's cap exceeded by one -> overflow = 1, that chunk lacks
    exactly its last row, the others are intact."""
    rows, _ = touched_input(N, 2 if N > 65 else 0)
    n_rows = rows.shape[0]
    kept, flags = R.touched(rows, N)
    begin = _bounds(N, n)
    whole = run_touched(rows, N, n_rows, kept.shape[0])["rows"].reshape(-1, 16)[:kept.shape[0]]
    assert np.array_equal(whole, fb(kept))
    full, _ = R.chunk_split(kept, begin, [N] * n)
    sizes = [c.shape[0] for c in full]
    assert n == 1 or N > 65 or 0 in sizes                # (empty chunks: N = 65 has two words; at N = 1025, n = 16 every other one)
    victim = int(np.argmax(sizes))
    for caps in (sizes, [s - (c == victim) for c, s in enumerate(sizes)]):
        want, overflow = R.chunk_split(kept, begin, caps)
        h = run_touched(rows, N, n_rows, 0, chunks=(begin, caps))
        check_touched_map(h, flags, N)
        assert h["overflow"][0] == overflow == int(caps is not sizes) and is_can(h["overflow"][1:])
        for c in range(n):
            assert np.array_equal(h["chunks"][c][:caps[c]], fb(want[c])) and is_can(h["chunks"][c][caps[c]:]), c
        if not overflow:
            assert np.array_equal(np.concatenate([h["chunks"][c][:caps[c]] for c in range(n)]), whole)


@pytest.mark.parametrize("begin,caps", [([0, 100, 4099], [9, 9]), ([0, 128, 64, 4099], [9, 9, 9]), ([0, 128, 4098], [9, 9]),
                                        ([0, 128, 4100], [9, 9]), ([64, 128, 4099], [9, 9]), ([0], []),
                                        (_bounds(4099, 16) + [4099], [9] * 17)])
def test_touched_pack_chunks_refuses_bad_tables(hip_lib, begin, caps):
    rows, _ = touched_input(4099)
    with pytest.raises(RuntimeError, match="mtgs_dp_touched_pack_chunks"):
        run_touched(rows, 4099, 4099, 0, chunks=(begin[:17], caps))


# ---- mtgs_dp_union ------------------------------------------------------------------------------------------------------------------
class Union:
    def __init__(self, W, N, words_ptr, stride_b, masks, ref_words):
        nw, P = R.n_words(N), len(masks)
        self.nw, self.masks = nw, masks
        self.uw, self.up, self.totals = can(2 * P * nw + 4), can(P * nw + 3), can(2 * P + 2)
        self.blocks = can(P * (nw // 256 + 1) + 2)
        self.m = up(np.asarray([m & (2 ** 64 - 1) for m in masks], dtype=np.uint64).view(np.int64))
        _call("mtgs_dp_union", W, N, words_ptr, stride_b, P, self.m.data_ptr(), self.uw.data_ptr(), self.up.data_ptr(),
              self.totals.data_ptr(), self.blocks.data_ptr(), _st(self.uw))
        self.words, self.prefix, self.tot = R.union(ref_words, masks)
        self.counts = [int(t >> 32) for t in self.tot]

    def check(self):
        nw, P = self.nw, len(self.masks)
        uw, upf, tot = u32(self.uw), u32(self.up), u32(self.totals)
        assert np.array_equal(uw[:2 * P * nw].view(np.uint64).reshape(P, nw), self.words) and is_can(uw[2 * P * nw:])
        assert np.array_equal(upf[:P * nw].reshape(P, nw), self.prefix) and is_can(upf[P * nw:])
        assert np.array_equal(tot[:2 * P].view(np.int64), self.tot) and is_can(tot[2 * P:])

    def words_ptr(self, p):
        return self.uw.data_ptr() + 8 * self.nw * p

    def prefix_ptr(self, p):
        return self.up.data_ptr() + 4 * self.nw * p


def union_of(D, masks):
    return Union(D.W, D.N, D.words_ptr(0), D.stride_b, masks, np.stack([R.words_of(f) for f, _ in D.sc["senders"]]))


@pytest.mark.parametrize("N,W,mix", [(1, 1, "mixed"), (33, 3, "full"), (65, 64, "mixed"), (1025, 64, "full"), (4099, 8, "disjoint"),
                                     (4099, 64, "mixed"), (4099, 33, "mixed"), (16449, 3, "random")])
def test_union_maps(hip_lib, N, W, mix):
    """Subsets: none (empty words, total 0), one sender, all, the last sender alone (bit 63 at W = 64), overlapping subsets; the
    senders identical ("full"), disjoint and mixed; N = 16449 is 258 words: one 256-word block and a bit."""
    D = Dev(scene(N, W, mix))
    allm = (1 << W) - 1
    masks = [0, 1, allm, 1 << (W - 1), allm & 0x5555555555555555, allm & 0x0F0F0F0F0F0F0F3F, allm & ~1]
    U = union_of(D, masks)
    torch.cuda.synchronize()
    U.check()
    assert U.counts[0] == 0 and not U.words[0].any()
    assert U.counts[2] == int(np.logical_or.reduce(D.sc["flags"]).sum())


def test_union_second_trip_of_the_block_count_loop(hip_lib):
    """N = 64 * 256 * 257 + 1: 258 blocks of 256 words, so the last blocks sum more than 256 counts in front of them.  Words only."""
    N, W = 64 * 256 * 257 + 1, 2
    nw = R.n_words(N)
    rng = np.random.default_rng(5)
    words = (rng.integers(0, 2 ** 63, (W, nw), dtype=np.int64).astype(np.uint64) << np.uint64(1)) & \
        rng.integers(0, 2 ** 63, (W, nw), dtype=np.int64).astype(np.uint64)
    words[:, -1] = 1                                     # (bits at positions >= N are zero in a map)
    stride_b = 8 * nw + 48
    buf = can(W * stride_b // 4 + 4)
    for r in range(W):
        buf[r * stride_b // 4:r * stride_b // 4 + 2 * nw] = up(words[r].view(np.int32))
    U = Union(W, N, buf.data_ptr(), stride_b, [3, 2, 0], words)
    torch.cuda.synchronize()
    U.check()
    assert U.counts[0] > 500_000 and nw * 8 < 600_000


# ---- mtgs_dp_reduce / _slices / _slices_cap ------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", W_LIST)
def test_reduce_every_size(hip_lib, W):
    """Dense sums at every N of N_LIST: geometry bit for bit (exactly +0.0 where no sender has a row), colour within the bar, the
    slack untouched; the three entry points and the (K, degree) pairs take turns."""
    for i, N in enumerate(N_LIST):
        sc = scene(N, W, "mixed")
        D = Dev(sc, pad_rows=i % 2)
        K, degree = KDEG[i % len(KDEG)]
        entry = ("reduce", "slices", "cap")[i % 3]
        h = host(run_reduce(D, K, degree, entry), N, 1, K)
        geo = check_dense({"reduce": "mtgs_dp_reduce", "slices": "mtgs_dp_reduce_slices", "cap": "mtgs_dp_reduce_slices_cap"}[entry], h, sc, K,
                          degree)
        nobody = ~np.logical_or.reduce(sc["flags"])
        assert not fb(geo)[nobody].any() and not h["vm"][:N][nobody].any() and not h["vc"][:N][nobody].any()


@pytest.mark.parametrize("K,degree", KDEG)
@pytest.mark.parametrize("N,W,mix", [(1025, 3, "full"), (33, 8, "full"), (1025, 64, "full"), (4099, 8, "random"), (4099, 33, "mixed")])
def test_reduce_colour_degrees(hip_lib, N, W, mix, K, degree):
    """Every (K, degree) pair; "full": every sender has all 32 rows of every tile, so all eight steps of a tile run."""
    sc = scene(N, W, mix)
    h = host(run_reduce(Dev(sc), K, degree), N, 1, K)
    check_dense("mtgs_dp_reduce", h, sc, K, degree)


@pytest.mark.parametrize("N,W,mix", [(65, 2, "mixed"), (1025, 8, "random"), (2049, 64, "mixed"), (4099, 33, "mixed")])
def test_reduce_slices_masks_and_strides(hip_lib, N, W, mix):
    """coeff_stride = T K 3 with a slice offset (the other slices keep the canary); coeff_mask none / one bit / the last sender
    (bit 63 at W = 64) / all; write_geometry = 0 leaves the geometry canary; the sparse write (bit 1) into canary-filled outputs
    writes exactly the Gaussians some sender has a row for, with the values of the dense write."""
    sc = scene(N, W, mix)
    D = Dev(sc)
    K, degree, T = 9, 2, 3
    anyone = np.logical_or.reduce(sc["flags"])
    for j, mask in enumerate((0, 1, 1 << (W - 1), (1 << W) - 1, ~0)):
        t, wg = j % T, int(j % 2 == 0)
        h = host(run_reduce(D, K, degree, "slices", mask=mask, wg=wg, T=T, t=t), N, T, K)
        check_dense("mtgs_dp_reduce_slices", h, sc, K, degree, mask=mask, wg=wg, T=T, t=t)
        hs = host(run_reduce(D, K, degree, "cap", mask=mask, wg=wg | 2, T=T, t=t), N, T, K)
        check_dense("mtgs_dp_reduce_slices_cap", hs, sc, K, degree, mask=mask, wg=wg, T=T, t=t, written=anyone)
        for name in ("vm", "vq", "vs", "vo", "vc"):      # same values as the dense write
            assert np.array_equal(hs[name][:N][anyone], h[name][:N][anyone]), name


@pytest.mark.parametrize("N,W,mix", [(1025, 3, "full"), (1025, 8, "random"), (4099, 33, "mixed")])
def test_reduce_row_cap(hip_lib, N, W, mix):
    """row_cap: the rows a sender's block HOLDS.  The block stride is larger and what lies behind the rows is all-one bits (map
    words of a dense map are): never summed.  Caps: the exact largest count, one less, inside a tile (40 of the first 64 rows of
    a full sender), at a tile's first row (64, 32), one row; 0 = the whole block.  The sums exclude exactly the rows at
    positions >= row_cap.  (The garbage keeps the Gaussian index of the row it replaces, so that a kernel that did read it would
    add a NaN to that Gaussian instead of indexing its accumulators with it.)"""
    sc = scene(N, W, mix)
    D = Dev(sc, pad_rows=7)
    top = max(D.n_rows)
    K, degree = 16, 3
    for cap in (top, top - 1, 40, 64, 32, 1, 0):
        if cap > top:
            continue
        rows = D.rows.clone()
        held = D.cap if cap == 0 else cap
        blockv = rows[:W * D.row_stride].view(W, D.cap, 16)
        blockv[:, held:, :15] = -1                       # 0xffffffff: a NaN as a float (the index word stays: a sum would show)
        h = host(run_reduce(D, K, degree, "cap", row_cap=cap, rows=rows), N, 1, K)
        check_dense("mtgs_dp_reduce_slices_cap", h, sc, K, degree, row_cap=None if cap == 0 else cap)
    with pytest.raises(RuntimeError, match="row_cap"):
        run_reduce(D, K, degree, "cap", row_cap=D.cap + 1)


@pytest.mark.parametrize("N,W,mix", [(1025, 3, "full"), (4099, 8, "random"), (4099, 64, "mixed"), (2049, 33, "mixed")])
def test_reduce_ranges(hip_lib, N, W, mix):
    """[g_begin, g_end): chunk calls with every sender's rows starting at ITS first row of the chunk reproduce the one-call result
    bit for bit; a range that ends inside a word or a tile writes nothing at or behind g_end; a g_begin off a word boundary raises."""
    sc = scene(N, W, mix)
    D = Dev(sc)
    K, degree = 16, 3
    one = host(run_reduce(D, K, degree), N, 1, K)
    check_dense("mtgs_dp_reduce", one, sc, K, degree)
    for n_chunks in (2, 5):
        begin = _bounds(N, n_chunks)
        out = None
        for c in range(n_chunks):
            rows, stride = D.chunk_rows(begin[c], pad_rows=c % 2)
            out = run_reduce(D, K, degree, "slices", g_begin=begin[c], g_end=begin[c + 1], rows=rows, row_stride=stride, out=out)
        h = host(out, N, 1, K)
        for name in one:
            assert np.array_equal(h[name], one[name]), (n_chunks, name)
    for g_begin in (0, 64, 64 * (R.n_words(N) // 2)):
        rows, stride = D.chunk_rows(g_begin)
        for size in (1, 31, 32, 33, 64):
            g_end = g_begin + size
            assert g_end < N
            h = host(run_reduce(D, K, degree, "slices", g_begin=g_begin, g_end=g_end, rows=rows, row_stride=stride), N, 1, K)
            inside = (np.arange(N) >= g_begin) & (np.arange(N) < g_end)
            for name in one:
                assert np.array_equal(h[name][:N][inside], one[name][:N][inside]), (g_begin, size, name)
                assert is_can(h[name][:N][~inside]) and is_can(h[name][N:]), (g_begin, size, name)
    for entry in ("reduce", "slices", "cap"):
        with pytest.raises(RuntimeError, match="multiple of 64"):
            run_reduce(D, K, degree, entry, g_begin=32, g_end=128)


def test_more_than_64_senders_are_refused(hip_lib):
    sc = scene(65, 64, "mixed")
    D = Dev(sc)
    for entry in ("reduce", "slices", "cap"):
        with pytest.raises(RuntimeError, match=r"code 4"):
            run_reduce(D, 4, 1, entry, W=65)
    U = union_of(D, [1, 3])
    x = can(64)
    p = x.data_ptr()
    rows_args = (65, D.N, 4, 1, D.means.data_ptr(), D.words_ptr(0), D.prefix_ptr(0), D.stride_b, D.rows.data_ptr(), D.row_stride,
                 D.cams.data_ptr(), 0, -1)
    with pytest.raises(RuntimeError, match=r"code 4"):
        _call("mtgs_dp_reduce_rows", *rows_args, C.c_uint64(1), p, U.words_ptr(0), U.prefix_ptr(0), p, p, 1, p, U.words_ptr(1),
              U.prefix_ptr(1), p, 1, 12, _st(x))
    with pytest.raises(RuntimeError, match=r"code 4"):
        _call("mtgs_dp_reduce_rows_groups", *rows_args, 1, p, p, U.words_ptr(0), U.prefix_ptr(0), p, p, 1, 12, _st(x))
    with pytest.raises(RuntimeError, match="mtgs_dp_union"):
        _call("mtgs_dp_union", 65, D.N, D.words_ptr(0), D.stride_b, 1, U.m.data_ptr(), p, p, p, p, _st(x))
    torch.cuda.synchronize()
    assert is_can(u32(x))


# ---- row outputs: mtgs_dp_reduce_rows / mtgs_dp_reduce_rows_groups ---------------------------------------------------------------
def row_buffers(N, geo_cap, coef_cap, coef_stride):
    return {"geo_rows": can((geo_cap + SL) * 16), "geo_row_of": can(N + SL), "geo_ids": can(geo_cap + SL),
            "coef_rows": can((coef_cap + SL) * coef_stride), "coef_row_of": can(N + SL)}


def run_rows(D, U, K, degree, mask, sub, b, geo=True, coef=True, geo_cap=0, coef_cap=0, coef_stride=0, g_begin=0, g_end=-1):
    z = lambda name, on: b[name].data_ptr() if on else None
    _call("mtgs_dp_reduce_rows", D.W, D.N, K, degree, D.means.data_ptr(), D.words_ptr(0), D.prefix_ptr(0), D.stride_b, D.rows.data_ptr(),
          D.row_stride, D.cams.data_ptr(), g_begin, g_end, C.c_uint64(mask & (2 ** 64 - 1)), z("geo_rows", geo), U.words_ptr(0),
          U.prefix_ptr(0), z("geo_row_of", geo), z("geo_ids", geo), geo_cap, z("coef_rows", coef), U.words_ptr(sub), U.prefix_ptr(sub),
          z("coef_row_of", coef), coef_cap, coef_stride, _st(D.rows))


@pytest.mark.parametrize("N,W,mix", [(1, 1, "mixed"), (33, 3, "full"), (65, 64, "mixed"), (1025, 8, "random"), (4099, 8, "disjoint"),
                                     (4099, 64, "mixed"), (2049, 33, "mixed")])
def test_reduce_rows(hip_lib, N, W, mix):
    """Rows through union maps of mtgs_dp_union: every geo row equals the dense entries bit for bit (words 11..13 = C0 * sum v_rgb
    against the float32 reference, word 14 zero, word 15 and geo_ids the index, row_of -1 or the row); coefficient rows equal the
    dense v_coeffs rows of the same mask bit for bit; a capacity of count - 1 drops the last row, row_of still names it, nothing is
    written past the cap; coef_stride > 3 K leaves the canary in the gaps."""
    sc = scene(N, W, mix)
    D = Dev(sc)
    K, degree = 16, 3
    allm = (1 << W) - 1
    masks = [allm, allm, 1, 1 << (W - 1), allm & 0x5555555555555555, 0]
    U = union_of(D, masks)
    U.check()
    geo14 = R.reduce_geometry_f32(sc["senders"], N)
    for sub in range(1, len(masks)):
        mask = masks[sub]
        dense = host(run_reduce(D, K, degree, "slices", mask=mask), N, 1, K)
        check_dense("mtgs_dp_reduce_slices", dense, sc, K, degree, mask=mask)
        dense_c = dense["vc"][:N, 0].view(np.float32)
        for cut, pad in ((0, 0), (1, 5)):
            gcap, ccap = max(U.counts[0] - cut, 0), max(U.counts[sub] - cut, 0)
            cs = 3 * K + pad
            b = row_buffers(N, gcap, ccap, cs)
            run_rows(D, U, K, degree, mask, sub, b, geo_cap=gcap, coef_cap=ccap, coef_stride=cs)
            h = {k: u32(v) for k, v in b.items()}
            gr, gro, gid, cr, cro = R.row_outputs(geo14, dense_c, U.words[0], U.words[sub], N, gcap, ccap)
            got = h["geo_rows"].reshape(-1, 16)
            assert np.array_equal(got[:gr.shape[0]], fb(gr)) and is_can(got[gr.shape[0]:]), (sub, cut)
            assert np.array_equal(h["geo_row_of"][:N].view(np.int32), gro) and is_can(h["geo_row_of"][N:])
            assert np.array_equal(h["geo_ids"][:gid.size].view(np.int32), gid) and is_can(h["geo_ids"][gid.size:])
            assert cut == 0 or U.counts[0] == 0 or int(gro.max()) == gcap      # (the dropped row is still named)
            got = h["coef_rows"].reshape(-1, cs)
            assert np.array_equal(got[:cr.shape[0], :3 * K], fb(cr)) and is_can(got[:cr.shape[0], 3 * K:]) and is_can(got[cr.shape[0]:])
            assert np.array_equal(h["coef_row_of"][:N].view(np.int32), cro) and is_can(h["coef_row_of"][N:])
            if cut == 0:                                 # (and against float64, as the dense entries they equal)
                want, S = R.reduce_colour_f64(sc["senders"], sc["means"], sc["cams"], K, degree, mask)
                ids = np.flatnonzero(cro >= 0)
                note_ratio("mtgs_dp_reduce_rows", got[:ids.size, :3 * K].view(np.float32).reshape(-1, K, 3), want[ids], S[ids], W)
    # either half alone
    b = row_buffers(N, U.counts[0], U.counts[2], 3 * K)
    run_rows(D, U, K, degree, masks[2], 2, b, coef=False, geo_cap=U.counts[0])
    h = {k: u32(v) for k, v in b.items()}
    assert is_can(h["coef_rows"]) and is_can(h["coef_row_of"]) and not is_can(h["geo_row_of"][:N])
    b = row_buffers(N, U.counts[0], U.counts[2], 3 * K)
    run_rows(D, U, K, degree, masks[2], 2, b, geo=False, coef_cap=U.counts[2], coef_stride=3 * K)
    h = {k: u32(v) for k, v in b.items()}
    assert is_can(h["geo_rows"]) and is_can(h["geo_row_of"]) and is_can(h["geo_ids"]) and not is_can(h["coef_row_of"][:N])


@pytest.mark.parametrize("n_groups", [1, 3, 8])
@pytest.mark.parametrize("N,W,mix", [(65, 3, "mixed"), (4099, 8, "random"), (2049, 64, "mixed")])
def test_reduce_rows_groups(hip_lib, N, W, mix, n_groups):
    """Every colour group of a step in one launch: bit-identical to one mtgs_dp_reduce_rows call per group (overlapping masks, a
    group with an empty mask), with and without the geometry rows (geo_rows NULL)."""
    from mtgs_amd import _abi
    sc = scene(N, W, mix)
    D = Dev(sc)
    K, degree = 16, 3
    allm = (1 << W) - 1
    gm = [allm & 0x5555555555555555, 0, allm & 0x3333333333333333, 1, 1 << (W - 1), allm, allm & ~1, allm & 0x0F0F0F0F0F0F0F0F][:n_groups]
    U = union_of(D, [allm] + gm)
    cs = 3 * K + 2
    for with_geo in (True, False):
        single = [row_buffers(N, U.counts[0], U.counts[1 + j], cs) for j in range(n_groups)]
        for j in range(n_groups):
            run_rows(D, U, K, degree, gm[j], 1 + j, single[j], geo=with_geo and j == 0, geo_cap=U.counts[0], coef_cap=U.counts[1 + j],
                     coef_stride=cs)
        grouped = [row_buffers(N, U.counts[0], U.counts[1 + j], cs) for j in range(n_groups)]
        tab = np.zeros(n_groups, dtype=_abi.struct_dtype("mtgs_dp_group"))
        for j in range(n_groups):
            tab[j] = (gm[j], grouped[j]["coef_rows"].data_ptr(), U.words_ptr(1 + j), U.prefix_ptr(1 + j), grouped[j]["coef_row_of"].data_ptr(),
                      U.counts[1 + j])
        tab_dev = up(tab.view(np.uint8))
        g0 = grouped[0]
        z = lambda name: g0[name].data_ptr() if with_geo else None
        _call("mtgs_dp_reduce_rows_groups", W, N, K, degree, D.means.data_ptr(), D.words_ptr(0), D.prefix_ptr(0), D.stride_b,
              D.rows.data_ptr(), D.row_stride, D.cams.data_ptr(), 0, -1, n_groups, tab_dev.data_ptr(), z("geo_rows"), U.words_ptr(0),
              U.prefix_ptr(0), z("geo_row_of"), z("geo_ids"), U.counts[0], cs, _st(D.rows))
        torch.cuda.synchronize()
        for j in range(n_groups):
            for name in single[j]:
                assert np.array_equal(u32(grouped[j][name]), u32(single[j][name])), (with_geo, j, name)
        assert is_can(u32(g0["geo_rows"])) != with_geo or U.counts[0] == 0
        # the colour rows against float64 as well (the rows are the dense entries)
        for j in range(n_groups):
            want, S = R.reduce_colour_f64(sc["senders"], sc["means"], sc["cams"], K, degree, gm[j])
            ids = np.flatnonzero(R.flags_of(U.words[1 + j], N))
            got = u32(grouped[j]["coef_rows"]).reshape(-1, cs)[:ids.size, :3 * K].view(np.float32).reshape(-1, K, 3)
            note_ratio("mtgs_dp_reduce_rows_groups", got, want[ids], S[ids], W)


# ---- mtgs_dp_accumulate -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,degree", [(16, 3), (25, 4)])
@pytest.mark.parametrize("n_rows", [0, 1, 15, 16, 17])
def test_accumulate(hip_lib, K, degree, n_rows):
    """One sender's rows added into non-zero tensors (degree 4 takes the 32-threads-per-row form), with and without v_coeffs:
    geometry = ONE float32 addition per entry, exact; colour against float64 within the one-sender bar plus the rounding of the
    addition into the existing value, 2^-24 (|base| + S); the entries of the other Gaussians and the slack keep their bits."""
    N = 1025
    sc = scene(N, 8, "random")
    rows = sc["senders"][3][1][:n_rows]
    rng = np.random.default_rng(n_rows + K)
    shapes = ((N + SL, 3), (N + SL, 4), (N + SL, 3), (N + SL,), (N + SL, K, 3))
    base = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    src = up(rows) if n_rows else can(16)
    means, cam = up(sc["means"]), up(sc["cams"][3])
    for with_coeffs in (True, False):
        dev = [up(b) for b in base]
        _call("mtgs_dp_accumulate", n_rows, src.data_ptr(), N, K, degree, means.data_ptr(), cam.data_ptr(), *(d.data_ptr() for d in dev[:4]),
              dev[4].data_ptr() if with_coeffs else None, _st(means))
        got = [d.cpu().numpy() for d in dev]
        idx = R.row_index(rows)
        for i, (a, b) in enumerate(((0, 3), (3, 7), (7, 10), (10, 11))):
            want = base[i].copy().reshape(N + SL, -1)
            want[idx] = want[idx] + rows[:, a:b]
            assert np.array_equal(fb(got[i]).reshape(N + SL, -1), fb(want)), i
        ref, S = R.accumulate_f64(rows, sc["means"], sc["cams"][3], K, degree, [b[:N] for b in base])
        other = np.ones(N + SL, dtype=bool)
        other[idx] = False
        assert np.array_equal(fb(got[4])[other], fb(base[4])[other])
        if with_coeffs:
            err = np.abs(got[4][:N].astype(np.float64) - ref[4])
            bar = R.colour_bar(1, S)[:, None, :] + 2.0 ** -24 * (np.abs(base[4][:N].astype(np.float64)) + S[:, None, :])
            assert (err <= bar).all(), float((err - bar).max())
            if (bar > 0).any():
                name = "mtgs_dp_accumulate (share of its own bar)"
                RATIOS[name] = max(RATIOS.get(name, 0.0), float((err[bar > 0] / bar[bar > 0]).max()))
            nb = (degree + 1) ** 2
            assert np.array_equal(fb(got[4][:, nb:]), fb(base[4][:, nb:]))
        else:
            assert np.array_equal(fb(got[4]), fb(base[4]))
