"""Host references of the sparse, factored gradient exchange (csrc/dp.hip), written from the contract in include/mtgs_rast.h
("view-parallel data parallelism"): numpy only, no device, no library.

A SENDER is the pair (flags[N] bool, rows[count, 16] float32): which Gaussians it has a row for and the rows in index order.
Wire row: v_mean 3 | v_quat 4 | v_scale 3 | v_opacity 1 | v_rgb 3 | 0 | Gaussian index (int bits).
Map of a sender (and of a union of senders): words[ceil(N/64)] u64, bit n % 64 of word n // 64; prefix[ceil(N/64)] u32 = set
bits in the words before; row(n) = prefix[n // 64] + popcount(words[n // 64] below bit n % 64).

Geometry sums are EXACT expectations: the receiver adds one float32 value per sender, in rank order, into an accumulator that
starts at +0.0 (reduce_geometry_f32).  Colour sums are float64 (reduce_colour_f64) beside S = sum |v_rgb|, the scale of the bar
(16 + W) * 2^-23 * S the device has to meet; reduce_colour_f32 is the same expression in float32 and only shows that the inputs
are well conditioned (tests/test_dp_refs_host.py)."""
import numpy as np

C0 = np.float32(0.2820947917738781)
EPS = 2.0 ** -23


def colour_bar(W, S):
    """|device - float64| allowed per element: restatement 2.3 + rsq / cubic 3 + sequential sum (W - 1) / 2, in ulp of S, rounded up."""
    return (16 + W) * EPS * S


def n_words(N):
    return (int(N) + 63) // 64


def popcount64(w):
    w = np.ascontiguousarray(w, dtype=np.uint64)
    return np.unpackbits(w.view(np.uint8).reshape(-1, 8), axis=1).sum(1).astype(np.int64).reshape(w.shape)


def words_of(flags):
    flags = np.asarray(flags, dtype=bool)
    nw = n_words(flags.size)
    padded = np.zeros(nw * 64, dtype=np.uint8)
    padded[:flags.size] = flags
    return np.packbits(padded, bitorder="little").view("<u8").astype(np.uint64)


def flags_of(words, N):
    words = np.ascontiguousarray(words, dtype="<u8")
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:N].astype(bool)


def prefix_of(words):
    c = popcount64(words)
    return (np.cumsum(c) - c).astype(np.uint32), int(c.sum())


def vis_map(flags):
    """flags[N] -> (words u64, prefix u32, count); bits at positions >= N are zero."""
    words = words_of(flags)
    prefix, count = prefix_of(words)
    return words, prefix, count


def pack_rows(flags, v_means, v_quats, v_scales, v_opacities, v_rgb):
    """The wire rows [count, 16] of the flagged Gaussians in index order (v_rgb None: zeros)."""
    idx = np.flatnonzero(np.asarray(flags, dtype=bool))
    rows = np.zeros((idx.size, 16), dtype=np.float32)
    rows[:, 0:3] = np.asarray(v_means, np.float32).reshape(-1, 3)[idx]
    rows[:, 3:7] = np.asarray(v_quats, np.float32).reshape(-1, 4)[idx]
    rows[:, 7:10] = np.asarray(v_scales, np.float32).reshape(-1, 3)[idx]
    rows[:, 10] = np.asarray(v_opacities, np.float32).reshape(-1)[idx]
    if v_rgb is not None:
        rows[:, 11:14] = np.asarray(v_rgb, np.float32).reshape(-1, 3)[idx]
    rows[:, 15] = idx.astype(np.int32).view(np.float32)
    return rows


def row_index(rows):
    return np.ascontiguousarray(rows[:, 15]).view(np.int32).astype(np.int64)


def touched(rows, N):
    """(kept rows in the same order, flags[N] of their Gaussians): a row is kept when any of words 0..13 is != 0 -- a row of
    only -0.0 is not, a NaN row is; the pad (14) and the index (15) do not count."""
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, 16)
    keep = (rows[:, :14] != 0).any(1)
    flags = np.zeros(N, dtype=bool)
    flags[row_index(rows[keep])] = True
    return rows[keep], flags


def chunk_split(rows, begin, cap):
    """Index-ordered rows -> ([rows of the Gaussians in [begin[c], begin[c + 1]), at most cap[c] of them], overflow)."""
    idx = row_index(rows)
    out, overflow = [], 0
    for c in range(len(begin) - 1):
        mine = rows[(idx >= begin[c]) & (idx < begin[c + 1])]
        overflow |= int(mine.shape[0] > cap[c])
        out.append(mine[:cap[c]])
    return out, overflow


def union(words_per_sender, masks):
    """words[W, nw], masks[P] (bit r = sender r) -> (words[P, nw], prefix[P, nw], totals[P] = count << 32)."""
    wps = np.asarray(words_per_sender, dtype=np.uint64)
    W, nw = wps.shape
    uw = np.zeros((len(masks), nw), dtype=np.uint64)
    up = np.zeros((len(masks), nw), dtype=np.uint32)
    totals = np.zeros(len(masks), dtype=np.int64)
    for p, m in enumerate(masks):
        for r in range(W):
            if (int(m) >> r) & 1:
                uw[p] |= wps[r]
        up[p], cnt = prefix_of(uw[p])
        totals[p] = cnt << 32
    return uw, up, totals


def _cut(rows, row_cap):
    return rows if row_cap is None else rows[:max(int(row_cap), 0)]


def reduce_geometry_f32(senders, N, row_cap=None):
    """[N, 14] float32: words 0..10 the geometry sums, 11..13 sum v_rgb -- one float32 addition per sender that has a row, in
    rank order, from +0.0.  row_cap: only a sender's rows at positions < row_cap exist."""
    acc = np.zeros((N, 14), dtype=np.float32)
    for _, rows in senders:
        rows = _cut(rows, row_cap)
        idx = row_index(rows)
        acc[idx] = acc[idx] + rows[:, :14]          # (indices are unique within a sender)
    return acc


def sh_basis(degree, d, dtype=np.float64):
    """Real SH basis [n, (degree + 1)^2] of unit vectors d[n, 3] (the polynomial form of gsplat's _eval_sh_bases_fast), every
    operation in `dtype`."""
    f = dtype
    x, y, z = (d[:, i].astype(f) for i in range(3))
    b = [np.full_like(x, f(0.2820947917738781))]
    if degree >= 1:
        b += [f(-0.48860251190292) * y, f(0.48860251190292) * z, f(-0.48860251190292) * x]
    if degree >= 2:
        z2 = z * z
        t0b = f(-1.092548430592079) * z
        c1, s1 = x * x - y * y, f(2) * x * y
        p6 = f(0.9461746957575601) * z2 - f(0.3153915652525201)
        b += [f(0.5462742152960395) * s1, t0b * y, p6, t0b * x, f(0.5462742152960395) * c1]
    if degree >= 3:
        t0c = f(-2.285228997322329) * z2 + f(0.4570457994644658)
        t1b = f(1.445305721320277) * z
        c2, s2 = x * c1 - y * s1, x * s1 + y * c1
        p12 = z * (f(1.865881662950577) * z2 - f(1.119528997770346))
        b += [f(-0.5900435899266435) * s2, t1b * s1, t0c * y, p12, t0c * x, t1b * c1, f(-0.5900435899266435) * c2]
    if degree >= 4:
        t0d = z * (f(-4.683325804901025) * z2 + f(2.007139630671868))
        t1c = f(3.31161143515146) * z2 - f(0.47308734787878)
        t2b = f(-1.770130769779931) * z
        c3, s3 = x * c2 - y * s2, x * s2 + y * c2
        p20 = f(1.984313483298443) * z * p12 - f(1.006230589874905) * p6
        b += [f(0.6258357354491763) * s3, t2b * s2, t1c * s1, t0d * y, p20, t0d * x, t1c * c1, t2b * c2, f(0.6258357354491763) * c3]
    return np.stack(b, axis=1)


def _reduce_colour(senders, means, cams, K, degree, mask, row_cap, dtype):
    N = means.shape[0]
    nb = (degree + 1) ** 2
    assert nb <= K
    out = np.zeros((N, K, 3), dtype=dtype)
    S = np.zeros((N, 3), dtype=np.float64)
    means, cams = np.asarray(means, np.float32).astype(dtype), np.asarray(cams, np.float32).astype(dtype)
    for r, (_, rows) in enumerate(senders):
        if not (int(mask) >> r) & 1:
            continue
        rows = _cut(rows, row_cap)
        idx = row_index(rows)
        d = means[idx] - cams[r]
        d = d / np.sqrt((d * d).sum(1, dtype=dtype), dtype=dtype)[:, None]
        rgb = rows[:, 11:14].astype(dtype)
        out[idx, :nb] = out[idx, :nb] + sh_basis(degree, d, dtype)[:, :, None] * rgb[:, None, :]
        S[idx] += np.abs(rows[:, 11:14].astype(np.float64))
    return out, S


def reduce_colour_f64(senders, means, cams, K, degree, mask, row_cap=None):
    """(v_coeffs[N, K, 3] float64 = sum over the senders r of `mask` of basis_k(normalize(mean - cam_r)) * v_rgb_r, zero for
    k >= (degree + 1)^2; S[N, 3] = sum |v_rgb_r| over the same senders)."""
    return _reduce_colour(senders, means, cams, K, degree, mask, row_cap, np.float64)


def reduce_colour_f32(senders, means, cams, K, degree, mask, row_cap=None):
    return _reduce_colour(senders, means, cams, K, degree, mask, row_cap, np.float32)


def accumulate_f64(rows, means, cam, K, degree, base):
    """mtgs_dp_accumulate: ONE sender's rows added into base = (v_means, v_quats, v_scales, v_opacities, v_coeffs | None);
    returns the five float64 results and S[N, 3] = |v_rgb| of the rows."""
    N = means.shape[0]
    out = [None if b is None else np.asarray(b, np.float32).astype(np.float64).copy() for b in base]
    idx = row_index(rows)
    r64 = rows.astype(np.float64)
    out[0][idx] += r64[:, 0:3]
    out[1][idx] += r64[:, 3:7]
    out[2][idx] += r64[:, 7:10]
    out[3][idx] += r64[:, 10]
    S = np.zeros((N, 3))
    S[idx] = np.abs(r64[:, 11:14])
    if out[4] is not None:
        add, _ = reduce_colour_f64([(None, rows)], means, np.asarray(cam, np.float32).reshape(1, 3), K, degree, 1)
        out[4] += add
    return out, S


def row_outputs(geo14, coeffs, geo_words, coef_words, N, geo_cap=None, coef_cap=None):
    """The row form of the dense results through union maps: geo_rows[min(count, cap), 16] = {11 geometry sums, C0 * sum v_rgb 3
    (one float32 multiply), 0, index}, geo_row_of[N] (-1 or the row, also of a row beyond the capacity), geo_ids[rows written];
    coef_rows[min(count, cap), K * 3] = the dense coefficient entries, coef_row_of[N].  Either half may be None."""
    def numbering(words):
        flags = flags_of(words, N)
        ids = np.flatnonzero(flags)
        row_of = np.full(N, -1, dtype=np.int32)
        row_of[ids] = np.arange(ids.size, dtype=np.int32)
        return ids, row_of
    geo_rows = geo_row_of = geo_ids = coef_rows = coef_row_of = None
    if geo14 is not None:
        ids, geo_row_of = numbering(geo_words)
        ids = ids[:ids.size if geo_cap is None else geo_cap]
        geo_rows = np.zeros((ids.size, 16), dtype=np.float32)
        geo_rows[:, :11] = geo14[ids, :11]
        geo_rows[:, 11:14] = C0 * geo14[ids, 11:14].astype(np.float32)
        geo_rows[:, 15] = ids.astype(np.int32).view(np.float32)
        geo_ids = ids.astype(np.int32)
    if coeffs is not None:
        ids, coef_row_of = numbering(coef_words)
        ids = ids[:ids.size if coef_cap is None else coef_cap]
        coef_rows = coeffs[ids].reshape(ids.size, int(np.prod(coeffs.shape[1:])))
    return geo_rows, geo_row_of, geo_ids, coef_rows, coef_row_of
