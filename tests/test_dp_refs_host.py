"""tests/dp_refs.py without a GPU: (1) maps, rows and row numbers against brute-force Python loops on every visibility pattern
of tests/test_gpu_dp_edges.py; (2) the colour reference against float64 autograd of oracle/torch_ref.spherical_harmonics -- an
independent statement of the basis and of the normalisation; (3) the input sets of the GPU file are conditioned as its bar
assumes: every |mean - cam| >= 0.5, every |basis| < 1, and the float32 restatement of the colour sum stays within a QUARTER of the
bar (16 + W) * 2^-23 * S the device has to meet."""
import numpy as np
import pytest
import torch

from tests import dp_refs as R
from tests import test_gpu_dp_edges as E


def _popcount(x):
    return bin(int(x)).count("1")


# ---- (1) maps and rows against loops ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", E.N_LIST)
def test_vis_map_and_rows_against_loops(N):
    sc = E.scene(N, 33, "mixed")                         # the eleven patterns, three times
    for r in range(11):
        flags, rows = sc["senders"][r]
        words, prefix, count = R.vis_map(flags)
        nw = (N + 63) // 64
        want_w, want_p, run = [0] * nw, [0] * nw, 0
        for w in range(nw):
            want_p[w] = run
            for b in range(64):
                n = 64 * w + b
                if n < N and sc["radii"][r, n] > 0:
                    want_w[w] |= 1 << b
                    run += 1
        assert words.dtype == np.uint64 and prefix.dtype == np.uint32 and words.shape == prefix.shape == (nw,)
        assert [int(w) for w in words] == want_w and [int(p) for p in prefix] == want_p and count == run
        assert np.array_equal(R.flags_of(words, N), flags) and np.array_equal(R.popcount64(words), [_popcount(w) for w in want_w])
        g = sc["grads"]
        j = 0
        for n in range(N):
            if not flags[n]:
                continue
            assert j == want_p[n // 64] + _popcount(want_w[n // 64] & ((1 << (n % 64)) - 1))       # the row of Gaussian n
            want = list(g["v_means"][r, n]) + list(g["v_quats"][r, n]) + list(g["v_scales"][r, n]) + [g["v_opacities"][r, n]] \
                + list(g["v_rgb"][r, n]) + [np.float32(0.0)]
            assert np.array_equal(E.fb(rows[j, :15]), E.fb(np.array(want, dtype=np.float32))) and rows[j, 15:].view(np.int32)[0] == n
            j += 1
        assert j == rows.shape[0] == count
    none = R.pack_rows(sc["senders"][0][0], *(sc["grads"][k][0] for k in ("v_means", "v_quats", "v_scales", "v_opacities")), None)
    assert not none[:, 11:15].any() and np.array_equal(none[:, :11], sc["senders"][0][1][:, :11])


def test_full_word_edges():
    """Bit 63, popcount 64 and the mask below lane 63 in the reference itself."""
    words, prefix, count = R.vis_map(np.ones(130, dtype=bool))
    assert [int(w) for w in words] == [2 ** 64 - 1, 2 ** 64 - 1, 3] and list(prefix) == [0, 64, 128] and count == 130
    words, prefix, count = R.vis_map(np.arange(128) == 63)
    assert [int(w) for w in words] == [1 << 63, 0] and list(prefix) == [0, 1] and count == 1


@pytest.mark.parametrize("r", [0, 2])
@pytest.mark.parametrize("N", E.N_LIST)
def test_touched_and_chunks_against_loops(N, r):
    rows, special = E.touched_input(N, r)
    kept, flags = R.touched(rows, N)
    want, gaussians = [], []
    for j in range(rows.shape[0]):
        # != 0 per word: -0.0 is zero, NaN is not
        if any(not (float(v) == 0.0) for v in rows[j, :14]):
            want.append(j)
            gaussians.append(int(rows[j, 15:].view(np.int32)[0]))
    assert np.array_equal(E.fb(kept), E.fb(rows[want])) and np.array_equal(np.flatnonzero(flags), gaussians)
    assert 0 not in want and all((j in want) == (kind == "nan") for j, kind in special.items())
    assert r == 0 or N <= 128 or gaussians[-1] != want[-1]      # (r = 2: a row's position is not its Gaussian)
    if N >= 65:
        begin = E._bounds(N, 4)
        caps = [2, N, 0, N]
        chunks, overflow = R.chunk_split(kept, begin, caps)
        idx = R.row_index(kept)
        over = 0
        for c in range(4):
            mine = [j for j in range(kept.shape[0]) if begin[c] <= idx[j] < begin[c + 1]]
            over |= len(mine) > caps[c]
            assert np.array_equal(E.fb(chunks[c]), E.fb(kept[mine[:caps[c]]]))
        assert overflow == over


@pytest.mark.parametrize("N,W,mix", [(1, 1, "mixed"), (65, 64, "mixed"), (1025, 8, "random"), (4099, 8, "disjoint"), (33, 3, "full")])
def test_union_geometry_and_row_outputs_against_loops(N, W, mix):
    sc = E.scene(N, W, mix)
    words = np.stack([R.words_of(f) for f, _ in sc["senders"]])
    masks = [0, 1, (1 << W) - 1, 1 << (W - 1), ((1 << W) - 1) & 0x5555555555555555]
    uw, upf, tot = R.union(words, masks)
    for p, m in enumerate(masks):
        flags = np.zeros(N, dtype=bool)
        for r in range(W):
            if (m >> r) & 1:
                flags |= sc["flags"][r]
        w2, p2, c2 = R.vis_map(flags)
        assert np.array_equal(uw[p], w2) and np.array_equal(upf[p], p2) and int(tot[p]) == c2 << 32
    # geometry: one float32 addition per sender that has a row, in rank order, from +0.0
    for cap in (None, 1, 40):
        geo = R.reduce_geometry_f32(sc["senders"], N, cap)
        want = np.zeros((N, 14), dtype=np.float32)
        for flags, rows in sc["senders"]:
            for j in range(rows.shape[0] if cap is None else min(cap, rows.shape[0])):
                n = int(rows[j, 15:].view(np.int32)[0])
                for k in range(14):
                    want[n, k] = np.float32(want[n, k] + rows[j, k])
        assert np.array_equal(E.fb(geo), E.fb(want))
    geo = R.reduce_geometry_f32(sc["senders"], N)
    coeffs = np.arange(N * 12, dtype=np.float32).reshape(N, 4, 3)
    for cap in (None, max(int(tot[2] >> 32) - 1, 0)):
        gr, gro, gid, cr, cro = R.row_outputs(geo, coeffs, uw[2], uw[4], N, cap, cap)
        u = 0
        for n in range(N):
            if not R.flags_of(uw[2], N)[n]:
                assert gro[n] == -1
                continue
            assert gro[n] == u
            if cap is None or u < cap:
                assert gid[u] == n and np.array_equal(E.fb(gr[u, :11]), E.fb(geo[n, :11])) and gr[u, 14] == 0
                assert np.array_equal(E.fb(gr[u, 11:14]), E.fb(np.float32(0.2820947917738781) * geo[n, 11:14]))
                assert gr[u, 15:].view(np.int32)[0] == n
            u += 1
        assert gr.shape[0] == gid.size == (u if cap is None else min(u, cap))
        ids = np.flatnonzero(cro >= 0)
        assert np.array_equal(cro[ids], np.arange(ids.size)) and np.array_equal(ids, np.flatnonzero(R.flags_of(uw[4], N)))
        assert np.array_equal(cr, coeffs[ids[:cr.shape[0]]].reshape(-1, 12)) and cr.shape[0] == (ids.size if cap is None else min(ids.size, cap))


# ---- (2) the colour reference against autograd of the independent restatement ---------------------------------------------------------
@pytest.mark.parametrize("K,degree", E.KDEG + ((25, 4),))
def test_colour_reference_against_autograd(K, degree):
    from oracle import torch_ref
    sc = E.scene(1025, 8, "random")
    N, W = sc["N"], sc["W"]
    mask = 0b10110101
    got, S = R.reduce_colour_f64(sc["senders"], sc["means"], sc["cams"], K, degree, mask)
    want = torch.zeros(N, K, 3, dtype=torch.float64)
    S_want = np.zeros((N, 3))
    means = torch.from_numpy(sc["means"]).double()
    for r in range(W):
        if not (mask >> r) & 1:
            continue
        v_rgb = torch.from_numpy(np.where(sc["flags"][r][:, None], sc["grads"]["v_rgb"][r], 0.0)).double()
        coeffs = torch.zeros(N, K, 3, dtype=torch.float64, requires_grad=True)
        dirs = means - torch.from_numpy(sc["cams"][r]).double()          # (not normalised: the restatement does that itself)
        (torch_ref.spherical_harmonics(degree, dirs, coeffs) * v_rgb).sum().backward()
        want += coeffs.grad
        S_want += np.abs(v_rgb.numpy())
    assert np.abs(got - want.numpy()).max() <= 1e-14 and np.array_equal(S, S_want)
    assert not got[:, (degree + 1) ** 2:].any() and float(np.abs(got).max()) > 0.1
    # one sender's rows into existing values: the same expression
    base = [np.ones((N, 3), np.float32), np.ones((N, 4), np.float32), np.ones((N, 3), np.float32), np.ones(N, np.float32),
            np.ones((N, K, 3), np.float32)]
    rows = sc["senders"][0][1]
    out, S1 = R.accumulate_f64(rows, sc["means"], sc["cams"][0], K, degree, base)
    one, S0 = R.reduce_colour_f64(sc["senders"], sc["means"], sc["cams"], K, degree, 1)
    assert np.array_equal(out[4], 1.0 + one) and np.array_equal(S1, S0)
    geo = R.reduce_geometry_f32(sc["senders"][:1], N).astype(np.float64)
    assert np.array_equal(out[0], 1.0 + geo[:, 0:3]) and np.array_equal(out[3], 1.0 + geo[:, 10])


# ---- (3) conditioning of every input set of the GPU file ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,W,mix", E.SCENES)
def test_gpu_inputs_are_conditioned(N, W, mix):
    sc = E.scene(N, W, mix)
    d = sc["means"][None].astype(np.float64) - sc["cams"][:, None].astype(np.float64)
    dist = np.sqrt((d * d).sum(-1))
    assert dist.min() >= 0.5
    basis = R.sh_basis(4, (d / dist[..., None]).reshape(-1, 3))
    assert float(np.abs(basis).max()) < 1.0
    full = (1 << W) - 1
    worst = 0.0
    for (K, degree), mask in zip(((16, 3), (4, 1), (9, 2)), (full, full, full & 0x5555555555555555)):
        f64, S = R.reduce_colour_f64(sc["senders"], sc["means"], sc["cams"], K, degree, mask)
        f32, S32 = R.reduce_colour_f32(sc["senders"], sc["means"], sc["cams"], K, degree, mask)
        assert f32.dtype == np.float32 and np.array_equal(S, S32)
        err = np.abs(f32.astype(np.float64) - f64)
        bar = R.colour_bar(W, S)[:, None, :]
        assert (err <= 0.25 * bar).all(), float((err / np.maximum(bar, 1e-300)).max())
        if (S > 0).any():
            worst = max(worst, float((err / np.maximum(R.EPS * S[:, None, :], 1e-300))[np.broadcast_to(S[:, None, :] > 0, err.shape)].max()))
    assert worst <= 0.25 * (16 + W)


def test_accumulate_inputs_are_conditioned():
    """mtgs_dp_accumulate also runs degree 4 (one sender; its bar is the W = 1 bar plus the rounding of the addition into the
    existing value): a quartic carries one more factor than the cubic the bar was reasoned for, so the float32 restatement is
    held to HALF of the W = 1 bar there (measured: 4.4 of 17), and to a quarter at degree 3 as everywhere."""
    sc = E.scene(1025, 8, "random")
    for (K, degree), share in (((16, 3), 0.25), ((25, 4), 0.5)):
        one = [(None, sc["senders"][3][1])]
        f64, S = R.reduce_colour_f64(one, sc["means"], sc["cams"][3:4], K, degree, 1)
        f32, _ = R.reduce_colour_f32(one, sc["means"], sc["cams"][3:4], K, degree, 1)
        assert (np.abs(f32.astype(np.float64) - f64) <= share * R.colour_bar(1, S)[:, None, :]).all()
