"""The per-Gaussian operators around the scene graph at block, node and option edges: Fourier colour (csrc/fourier.hip),
deformation embedding (deform.hip), densification statistics (stats.hip), refinement (refine.hip) and the out-of-box loss
(oob.hip), each against the plain references of tests/node_refs.py (refinement: oracle/refine_oracle.py with the same Philox
samples).

All cases are tiny: the sizes are chosen for launch geometry (0, 1, one wave +- 1, one block +- 1, two blocks + 1), not for
workload.  The input builders and their conditioning checks are shared with tests/test_node_refs_host.py, which runs the
conditioning check of every refinement and out-of-box case without a GPU: no statistic lies within 1e-4 relative of the
threshold it is compared with, so the float32 device and the float64 oracle must take the SAME decision for every row and
masks, counts and order are compared for identity.

Tolerances are either those of the existing test of the same operator (test_gpu_densify.py, test_gpu_loss.py) or a bound on
the rounding of the float32 arithmetic the kernel's header comment describes, computed per element from the float64 reference;
the constant of each such bound was measured on the CPU (float32 NumPy against float64) and carries its measurement."""
import numpy as np
import pytest
import torch

from tests import node_refs as R

pytestmark = pytest.mark.gpu

BLOCK_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 513]
U32 = R.U32

# A float32 sum of n terms against the float64 sum: |err| <= C_SUM * 2^-24 * sum |term|.  Measured on the CPU for the largest
# Fourier size (N = 1366, 4098 products per weight, formed and added in float32 one after the other in element order) over the
# four series lengths: worst |err| / (2^-24 * abs_terms_w[f]) = 4.24 (at F = 1; 0.52, 1.69, 1.57 at F = 2, 31, 32).  Times 4,
# because the device adds in another order (a wave tree, four waves, per-block partials, then the library's sum over the
# blocks).  abs_terms_w adds |<features_dc[n,f,:], v_dc[n,:]>| per Gaussian, so a small case whose three products cancel is
# ill-conditioned against it; tests/test_node_refs_host.py requires of every case that the plain float32 sum stays within
# C_SUM / 4, and FOURIER_SEEDS replaces the seeds that do not.
C_SUM = 17.0
# sin / cos of the embedding: np.sin / np.cos in float32 at the float32 arguments of every case below (up to 2^15 |x|,
# |x| <= 3) against float64 at the same arguments: worst error 6.72e-8.  Times 4 for another libm: 2.7e-7, below the cap of 1e-5.
SINCOS_TOL = 2.7e-7


def bits(t):
    """The bit patterns of a float32 tensor (bit-for-bit comparisons that also hold for NaN and -0.0)."""
    return t.detach().contiguous().cpu().view(torch.int32)


# ---- Fourier colour -------------------------------------------------------------------------------------------------------------
# fourier.hip: one thread per (Gaussian, channel), 256 per block, FOURIER_MAX_DIM = 32.  3 N = 0, 3, 63, 66, 255, 258, 513, 771,
# 4098: below, at and above a wave and a block, with dead lanes in the last wave of the weight-gradient tree.
FOURIER_NS = [0, 1, 21, 22, 85, 86, 171, 257, 1366]
FOURIER_FS = [1, 2, 31, 32]


FOURIER_SEEDS = {(1, 31): 3, (1, 32): 2, (21, 32): 1}


def fourier_inputs(N, F):
    g = torch.Generator().manual_seed(FOURIER_SEEDS.get((N, F), 0) * 1000003 + N * 100 + F)
    return torch.randn(N, F, 3, generator=g), torch.rand(F, generator=g) * 2 - 1, torch.randn(N, 3, generator=g)


def seq_sum_f32(terms):
    """The float32 sum of a float32 vector, one add after the other."""
    acc = np.float32(0)
    for x in terms:
        acc = np.float32(acc + x)
    return acc


def fourier_seq_f32_ratio(N, F):
    """worst |v_w(float32, sequential) - v_w(float64)| / (2^-24 abs_terms_w) over f: the measurement behind C_SUM."""
    fdc, w, G = (t.numpy() for t in fourier_inputs(N, F))
    _, _, v_w, abs_w = R.fourier_ref(fdc, w, G)
    worst = 0.0
    for f in range(F):
        got = seq_sum_f32((fdc[:, f, :] * G).reshape(-1))
        worst = max(worst, abs(float(got) - v_w[f]) / (U32 * abs_w[f]))
    return worst


@pytest.mark.parametrize("F", FOURIER_FS)
@pytest.mark.parametrize("N", FOURIER_NS)
def test_fourier_dc_edges(hip_lib, N, F):
    """dc and v_features_dc: |err| <= 4 F 2^-24 sum_f |term| per element (first-order rounding of an F-term float32 sum, a
    margin of 4 for FMA contraction); v_w[f]: C_SUM 2^-24 abs_terms_w[f].  Without a gradient for the weights the kernel gets
    partial_w = NULL: v_features_dc must not change by a bit."""
    from mtgs_amd.nodes import _FourierDC, fourier_features_dc, idft_weights
    fdc, w, G = fourier_inputs(N, F)
    dc_ref, vf_ref, vw_ref, abs_w = R.fourier_ref(fdc.numpy(), w.numpy(), G.numpy())
    f64 = lambda t: t.numpy().astype(np.float64)
    dc_bound = 4 * F * U32 * np.einsum("nfc,f->nc", np.abs(f64(fdc)), np.abs(f64(w)))
    vf_bound = 4 * F * U32 * np.abs(vf_ref)

    def run(w_grad):
        p = fdc.cuda().requires_grad_(True)
        wd = w.cuda().requires_grad_(w_grad)
        dc = _FourierDC.apply(p, wd)
        (dc * G.cuda()).sum().backward()
        return dc.detach(), p.grad, wd.grad
    dc, vf, vw = run(True)
    dc0, vf0, vw0 = run(False)
    assert dc.shape == (N, 3) and vf.shape == (N, F, 3) and vw.shape == (F,) and vw0 is None
    assert torch.equal(bits(dc), bits(dc0)) and torch.equal(bits(vf), bits(vf0))
    assert (np.abs(f64(dc.cpu()) - dc_ref) <= dc_bound).all(), np.abs(f64(dc.cpu()) - dc_ref).max()
    assert (np.abs(f64(vf.cpu()) - vf_ref) <= vf_bound).all(), np.abs(f64(vf.cpu()) - vf_ref).max()
    err_w = np.abs(f64(vw.cpu()) - vw_ref)
    assert (err_w <= C_SUM * U32 * abs_w).all(), (err_w / np.maximum(U32 * abs_w, 1e-300)).max()
    if N == 0:
        assert torch.equal(vw.cpu(), torch.zeros(F))
    # the public entry: the weights are the IDFT base of the frame's normalised timestamp, formed on the device
    wx = idft_weights(torch.as_tensor(0.3, device="cuda") * 1.5, F, True, device=torch.device("cuda"))
    dcx = fourier_features_dc(fdc.cuda(), 0.3, 1.5, "temporal")
    assert dcx.shape == (N, 3) and torch.equal(bits(dcx), bits(_FourierDC.apply(fdc.cuda(), wx)))
    ref_x = R.fourier_ref(fdc.numpy(), wx.cpu().numpy(), G.numpy())[0]
    bound_x = 4 * F * U32 * np.einsum("nfc,f->nc", np.abs(f64(fdc)), np.abs(f64(wx.cpu())))
    assert (np.abs(f64(dcx.cpu()) - ref_x) <= bound_x).all()


@pytest.mark.parametrize("F", [0, 33])
def test_fourier_dc_refuses_unsupported_series_lengths(hip_lib, F):
    from mtgs_amd.nodes import _FourierDC, fourier_features_dc
    fdc = torch.zeros(5, F, 3, device="cuda")
    with pytest.raises(RuntimeError, match="mtgs_fourier_dc_fwd"):
        _FourierDC.apply(fdc, torch.zeros(F, device="cuda"))
    if F > 0:
        with pytest.raises(RuntimeError, match="mtgs_fourier_dc_fwd"):
            fourier_features_dc(fdc, 0.3, 1.0, "temporal")


# ---- deformation embedding ------------------------------------------------------------------------------------------------------
# deform.hip: one thread per Gaussian, 256 per block; DEFORM_MAX_FREQS = 16, DEFORM_MAX_COND = 64 (the shared tail is full at
# (16, 16, 64)); no frequency at all; a tail of one column and of 1 + 2 + 64.
DEFORM_CFGS = [(10, 10, 16), (0, 0, 0), (16, 16, 64), (1, 0, 1), (0, 1, 64)]
DEFORM_TS = [0.0, 0.37, 1.0]
DEFORM_HEIGHT = 1.7


def deform_inputs(N, E):
    """means with |x| = |means / height * 2| spread up to about 3, an instance code in [0, 1)."""
    g = torch.Generator().manual_seed(N * 131 + E)
    means = (torch.rand(N, 3, generator=g) * 2 - 1) * (3.0 * DEFORM_HEIGHT / 2)
    return means, torch.rand(1, E, generator=g)


def sincos_f32_error():
    """worst |float32 np.sin / np.cos - float64| at the float32 arguments of every embedding case: the measurement behind
    SINCOS_TOL."""
    worst = 0.0
    for N in BLOCK_SIZES:
        for xf, tf, E in DEFORM_CFGS:
            for t in DEFORM_TS:
                _, ax, at = R.deform_embed_args(deform_inputs(N, E)[0].numpy(), DEFORM_HEIGHT, t, xf, tf)
                for a in (ax.reshape(-1), at.reshape(-1)):
                    for fn in (np.sin, np.cos):
                        if a.size:
                            worst = max(worst, float(np.abs(fn(a).astype(np.float64) - fn(a.astype(np.float64))).max()))
    return worst


def _raw_columns(xf, tf, E):
    """The columns that are copies or the same float32 expression: x, t, cond."""
    xw = 3 + 6 * xf
    return [0, 1, 2, xw] + list(range(xw + 1 + 2 * tf, xw + 1 + 2 * tf + E))


def _check_rows(got, ref, xf, tf, E):
    raw = _raw_columns(xf, tf, E)
    assert np.array_equal(got[:, raw].view(np.int32), ref[:, raw].astype(np.float32).view(np.int32)), "x / t / cond columns"
    err = np.abs(got.astype(np.float64) - ref)
    assert err.size == 0 or err.max() <= SINCOS_TOL, err.max()


@pytest.mark.parametrize("cfg", DEFORM_CFGS, ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("N", BLOCK_SIZES)
def test_deform_embed_edges(hip_lib, N, cfg):
    """The row matrix through _Embed, the gradient of the instance code, and a direct call with a row stride wider than the
    row into a buffer that holds a NaN pattern: the 5 columns behind every row and every row >= N keep the pattern."""
    from mtgs_amd._lib import call, ptr, stream_of
    from mtgs_amd.deform import _Embed
    xf, tf, E = cfg
    width = R.deform_embed_width(xf, tf, E)
    means, cond = deform_inputs(N, E)
    g = torch.Generator().manual_seed(7)
    for t in DEFORM_TS:
        ref = R.deform_embed_ref(means.numpy(), DEFORM_HEIGHT, t, cond.numpy(), xf, tf)
        assert ref.shape == (N, width)
        c = cond.cuda().requires_grad_(True)
        out = _Embed.apply(means.cuda(), DEFORM_HEIGHT, t, c, xf, tf)
        assert out.shape == (N, width)
        _check_rows(out.detach().cpu().numpy(), ref, xf, tf, E)
        V = torch.randn(N, width, generator=g)
        (out * V.cuda()).sum().backward()
        v = V[:, width - E:].numpy().astype(np.float64)
        assert c.grad.shape == cond.shape
        assert (np.abs(c.grad.cpu().numpy().astype(np.float64).reshape(-1) - v.sum(0)) <= C_SUM * U32 * np.abs(v).sum(0)).all()
        # direct call: ld = width + 5, three rows more than N
        ld = width + 5
        pattern = torch.full((N + 3, ld), 0x7FC0BEEF, dtype=torch.int32, device="cuda")
        buf = pattern.clone()
        m, cd = means.cuda(), cond.cuda()
        call("mtgs_deform_embed", N, ptr(m), DEFORM_HEIGHT, t, ptr(cd) if E else None, E, xf, tf, ptr(buf), ld, stream_of(m))
        _check_rows(buf.view(torch.float32)[:N, :width].cpu().numpy(), ref, xf, tf, E)
        assert torch.equal(buf[:N, width:], pattern[:N, width:]) and torch.equal(buf[N:], pattern[N:])


@pytest.mark.parametrize("bad", ["E65", "xf17", "tf17", "ld_short", "height0"])
def test_deform_embed_refuses_and_writes_nothing(hip_lib, bad):
    from mtgs_amd._lib import call, ptr, stream_of
    N, xf, tf, E, height = 70, 2, 2, 4, 1.7
    if bad == "E65":
        E = 65
    elif bad == "xf17":
        xf = 17
    elif bad == "tf17":
        tf = 17
    elif bad == "height0":
        height = 0.0
    width = R.deform_embed_width(xf, tf, E)
    ld = width - 1 if bad == "ld_short" else width
    means, cond = deform_inputs(N, E)
    m, cd = means.cuda(), cond.cuda()
    pattern = torch.full((N, width), 0x7FC0BEEF, dtype=torch.int32, device="cuda")
    buf = pattern.clone()
    with pytest.raises(RuntimeError, match="mtgs_deform_embed"):
        call("mtgs_deform_embed", N, ptr(m), height, 0.37, ptr(cd), E, xf, tf, ptr(buf), ld, stream_of(m))
    torch.cuda.synchronize()
    assert torch.equal(buf, pattern)


# ---- densification statistics ---------------------------------------------------------------------------------------------------
# stats.hip: 256 Gaussians per block, the batch form finds a block's node by binary search over first_block, the rows form a
# row's node by binary search over start: a node of size 0 shares both with its successor.  Zero-size first, last, two adjacent
# ones in the middle, and a table that is a single node of 0.
STATS_TABLES = [[0, 255, 256, 1], [257, 64, 0], [1, 0, 0, 256, 257], [0]]
STATS_WH = (960, 540)


def stats_inputs(sizes, seed, pad=37):
    """Statistics of every node (float32 CPU tensors) and two frames (radii [1,N] int32, absgrad [1,N,2]); the collected
    arrays are `pad` Gaussians longer than the nodes."""
    g = torch.Generator().manual_seed(seed)
    N = sum(sizes) + pad
    stats = [[torch.rand(n, generator=g), torch.ones(n) + torch.randint(0, 5, (n,), generator=g).float(),
              torch.rand(n, generator=g) * 30] for n in sizes]
    frames = [((torch.randint(0, 40, (1, N), generator=g) * (torch.rand(1, N, generator=g) < 0.4)).int(),
               torch.rand(1, N, 2, generator=g) * 1e-3) for _ in range(2)]
    return stats, frames


def _stats_reference(sizes, stats, frames):
    W, H = STATS_WH
    ref = [[t.double() for t in s] for s in stats]
    starts = np.cumsum([0] + list(sizes))[:-1]
    N = frames[0][0].shape[1]
    for radii, grad in frames:
        for s, st, n in zip(ref, starts, sizes):
            mask = torch.zeros(N, dtype=torch.bool)
            mask[st:st + n] = True
            R.stats_ref(s, radii.double(), grad.double(), mask, W, H)
    return ref


def _assert_stats(got, ref):
    for sg, sr in zip(got, ref):
        for a, b, name in zip(sg, sr, ("xys_grad_norm", "vis_counts", "max_2Dsize")):
            a = a.cpu().double()
            assert a.shape == b.shape, name
            if name == "xys_grad_norm":      # one sqrt and one add per element
                assert torch.allclose(a, b, rtol=1e-6, atol=1e-7), (name, float((a - b).abs().max()))
            else:
                assert torch.equal(a, b), name


@pytest.mark.parametrize("form", ["node", "batch"])
@pytest.mark.parametrize("sizes", STATS_TABLES, ids=lambda s: "-".join(map(str, s)))
def test_statistics_node_tables(hip_lib, sizes, form):
    from mtgs_amd.densify import update_statistics, update_statistics_all
    W, H = STATS_WH
    stats, frames = stats_inputs(sizes, seed=sum(sizes) + len(sizes))
    ref = _stats_reference(sizes, stats, frames)
    dev = [[t.cuda() for t in s] for s in stats]
    for radii, grad in frames:
        if form == "batch":
            update_statistics_all([tuple(s) for s in dev], radii.cuda(), grad.cuda(), W, H)
        else:
            start = 0
            for s, n in zip(dev, sizes):
                update_statistics(*s, radii.cuda(), grad.cuda(), W, H, start=start)
                start += n
    _assert_stats(dev, ref)


STATS_ROWS_SIZES = [0, 255, 0, 0, 256, 1, 257, 0]      # zero-size nodes at the front, in the middle (twice) and at the end
STATS_ROWS_PREFIX, STATS_ROWS_SUFFIX = 100, 50        # Gaussians of no listed node in front of the first and behind the last


def stats_rows_inputs(seed=5):
    """A hand-built frame in the compact form: rows [capacity, 16] with the gradient in columns 0-1 and the absgrad in 2-3,
    vis_ids a shuffled subset of ALL flat indices (some in the static prefix, some behind the last node), a device count
    smaller than the capacity."""
    g = torch.Generator().manual_seed(seed)
    sizes = STATS_ROWS_SIZES
    starts = (STATS_ROWS_PREFIX + np.cumsum([0] + sizes)[:-1]).tolist()
    N = STATS_ROWS_PREFIX + sum(sizes) + STATS_ROWS_SUFFIX
    capacity = N // 2
    count = capacity - 70
    vis_ids = torch.randperm(N, generator=g)[:capacity].int()
    rows = torch.randn(capacity, 16, generator=g) * 1e-3
    radii = torch.randint(1, 40, (1, N), generator=g).int()
    flat = [torch.rand(N, generator=g), torch.ones(N) + torch.randint(0, 5, (N,), generator=g).float(), torch.rand(N, generator=g) * 30]
    return sizes, starts, N, capacity, count, vis_ids, rows, radii, flat


@pytest.mark.parametrize("col", [0, 2])
def test_statistics_rows_by_hand(hip_lib, col):
    """The three statistics live in one buffer each that covers EVERY Gaussian of the frame; the listed nodes are slices of
    it.  The whole buffers are compared: rows at or beyond the device count, and ids in front of the first or behind the
    last listed node, leave them untouched bit for bit.  The device count sits in the high 32 bits of the packed word (the
    low half holds another number)."""
    from mtgs_amd.densify import update_statistics_rows
    W, H = STATS_WH
    sizes, starts, N, capacity, count, vis_ids, rows, radii, flat = stats_rows_inputs()
    ids = vis_ids[:count].long()
    assert int((ids < STATS_ROWS_PREFIX).sum()) > 5 and int((ids >= starts[-1] + sizes[-1]).sum()) > 5 and count < capacity
    ref = [t.double() for t in flat]
    R.stats_ref_rows([[t[st:st + n] for t in ref] for st, n in zip(starts, sizes)], starts, radii, rows, vis_ids, W, H, col, count)
    dev = [t.cuda() for t in flat]
    packed = torch.tensor([(count << 32) | 0x00ABCDEF], dtype=torch.int64, device="cuda")
    update_statistics_rows([tuple(t[st:st + n] for t in dev) for st, n in zip(starts, sizes)], radii.cuda(), rows.cuda(),
                           vis_ids.cuda(), W, H, starts=starts, absgrad=(col == 2), n_vis=capacity, n_vis_dev=packed)
    outside = torch.ones(N, dtype=torch.bool)             # Gaussians of no listed node
    outside[starts[0]:starts[-1] + sizes[-1]] = False
    touched = torch.zeros(N, dtype=torch.bool)
    touched[ids] = True
    unchanged = outside | ~touched                        # (rows at or beyond the count hold valid ids of their own: ignored)
    assert int((~touched)[vis_ids[count:].long()].sum()) == capacity - count
    for a, b, src, name in zip(dev, ref, flat, ("xys_grad_norm", "vis_counts", "max_2Dsize")):
        a = a.cpu()
        assert torch.equal(bits(a[unchanged]), bits(src[unchanged])), name
        if name == "xys_grad_norm":
            assert torch.allclose(a.double(), b, rtol=1e-6, atol=1e-7), name
        else:
            assert torch.equal(a.double(), b), name
    inside = touched & ~outside
    assert int(inside.sum()) > 100 and bool((dev[1].cpu()[inside] == flat[1][inside] + 1).all())


# ---- refinement -----------------------------------------------------------------------------------------------------------------
# refine.hip: one thread per Gaussian, 256 per block; the flag byte holds bit 0 (old row kept), bits 1 .. S (children),
# bit 1 + S (duplicate), bit 7 (split parent), and `kind` / the Philox slot follow the same numbering.
REFINE_STEP, REFINE_SEED = 4000, 1234567


# one seed per case: the first of its sequence that meets the conditioning check of refine_margin (tests/test_node_refs_host.py)
REFINE_SEEDS = {'mixed-S1-clone': 11,
 'mixed-S1-copy': 210,
 'mixed-S2-clone': 21,
 'mixed-S2-copy': 120,
 'mixed-S3-clone': 131,
 'mixed-S3-copy': 1130,
 'mixed-S4-clone': 341,
 'mixed-S4-copy': 140,
 'N1-S2': 3,
 'N1-S4': 5,
 'N2-S2': 4,
 'N2-S4': 6,
 'N255-S2': 657,
 'N255-S4': 559,
 'N256-S2': 458,
 'N256-S4': 260,
 'N257-S2': 259,
 'N257-S4': 261,
 'same-S2': 109,
 'same-S3': 10,
 'split-S2': 109,
 'split-S3': 10,
 'culled-S2': 109,
 'culled-S3': 110,
 'dups-S2': 109,
 'dups-S3': 10,
 'viszero-S2': 3,
 'viszero-S4': 4}


def _case(name, N, S, clone=True, regime="mixed"):
    return dict(name=name, N=N, S=S, clone=clone, regime=regime, seed=REFINE_SEEDS[name])


REFINE_CASES = (
    [_case(f"mixed-S{S}-{'clone' if c else 'copy'}", 1000, S, c) for S in (1, 2, 3, 4) for c in (True, False)]
    + [_case(f"N{N}-S{S}", N, S) for N in (1, 2, 255, 256, 257) for S in (2, 4)]
    + [_case(f"{r}-S{S}", 300, S, regime=r) for r in ("same", "split", "culled", "dups") for S in (2, 3)]
    + [_case("viszero-S2", 300, 2, regime="viszero"), _case("viszero-S4", 300, 4, regime="viszero")]
)
REFINE_BY_NAME = {c["name"]: c for c in REFINE_CASES}


def refine_cfg(case):
    from mtgs_amd.densify import RefineConfig
    return RefineConfig(n_split_samples=case["S"], clone_sample_means=case["clone"], stop_split_at=20000)


def refine_inputs(case):
    """params, stats = (xys_grad_norm, vis_counts, max_2Dsize), moments: float32 CPU tensors.
    mixed: every rule of step 4000 fires (scales of two populations so that children die of their size and duplicates exist,
    means beyond |x| = 100, opacities below the cull limit, screen sizes beyond both limits).
    same: nothing is split, duplicated or culled.  split: every Gaussian is split, some children die.  culled: opacity logits
    about -12.  dups: every Gaussian is duplicated, nothing else.  viszero: mixed with vis_counts = 0 rows, with and without
    an accumulated gradient (x / 0 = +inf compares true, 0 / 0 = NaN compares false, as in NumPy)."""
    N, regime = case["N"], case["regime"]
    g = torch.Generator().manual_seed(1000 + case["seed"])
    U = lambda *s: torch.rand(*s, generator=g)
    span = torch.where(U(N, 1) < 0.5, torch.tensor(0.25), torch.tensor(1.3))
    p = {"means": (U(N, 3) * 2 - 1) * torch.tensor([60.0, 8.0, 140.0]), "scales": torch.log(U(N, 3) * span + 0.01),
         "quats": torch.randn(N, 4, generator=g) * 1.7, "opacities": torch.randn(N, 1, generator=g) * 3.0,
         "features_dc": torch.randn(N, 3, generator=g), "features_rest": torch.randn(N, 2, 3, generator=g)}
    gn, vc, m2 = U(N) * 0.028, torch.randint(1, 12, (N,), generator=g).float(), U(N) * 180.0
    if regime in ("same", "split", "dups"):
        m2 = U(N) * 90.0
        p["opacities"] = U(N, 1) * 6 - 2
    if regime == "same":
        gn, p["scales"] = U(N) * 0.0005, torch.log(U(N, 3) * 0.3 + 0.01)
    elif regime == "split":
        gn, p["scales"], p["opacities"] = (2 + U(N)) * 0.01 * vc, torch.log(U(N, 3) * 0.8 + 0.4), torch.randn(N, 1, generator=g) * 3.0
    elif regime == "dups":
        gn, p["scales"] = (2 + U(N)) * 0.01 * vc, torch.log(U(N, 3) * 0.15 + 0.01)
    elif regime == "culled":
        p["opacities"] = -12 + U(N, 1) * 0.5
    elif regime == "viszero":
        vc[::5] = 0
        gn[::10] = 0
    else:
        assert regime == "mixed", regime
    moments = {k: (torch.randn(v.shape, generator=g), torch.rand(v.shape, generator=g)) for k, v in p.items()}
    return p, (gn, vc, m2), moments


_refine_oracle = {}


def refine_oracle(case):
    """(inputs, oracle result) of a case, computed once."""
    from oracle import refine_oracle as ro
    if case["name"] not in _refine_oracle:
        p, stats, moments = refine_inputs(case)
        with np.errstate(divide="ignore", invalid="ignore"):
            ref = ro.refinement_after({k: v.numpy() for k, v in p.items()}, tuple(s.numpy() for s in stats), refine_cfg(case), REFINE_STEP,
                                      lambda idx, slot: ro.normals3(REFINE_SEED, REFINE_STEP, idx, slot),
                                      moments={k: (a.numpy(), b.numpy()) for k, (a, b) in moments.items()})
        _refine_oracle[case["name"]] = ((p, stats, moments), ref)
    return _refine_oracle[case["name"]]


def refine_margin(case):
    """The input-conditioning check: the smallest relative distance of any statistic from the threshold refinement_after
    compares it with, in float64 -- the grad average, max exp(scales) before and after the / 1.6 shrink against the densify and
    the cull limits, sigmoid(opacity), |mean| of every old row, child and duplicate against 100, max_2Dsize against both screen
    sizes.  A NaN average (0 / 0) compares false whatever the threshold and is left out."""
    (p, stats, _), (_, _, masks) = refine_oracle(case)
    cfg = refine_cfg(case)
    assert REFINE_STEP > cfg.refine_every * cfg.reset_alpha_every and REFINE_STEP < cfg.stop_screen_size_at     # every rule is on
    gn, vc, m2 = (s.numpy().astype(np.float64) for s in stats)
    with np.errstate(divide="ignore", invalid="ignore"):
        avg = gn / vc
    mx = np.exp(p["scales"].numpy().astype(np.float64)).max(-1)
    cand = masks["candidates"]
    cs = np.exp(cand["scales"]).max(-1)
    alpha = 1.0 / (1.0 + np.exp(-p["opacities"].numpy().astype(np.float64).reshape(-1)))
    tests = [(avg[~np.isnan(avg)], cfg.densify_grad_thresh), (mx, cfg.densify_size_thresh), (mx / 1.6, cfg.densify_size_thresh),
             (alpha, cfg.cull_alpha_thresh), (np.linalg.norm(cand["means"], axis=-1), 100.0),
             (m2, cfg.split_screen_size), (m2, cfg.cull_screen_size)]
    for s in (mx, mx / 1.6, cs):
        tests += [(s, cfg.cull_scale_thresh), (s, 40.0 * cfg.cull_scale_thresh)]
    worst = np.inf
    for x, thr in tests:
        x = x[np.isfinite(x)]
        if x.size:
            worst = min(worst, float((np.abs(x - thr) / thr).min()))
    return worst


def refine_counts(case):
    """How often each branch is taken, from the oracle's masks."""
    (p, _, _), (_, _, masks) = refine_oracle(case)
    N, S = case["N"], case["S"]
    keep, splits, dups = masks["keep"], masks["splits"], masks["dups"]
    n_sp, n_du = int(splits.sum()), int(dups.sum())
    return dict(splits=n_sp, dups=n_du, culled_parents=int((~keep[:N] & splits).sum()), culled_old=int((~keep[:N] & ~splits).sum()),
                culled_children=int((~keep[N:N + S * n_sp]).sum()), culled_dups=int((~keep[N + S * n_sp:]).sum()),
                kept_old=int(keep[:N].sum()), kept_children=int(keep[N:N + S * n_sp].sum()), kept_dups=int(keep[N + S * n_sp:].sum()))


def refine_parents(case):
    """bool [N]: the Gaussians with a kept child or a kept duplicate."""
    _, (_, _, masks) = refine_oracle(case)
    m = np.zeros(case["N"], dtype=bool)
    m[masks["src_index"][masks["kind"] > 0]] = True
    return m


def _run_refine(case, **kw):
    from mtgs_amd.densify import refine_gaussians
    (p, stats, moments), _ = refine_oracle(case)
    return refine_gaussians({k: v.cuda() for k, v in p.items()}, tuple(s.cuda() for s in stats), refine_cfg(case), REFINE_STEP, REFINE_SEED,
                            moments={k: (a.cuda(), b.cuda()) for k, (a, b) in moments.items()}, **kw)


def _check_refine(case):
    """The criterion of test_gpu_densify.py: src_index, kind, n_after, n_split identical; rows within 2e-5 (means) / 2e-6 of
    max(1, |ref|); moments bit-exact."""
    (p, _, _), (ref, ref_m, masks) = refine_oracle(case)
    new, new_m, info = _run_refine(case)
    cnt = refine_counts(case)
    n_ref = ref["means"].shape[0]
    assert info["n_before"] == case["N"] and info["n_after"] == n_ref, (info["n_after"], n_ref)
    assert (info["n_old_kept"], info["n_children"], info["n_dups"]) == (cnt["kept_old"], cnt["kept_children"], cnt["kept_dups"])
    assert int(info["n_split"]) == cnt["splits"]
    assert info["src_index"].shape == (n_ref,) and info["kind"].shape == (n_ref,)
    assert np.array_equal(info["src_index"].cpu().numpy(), masks["src_index"]) and np.array_equal(info["kind"].cpu().numpy(), masks["kind"])
    for k in ref:
        got = new[k].cpu().numpy().astype(np.float64)
        assert got.shape == ref[k].shape == (n_ref,) + tuple(p[k].shape[1:]), (k, got.shape)
        tol = 2e-5 if k == "means" else 2e-6
        if n_ref:
            assert np.abs(got - ref[k]).max() <= tol * max(1.0, np.abs(ref[k]).max()), (k, np.abs(got - ref[k]).max())
        for j in (0, 1):
            gm = new_m[k][j].cpu().numpy()
            assert gm.shape == ref[k].shape and np.array_equal(gm.view(np.int32), ref_m[k][j].astype(np.float32).view(np.int32)), (k, j)
    return new, new_m, info


@pytest.mark.parametrize("name", [c["name"] for c in REFINE_CASES])
def test_refinement_edges(hip_lib, name):
    case = REFINE_BY_NAME[name]
    N, S, regime = case["N"], case["S"], case["regime"]
    (p, stats, moments), (ref, _, masks) = refine_oracle(case)
    cnt = refine_counts(case)
    if regime == "mixed" and N == 1000:      # every branch and every flag bit is used
        assert min(cnt[k] for k in ("splits", "dups", "culled_parents", "culled_children", "culled_old")) > 20, cnt
        assert set(np.unique(masks["kind"])) == set(range(2 + S))
    new, new_m, info = _check_refine(case)
    if regime == "same":
        assert info["n_after"] == N and not bool(info["kind"].any()) and torch.equal(info["src_index"].cpu(), torch.arange(N, dtype=torch.int32))
        for k in p:
            assert torch.equal(bits(new[k]), bits(p[k])), k
            for j in (0, 1):
                assert torch.equal(bits(new_m[k][j]), bits(moments[k][j])), (k, j)
    elif regime == "split":
        assert cnt["splits"] == N and cnt["kept_old"] == 0 and cnt["dups"] == 0 and 0 < cnt["culled_children"] < S * N
        assert info["n_after"] == info["n_children"] == S * N - cnt["culled_children"]
        kind = info["kind"].cpu().numpy().astype(np.int64)
        src = info["src_index"].cpu().numpy()
        assert kind.min() >= 1 and (np.diff(kind) >= 0).all()                                    # sample-major
        assert all((np.diff(src[kind == 1 + s]) > 0).all() for s in range(S))                    # parents in order within a sample
    elif regime == "culled":
        assert info["n_after"] == 0 and info["src_index"].shape == (0,) and info["kind"].shape == (0,)
        for k in p:
            assert new[k].shape == (0,) + tuple(p[k].shape[1:]) and new_m[k][0].shape == new[k].shape == new_m[k][1].shape, k
    elif regime == "dups":
        assert cnt["splits"] == 0 and cnt["dups"] == N == cnt["kept_dups"] == cnt["kept_old"] and info["n_after"] == 2 * N
        assert torch.equal(info["kind"].cpu(), torch.cat([torch.zeros(N), torch.full((N,), 1.0 + S)]).to(torch.uint8))
    elif regime == "viszero":
        gn, vc, _ = (s.numpy() for s in stats)
        inf_rows, nan_rows = (vc == 0) & (gn > 0), (vc == 0) & (gn == 0)
        assert inf_rows.sum() > 20 and nan_rows.sum() > 20
        # +inf > threshold: split or duplicated, whichever the scales say; NaN > threshold is false: neither (screen-size splits aside)
        assert (masks["splits"] | masks["dups"])[inf_rows].all() and not masks["dups"][nan_rows].any()
        assert not (masks["splits"][nan_rows] & (stats[2].numpy()[nan_rows] <= 100.0)).any()


def test_refinement_moves_extras_and_calls_the_hook_once(hip_lib):
    """extras: 4-byte rows follow their parent bit for bit (the patterns of NaN and -0.0 among them); before_rows: one call,
    with the Gaussians that have a kept child or duplicate."""
    case = REFINE_BY_NAME["mixed-S3-clone"]
    N = case["N"]
    g = torch.Generator().manual_seed(2)
    e1 = torch.randint(-2 ** 31, 2 ** 31 - 1, (N,), generator=g, dtype=torch.int64).to(torch.int32)
    e2 = torch.randint(-2 ** 31, 2 ** 31 - 1, (N, 2), generator=g, dtype=torch.int64).to(torch.int32)
    special = torch.tensor([0x7FC00000, -0x80000000, 0x7F800001, -1], dtype=torch.int64).to(torch.int32)   # NaN, -0.0, sNaN, NaN
    e1[:400] = special.repeat(100)
    e2[:400, 1] = special.repeat(100)
    calls = []
    _, _, info = _run_refine(case, extras={"a": e1.cuda(), "b": e2.cuda()}, before_rows=lambda m: calls.append(m.clone()))
    src = info["src_index"].cpu().long()
    assert info["n_after"] > N and int((src < 400).sum()) > 100
    assert info["extras"]["a"].dtype == torch.int32 and torch.equal(info["extras"]["a"].cpu(), e1[src])
    assert info["extras"]["b"].dtype == torch.int32 and torch.equal(info["extras"]["b"].cpu(), e2[src])
    assert len(calls) == 1 and calls[0].dtype == torch.bool and calls[0].shape == (N,)
    want = refine_parents(case)
    assert 20 < want.sum() < N and np.array_equal(calls[0].cpu().numpy(), want)


@pytest.mark.parametrize("S", [0, 5])
@pytest.mark.parametrize("hook", [False, True])
def test_refinement_refuses_unsupported_sample_counts(hip_lib, S, hook):
    from mtgs_amd.densify import RefineConfig, refine_gaussians
    p, stats, _ = refine_inputs(REFINE_BY_NAME["N257-S2"])
    calls = []
    with pytest.raises(RuntimeError, match="n_split_samples"):
        refine_gaussians({k: v.cuda() for k, v in p.items()}, tuple(s.cuda() for s in stats), RefineConfig(n_split_samples=S),
                         REFINE_STEP, REFINE_SEED, before_rows=calls.append if hook else None)
    assert not calls


# ---- out-of-box regulariser -----------------------------------------------------------------------------------------------------
# oob.hip: OOB_BLOCK = 256 Gaussians per block, a block's node by binary search over first_block (a node of size 0 shares it with
# its successor), the visibility of a node from a ballot per wave.
OOB_SIZE = [2.5, 1.5, 4.0]
OOB_TOL = 1.5
OOB_SEEDS = {"256": 1}            # (a case whose default seed puts a coordinate within 1e-4 of its limit gets another one here)
OOB_CASES = ["256", "257", "1-0-1", "0-300", "300-0", "40x1", "inside", "outside", "last_lane"]


def oob_inputs(name):
    """nodes [(local means [n,3], opacity logits [n,1], size)], radii [1,N] int32, starts."""
    g = torch.Generator().manual_seed(OOB_SEEDS.get(name, 0) + sum(map(ord, name)))
    limit = torch.tensor([s / 2 + OOB_TOL for s in OOB_SIZE])
    sizes = {"40x1": [1] * 40, "inside": [257, 64], "outside": [257, 64], "last_lane": [257, 300, 129]}.get(name)
    if sizes is None:
        sizes = [int(s) for s in name.split("-")]
    starts, s = [], 11
    for k in sizes:
        starts.append(s)
        s += k
    total = s + 5
    nodes = [(torch.randn(k, 3, generator=g) * 2.0, torch.randn(k, 1, generator=g) * 2, OOB_SIZE) for k in sizes]
    radii = (torch.randint(1, 30, (1, total), generator=g) * (torch.rand(1, total, generator=g) < 0.5)).int()
    if name in ("1-0-1", "40x1"):    # nodes of one Gaussian: all visible, most out of their box
        radii = torch.randint(1, 30, (1, total), generator=g).int()
        nodes = [(m * 2.5, o, sz) for m, o, sz in nodes]
    if name == "inside":
        nodes = [((torch.rand(k, 3, generator=g) * 2 - 1) * limit * 0.9, o, sz) for (_, o, sz), k in zip(nodes, sizes)]
    elif name == "outside":          # every Gaussian beyond its box on some axis; the two ends of -log(1 - s + 1e-6)
        nodes = [(m + torch.sign(m) * limit, torch.where(torch.arange(k)[:, None] % 2 == 0, 8.0, -8.0), sz) for (m, _, sz), k in zip(nodes, sizes)]
    elif name == "last_lane":        # nodes 0 and 2: only their last Gaussian is visible (thread 0 of the second block / lane 0 of the third wave); node 1: none
        radii[:] = 0
        radii[0, starts[0] + 256] = 3
        radii[0, starts[2] + 128] = 1
    return nodes, radii, starts


def oob_margin(nodes):
    """The smallest relative distance of any |coordinate| from its limit."""
    worst = np.inf
    for means, _, size in nodes:
        limit = np.array([float(s) / 2 + OOB_TOL for s in size])
        if means.shape[0]:
            worst = min(worst, float((np.abs(np.abs(means.numpy().astype(np.float64)) - limit) / limit).min()))
    return worst


@pytest.mark.parametrize("name", OOB_CASES)
def test_oob_loss_node_edges(hip_lib, name):
    """Value 2e-5 * max(1, |ref|), gradients rtol 2e-4 atol 1e-7 (test_gpu_loss.py).  Nothing out of its box: exactly 0 with
    gradients that are exactly zero; a node without a visible Gaussian: a gradient that is exactly zero."""
    from mtgs_amd.loss import oob_loss
    nodes, radii, starts = oob_inputs(name)
    ref, g_ref = R.oob_ref(nodes, radii, starts, tolerance=OOB_TOL)
    P = [o.cuda().requires_grad_(True) for _, o, _ in nodes]
    val = oob_loss([(m.cuda(), p, size) for (m, _, size), p in zip(nodes, P)], radii.cuda(), starts, tolerance=OOB_TOL)
    (3.0 * val).backward()
    got = float(val.detach())
    assert not np.isnan(got) and abs(got - float(ref)) <= 2e-5 * max(1.0, abs(float(ref))), (got, float(ref))
    visible = [bool((radii[0, st:st + m.shape[0]] > 0).any()) for (m, _, _), st in zip(nodes, starts)]
    for p, gr, (m, o, _), vis in zip(P, g_ref, nodes, visible):
        assert p.grad.shape == o.shape and not bool(torch.isnan(p.grad).any())
        assert torch.allclose(p.grad.cpu().double(), 3.0 * gr, rtol=2e-4, atol=1e-7), float((p.grad.cpu().double() - 3.0 * gr).abs().max())
        if not vis or name == "inside":
            assert torch.equal(p.grad.cpu(), torch.zeros_like(o))
    if name == "inside":
        assert got == 0.0 and float(ref) == 0.0
    else:
        assert float(ref) > 0
    if name == "last_lane":
        assert visible == [True, False, True] and float(g_ref[0].abs().max()) > 0 and float(g_ref[2].abs().max()) > 0
    if name == "outside":
        assert all(bool((gr != 0).all()) for gr in g_ref)
